"""Deformable feature aggregation: the gfx950 kernels against what a user has without them, one process, alternated:
    python tools/dfa_bench.py [--out profiles/NAME.json] [--repeats 7] [--iters 20]

"kernels"      deformable_aggregation(...) — msda_dfa_{fwd,bwd}_<dtype>
"composition"  the expansion into this package's own multiscale_deformable_attention(..., padding_mode="zeros") with
               L = cams * levels: the location broadcast over levels and groups, the validity mask multiplied into the
               weights — the yardstick.
Shape: Sparse4D-sized — A 900 anchors, P 13 key points, 6 cameras, 4 levels of 32 x 88 ... 4 x 11, C 256, G 8 — at B 1 and 6,
fp32 and bf16.  Locations are drawn so that a point is in view of one or two cameras: every point gets a home camera and,
with probability one half, a second; elsewhere it lies outside the image.  Legs: forward (no grad) and forward + backward (all
three gradients).  Per leg `repeats` timed runs of `iters` calls between two events after a warm-up; every repeat visits every
leg.  Reported: median and min / max of the per-call times, and whether the kernels' slowest repeat is below the
composition's fastest ("ahead in every repeat") or not."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from msda_triton_amd import _lib, deformable_aggregation, multiscale_deformable_attention

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--iters", type=int, default=20)
a = ap.parse_args()
assert torch.cuda.is_available(), "dfa_bench.py needs a GPU"
dev = torch.device("cuda", 0)
A, P, CAMS, G, D = 900, 13, 6, 8, 32
LEVELS = [(32, 88), (16, 44), (8, 22), (4, 11)]
CASES = [(B, dt) for B in (1, 6) for dt in (torch.float32, torch.bfloat16)]


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters


def spread(v):
    return {"median": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5)}


results = []
for B, dt in CASES:
    torch.manual_seed(0)
    nl = len(LEVELS)
    shapes = torch.tensor([LEVELS] * CAMS, device=dev)
    I = CAMS * sum(h * w for h, w in LEVELS)  # noqa: E741
    home = torch.randint(0, CAMS, (B, A, P), device=dev)
    second = (home + 1) % CAMS
    cams = torch.arange(CAMS, device=dev)
    in_view = (cams == home[..., None]) | ((cams == second[..., None]) & (torch.rand(B, A, P, 1, device=dev) < 0.5))
    loc = torch.where(in_view[..., None], torch.rand(B, A, P, CAMS, 2, device=dev) * 0.98 + 0.01,
                      1.05 + torch.rand(B, A, P, CAMS, 2, device=dev)).to(dt).requires_grad_()
    fm = torch.randn(B, I, G, D, device=dev).to(dt).requires_grad_()
    wts = torch.rand(B, A, P, CAMS, nl, G, device=dev).to(dt).requires_grad_()
    go = torch.randn(B, A, G, D, device=dev).to(dt)
    leaves = (fm, loc, wts)
    level_shapes = LEVELS * CAMS

    def kernels():
        return deformable_aggregation(fm, shapes, loc, wts)

    def composition():
        valid = ((loc > 0) & (loc < 1)).all(-1).to(dt)
        points = loc.permute(0, 1, 3, 2, 4)[:, :, None, :, None].expand(B, A, G, CAMS, nl, P, 2).reshape(B, A, G, CAMS * nl, P, 2)
        attn = (wts * valid[..., None, None]).permute(0, 1, 5, 3, 4, 2).reshape(B, A, G, CAMS * nl, P)
        return multiscale_deformable_attention(fm, shapes.view(-1, 2), points, attn, "zeros", False, level_shapes=level_shapes)

    def step(f):
        def run():
            f().backward(go)
            for t in leaves:
                t.grad = None
        return run

    def fwd(f):
        def run():
            with torch.no_grad():
                f()
        return run

    legs = {"kernels_fwd": fwd(kernels), "composition_fwd": fwd(composition), "kernels_fwd_bwd": step(kernels),
            "composition_fwd_bwd": step(composition)}
    with torch.no_grad():
        err = (kernels().float() - composition().float()).abs().max().item()
    times = {n: [] for n in legs}
    info = {}
    for n, f in legs.items():
        for _ in range(5):
            f()
        if n.startswith("kernels"):
            li = _lib.last_launch_info()
            info[n] = {k: li[k] for k in ("fwd_variant", "sample_variant", "fwd_trips", "sample_trips", "value_path")}
    torch.cuda.synchronize()
    for _ in range(a.repeats):  # alternated: every repeat visits every leg
        for n, f in legs.items():
            times[n].append(timed(f, a.iters))
    row = {"case": f"B{B}_A{A}_P{P}_cams{CAMS}_levels{nl}_C{G * D}_G{G}_{str(dt).replace('torch.', '')}", "repeats": a.repeats,
           "iters": a.iters, "unit": "ms per call", "max_abs_diff_fwd": err, "pairs_in_view": round(in_view.float().mean().item(), 4),
           "launch_info": info}
    for n, v in times.items():
        row[n] = spread(v)
    for kind in ("fwd", "fwd_bwd"):
        cp, kr = row[f"composition_{kind}"], row[f"kernels_{kind}"]
        row[f"speedup_{kind}"] = round(cp["median"] / kr["median"], 3)
        row[f"verdict_{kind}"] = "kernels ahead in every repeat" if kr["max"] < cp["min"] else \
            ("composition ahead in every repeat" if cp["max"] < kr["min"] else "spreads overlap")
    results.append(row)
    print(json.dumps(row), flush=True)
    del fm, loc, wts, go, leaves

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "results": results}, f, indent=1)
