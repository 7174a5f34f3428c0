"""The deformable convolution core: the gfx950 kernels against what a user has without them, one process, alternated:
    python tools/dcn_bench.py [--out profiles/NAME.json] [--repeats 7] [--iters 20]

"window" / "direct"  deformable_conv_core(...) — msda_dcn_{fwd,bwd}_<dtype> with option "dcn_window" 1 / 0
"composition"        the PyTorch prologue — sampling_points [N, Ho Wo, G, 1, K, 2] from the lattice, the taps and the
                     offsets, the softmax when it is on — around this package's own multiscale_deformable_attention(...,
                     padding_mode="zeros"): the yardstick.
Shapes: three backbone stages, N = 16, D = 16, 3 x 3, stride 1, pad 1 — 56 x 56 with G = 4, 28 x 28 with G = 8, 14 x 14 with
G = 16 — fp32 and bf16, softmax off; the first once more with softmax on.  Legs: forward (no grad) and forward + backward
(all three gradients).  Per leg `repeats` timed runs of `iters` calls between two events after a warm-up; every repeat
visits every leg.  Reported: median and min / max of the per-call times, and per kernel leg whether its slowest repeat is
below the composition's fastest ("ahead in every repeat") or not."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from msda_triton_amd import _lib, deformable_conv_core, multiscale_deformable_attention
from msda_triton_amd.dcn import last_launch_info

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--iters", type=int, default=20)
a = ap.parse_args()
assert torch.cuda.is_available(), "dcn_bench.py needs a GPU"
dev = torch.device("cuda", 0)
CASES = [(N, S, G, 16, dt, sm) for (N, S, G) in ((16, 56, 4), (16, 28, 8), (16, 14, 16)) for dt in (torch.float32, torch.bfloat16)
         for sm in (False,)] + [(16, 56, 4, 16, torch.float32, True), (16, 56, 4, 16, torch.bfloat16, True)]
KH = KW = 3
DEFAULT_WINDOW = _lib.get_option("dcn_window")


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
for N, S, G, D, dt, softmax in CASES:
    torch.manual_seed(0)
    K = KH * KW
    x = torch.randn(N, S, S, G, D, device=dev).to(dt).requires_grad_()
    offset = torch.randn(N, S, S, G, K, 2, device=dev).to(dt).requires_grad_()
    mask = torch.randn(N, S, S, G, K, device=dev).to(dt).requires_grad_()
    go = torch.randn(N, S, S, G, D, device=dev).to(dt)
    leaves = (x, offset, mask)
    shapes = torch.tensor([[S, S]], device=dev)
    k = torch.arange(K, device=dev)
    tap = torch.stack([(k // KH) - 1, (k % KH) - 1], -1).to(dt)                       # (x, y) of tap k, centre (1, 1) taken off
    pix = torch.stack(torch.meshgrid(torch.arange(S, device=dev), torch.arange(S, device=dev), indexing="ij")[::-1], -1).to(dt)
    size = torch.tensor([S, S], device=dev, dtype=dt)

    def kernels():
        return deformable_conv_core(x, offset, mask, 3, 1, 1, 1, 1.0, softmax)

    def composition():
        # lx = wo - 1 + 1 + (i - 1 + ox): the point ((lx + 0.5) / W, (ly + 0.5) / H), [N, Ho Wo, G, 1, K, 2]
        points = ((pix.view(1, S, S, 1, 1, 2) + tap + offset + 0.5) / size).view(N, S * S, G, 1, K, 2)
        m = (mask.softmax(-1) if softmax else mask).view(N, S * S, G, 1, K)
        out = multiscale_deformable_attention(x.view(N, S * S, G, D), shapes, points, m, "zeros", False, level_shapes=[(S, S)])
        return out.view(N, S, S, G, D)

    def with_window(on, f):
        def run():
            _lib.set_option("dcn_window", on)
            f()
        return run

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

    legs = {"window_fwd": with_window(1, fwd(kernels)), "direct_fwd": with_window(0, fwd(kernels)), "composition_fwd": fwd(composition),
            "window_fwd_bwd": with_window(1, step(kernels)), "direct_fwd_bwd": with_window(0, step(kernels)),
            "composition_fwd_bwd": step(composition)}
    with torch.no_grad():
        err = (kernels().float() - composition().float()).abs().max().item()
    times = {n: [] for n in legs}
    used = {}
    for n, f in legs.items():
        for _ in range(5):
            f()
        used[n] = last_launch_info()["dcn_window"] if "composition" not in n else None
    torch.cuda.synchronize()
    for _ in range(a.repeats):  # alternated: every repeat visits every leg
        for n, f in legs.items():
            times[n].append(timed(f, a.iters))
    row = {"case": f"N{N}_{S}x{S}_G{G}_D{D}_{str(dt).replace('torch.', '')}" + ("_softmax" if softmax else ""), "repeats": a.repeats,
           "iters": a.iters, "unit": "ms per call", "max_abs_diff_fwd": err, "window_staged": used}
    for n, v in times.items():
        row[n] = spread(v)
    for kind in ("fwd", "fwd_bwd"):
        cp = row[f"composition_{kind}"]
        for leg in ("window", "direct"):
            kr = row[f"{leg}_{kind}"]
            row[f"speedup_{leg}_{kind}"] = round(cp["median"] / kr["median"], 3)
            row[f"verdict_{leg}_{kind}"] = "kernels ahead in every repeat" if kr["max"] < cp["min"] else \
                ("composition ahead in every repeat" if cp["max"] < kr["min"] else "spreads overlap")
    results.append(row)
    print(json.dumps(row), flush=True)
    del x, offset, mask, go, leaves
_lib.set_option("dcn_window", DEFAULT_WINDOW)

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "results": results}, f, indent=1)
