"""Key-aware deformable attention: the gfx950 kernels against the composition a user has without them, one process, alternated:
    python tools/key_aware_bench.py [--out profiles/NAME.json] [--repeats 7] [--iters 20]

"kernels"      key_aware_deformable_attention(...)              — msda_keyaware_{fwd,bwd}_<dtype>
"composition"  native_key_aware_deformable_attention(...) on the same GPU tensors — per level one grid_sample on each
               pyramid, the scores, one softmax, the contraction: the file's own PyTorch formulation, the yardstick.
Shapes: c2 @ 10k (B = 4, Q = 10 000, H = 8, D = 32, the 64 x 64 pyramid, P = 4) and the decoder shape (B = 8, Q = 900, H = 8,
D = 32, L = 4, P = 4), fp32 and bf16 (the composition computes bf16 tensors in float32, as the function does for them).
Legs: forward (no grad) and forward + backward (all four gradients).  Per leg `repeats` timed runs of `iters` calls between
two events after a warm-up; every repeat visits every leg.  Reported: the median and min / max of the per-call times, and
whether the kernels' slowest repeat is below the composition's fastest ("ahead in every repeat") or not."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from msda_triton_amd import synth
from msda_triton_amd.key_aware import key_aware_deformable_attention, native_key_aware_deformable_attention

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--iters", type=int, default=20)
a = ap.parse_args()
assert torch.cuda.is_available(), "key_aware_bench.py needs a GPU"
dev = torch.device("cuda", 0)
c2, c4 = synth.WORKLOADS["c2_q10k"], synth.WORKLOADS["c4_gdino_dec"]
CASES = [(f"{w.name}_{str(dt).replace('torch.', '')}", w.B, w.Q, w.H, w.D, [tuple(l) for l in w.levels], w.P, dt)
         for w in (c2, c4) for dt in (torch.float32, torch.bfloat16)]


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
for name, B, Q, H, D, levels, P, dt in CASES:
    torch.manual_seed(0)
    L, I = len(levels), sum(h * w for h, w in levels)  # noqa: E741
    shapes = torch.tensor(levels, device=dev)
    query, key, value = (torch.randn(n, device=dev).to(dt).requires_grad_() for n in ((B, Q, H, D), (B, I, H, D), (B, I, H, D)))
    points = torch.rand(B, Q, H, L, P, 2, device=dev).to(dt).requires_grad_()
    go = torch.randn(B, Q, H, D, device=dev).to(dt)
    leaves = (query, key, value, points)

    def kernels():
        return key_aware_deformable_attention(query, key, value, shapes, points, "border", False, level_shapes=levels)

    def composition():
        return native_key_aware_deformable_attention(query, key, value, shapes, points, "border", False, D ** -0.5, levels)[0]

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
    times = {k: [] for k in legs}
    for f in legs.values():
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    for _ in range(a.repeats):  # alternated: every repeat visits every leg
        for k, f in legs.items():
            times[k].append(timed(f, a.iters))
    row = {"case": name, "B": B, "Q": Q, "H": H, "D": D, "levels": levels, "P": P, "dtype": str(dt).replace("torch.", ""),
           "sampled_key_bytes_fp32": B * Q * H * L * P * D * 4, "repeats": a.repeats, "iters": a.iters, "unit": "ms per call"}
    for k, v in times.items():
        row[k] = spread(v)
    for kind in ("fwd", "fwd_bwd"):
        kr, cp = row[f"kernels_{kind}"], row[f"composition_{kind}"]
        row[f"speedup_{kind}"] = round(cp["median"] / kr["median"], 3)
        row[f"verdict_{kind}"] = "kernels ahead in every repeat" if kr["max"] < cp["min"] else \
            ("composition ahead in every repeat" if cp["max"] < kr["min"] else "spreads overlap")
    results.append(row)
    print(json.dumps(row), flush=True)
    del query, key, value, points, go, leaves

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "results": results}, f, indent=1)
