"""Module CORE with per-level point counts, fused against unfused, forward and forward + backward, in one process and
alternated:   python tools/fused_ragged_bench.py [--out profiles/NAME.json] [--repeats 7] [--iters 50]

"fused"   fused_module_core(..., points_per_level=)  — msda_{fwd,bwd}_fused_ragged_<suffix>
"unfused" the prologue as plain PyTorch ops (ragged_module_sampling_inputs) + multiscale_deformable_attention(...,
          points_per_level=): what a user had to write before the fused pair existed; it is the baseline.
Shapes: D-FINE 640 (B = 8, Q = 300, H = 8, D = 32, 80x80 / 40x40 / 20x20, [3, 6, 3], 4-d reference boxes) in fp32 and with
bf16 storage (value + projection), and c2 @ 10 000 queries with [2, 4, 6, 4], fp32.  Per leg: `repeats` timed runs of
`iters` calls each between two events after a warm-up; the median and the min / max of the per-call times are reported."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from msda_triton_amd import multiscale_deformable_attention, synth
from msda_triton_amd.functional import fused_module_core
from msda_triton_amd.ragged import ragged_module_sampling_inputs

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--iters", type=int, default=50)
a = ap.parse_args()
dev = torch.device("cuda", 0)
c2 = synth.WORKLOADS["c2_q10k"]
CASES = [
    ("dfine640_fp32", 8, 300, 8, 32, [(80, 80), (40, 40), (20, 20)], [3, 6, 3], 4, torch.float32),
    ("dfine640_bf16_storage", 8, 300, 8, 32, [(80, 80), (40, 40), (20, 20)], [3, 6, 3], 4, torch.bfloat16),
    ("c2_q10k_fp32", c2.B, c2.Q, c2.H, c2.D, [tuple(l) for l in c2.levels], [2, 4, 6, 4], 2, torch.float32),
]


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters


results = []
for name, B, Q, H, D, levels, counts, rd, sdt in CASES:
    torch.manual_seed(0)
    shapes = torch.tensor(levels, device=dev)
    value = torch.randn(B, sum(h * w for h, w in levels), H, D, device=dev).to(sdt).requires_grad_()
    proj = (torch.randn(B, Q, H, sum(counts), 3, device=dev) * 1.5).to(sdt).requires_grad_()
    ref = torch.rand(B, Q, rd, device=dev)
    go = torch.randn(B, Q, H, D, device=dev).to(sdt)

    def fused():
        return fused_module_core(value, shapes, proj, ref, "zeros", False, levels, points_per_level=counts)

    def unfused():
        pts, att = ragged_module_sampling_inputs(proj.float(), shapes, ref, counts)
        out = multiscale_deformable_attention(value, shapes, pts, att, "zeros", False, level_shapes=levels,
                                              points_per_level=counts)
        return out.to(sdt)

    def step(f):
        def run():
            f().backward(go)
            value.grad = proj.grad = None
        return run

    def fwd(f):
        def run():
            with torch.no_grad():
                f()
        return run

    legs = {"fused_fwd": fwd(fused), "unfused_fwd": fwd(unfused), "fused_fwd_bwd": step(fused), "unfused_fwd_bwd": step(unfused)}
    times = {k: [] for k in legs}
    for f in legs.values():
        for _ in range(20):
            f()
    torch.cuda.synchronize()
    for _ in range(a.repeats):  # alternated: every repeat visits every leg
        for k, f in legs.items():
            times[k].append(timed(f, a.iters))
    row = {"case": name, "B": B, "Q": Q, "H": H, "D": D, "levels": levels, "points_per_level": counts, "ref_dim": rd,
           "storage": str(sdt).replace("torch.", ""), "repeats": a.repeats, "iters": a.iters, "unit": "ms per call"}
    for k, v in times.items():
        row[k] = {"median": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5)}
    for kind in ("fwd", "fwd_bwd"):
        row[f"speedup_{kind}"] = round(row[f"unfused_{kind}"]["median"] / row[f"fused_{kind}"]["median"], 3)
    results.append(row)
    print(json.dumps(row), flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "results": results}, f, indent=1)
