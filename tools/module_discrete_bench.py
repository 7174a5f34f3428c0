"""The nn.Module's prologue in front of DISCRETE sampling — fused kernels against the composition, in one process and
alternated:
    python tools/module_discrete_bench.py [--out profiles/r16_module_discrete_bench.json] [--repeats 7] [--iters 50]

"fused"        fused_module_core(..., sampling_mode="discrete", fuse_discrete=True) — msda_{fwd,bwd}_fused_discrete_<suffix>
"composition"  ragged_module_sampling_inputs as plain PyTorch ops + multiscale_deformable_attention(..., points_per_level=,
               sampling_mode="discrete"): parts the parent commit has (it cannot build a discrete module at all); this is
               what fuse_discrete=False runs, and it is the yardstick.
Legs: the decoder shape of DESIGN.md 19 (B = 8, Q = 300, H = 8, D = 32, 80x80 / 40x40 / 20x20, num_points = [3, 6, 3]) with
a 4-d reference box, in fp32 and with bf16 value storage (value + projection in bf16 next to fp32 reference points: what
autocast hands the core), forward and forward + backward.  Per leg: `repeats` timed runs of `iters` calls between two
events after a warm-up; the median and the min / max of the per-call times are reported.  A leg is "ahead" only where its
SLOWEST repeat is below the other leg's FASTEST — the rule `module.DISCRETE_IN_KERNELS_DTYPES` is filled by."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from msda_triton_amd.functional import fused_module_core

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--iters", type=int, default=50)
a = ap.parse_args()
torch.set_num_threads(min(16, torch.get_num_threads()))  # (the host threads the machine grants a job)
dev = torch.device("cuda", 0)
L640 = [(80, 80), (40, 40), (20, 20)]
CASES = [
    ("decoder640_box_fp32", 8, 300, 8, 32, L640, [3, 6, 3], torch.float32),
    ("decoder640_box_bf16_storage", 8, 300, 8, 32, L640, [3, 6, 3], torch.bfloat16),
]


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


def verdict(fused, comp):
    if fused["max"] < comp["min"]:
        return "fused ahead"
    return "composition ahead" if comp["max"] < fused["min"] else "neither ahead"


results = []
for name, B, Q, H, D, levels, counts, sdt in CASES:
    torch.manual_seed(0)
    shapes = torch.tensor(levels, device=dev)
    value = torch.randn(B, sum(h * w for h, w in levels), H, D, device=dev).to(sdt).requires_grad_()
    proj = (torch.randn(B, Q, H, sum(counts), 3, device=dev) * 1.5).to(sdt).requires_grad_()
    ref = torch.rand(B, Q, 4, device=dev)
    go = torch.randn(B, Q, H, D, device=dev).to(sdt)

    def core(fuse):
        def call():
            return fused_module_core(value, shapes, proj, ref, "border", False, levels, points_per_level=counts,
                                     sampling_mode="discrete", fuse_discrete=fuse)
        return call

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

    legs = {"fused_fwd": fwd(core(True)), "composition_fwd": fwd(core(False)), "fused_fwd_bwd": step(core(True)),
            "composition_fwd_bwd": step(core(False))}
    times = {k: [] for k in legs}
    for f in legs.values():
        for _ in range(20):
            f()
    torch.cuda.synchronize()
    for _ in range(a.repeats):  # alternated: every repeat visits every leg
        for k, f in legs.items():
            times[k].append(timed(f, a.iters))
    row = {"case": name, "B": B, "Q": Q, "H": H, "D": D, "levels": levels, "points_per_level": counts, "ref_dim": 4,
           "storage": str(sdt).replace("torch.", ""), "repeats": a.repeats, "iters": a.iters, "unit": "ms per call"}
    for k, v in times.items():
        row[k] = spread(v)
    for kind in ("fwd", "fwd_bwd"):
        row[f"ratio_{kind}"] = round(row[f"composition_{kind}"]["median"] / row[f"fused_{kind}"]["median"], 3)
        row[f"verdict_{kind}"] = verdict(row[f"fused_{kind}"], row[f"composition_{kind}"])
    results.append(row)
    print(json.dumps(row), flush=True)
    del value, proj, ref, go
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "results": results}, f, indent=1)
