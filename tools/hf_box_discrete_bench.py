"""The fused box prologue in front of DISCRETE sampling (D-FINE / DEIMv2 / RT-DETRv2 with decoder_method="discrete")
against the parent route, in one process and alternated:
    python tools/hf_box_discrete_bench.py [--out profiles/r14_hf_box_discrete_bench.json] [--repeats 7] [--iters 50]
                                          [--steps 10] [--no-model]

"fused"  fused_hf_box_core(..., sampling_mode="discrete")  — msda_{fwd,bwd}_fused_hfbox_discrete_<suffix>
"parent" transformers' prologue as plain PyTorch ops (hf_box_sampling_inputs) + multiscale_deformable_attention(...,
         points_per_level=, sampling_mode="discrete"): what `replace_hf_msda(model, discrete=True)` gives these models; it
         is the yardstick.
Core legs: D-FINE 640 (B = 8, Q = 300, H = 8, D = 32, 80x80 / 40x40 / 20x20, [3, 6, 3]) in fp32 and with bf16 storage
(value + projection next to fp32 boxes: what autocast hands the core), and RT-DETRv2 640 ([4, 4, 4]) in fp32.  Model leg:
one training step of a default-config DFineModel with decoder_method="discrete" at 640 x 640, B = 8,
`replace_hf_msda(model, discrete=True)` against `replace_hf_msda(model, fused=True, discrete=True, fuse_discrete=True)` — two models with the
same weights, alternated.  Per leg: `repeats` timed runs of `iters` calls (`steps` training steps) between two events
after a warm-up; the median and the min / max of the per-call times are reported.  A leg is "ahead" only where its SLOWEST
repeat is below the other leg's FASTEST."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from msda_triton_amd import multiscale_deformable_attention
from msda_triton_amd.functional import fused_hf_box_core, hf_box_sampling_inputs

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--no-model", action="store_true")
a = ap.parse_args()
torch.set_num_threads(min(16, torch.get_num_threads()))  # (the host threads the machine grants a job)
dev = torch.device("cuda", 0)
L640 = [(80, 80), (40, 40), (20, 20)]
CASES = [
    ("dfine640_fp32", 8, 300, 8, 32, L640, [3, 6, 3], torch.float32),
    ("dfine640_bf16_storage", 8, 300, 8, 32, L640, [3, 6, 3], torch.bfloat16),
    ("rtdetrv2_640_fp32", 8, 300, 8, 32, L640, [4, 4, 4], torch.float32),
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


def verdict(fused, parent):
    if fused["max"] < parent["min"]:
        return "fused ahead"
    return "parent ahead" if parent["max"] < fused["min"] else "neither ahead"


results = []
for name, B, Q, H, D, levels, counts, sdt in CASES:
    torch.manual_seed(0)
    shapes = torch.tensor(levels, device=dev)
    value = torch.randn(B, sum(h * w for h, w in levels), H, D, device=dev).to(sdt).requires_grad_()
    proj = (torch.randn(B, Q, H, sum(counts), 3, device=dev) * 1.5).to(sdt).requires_grad_()
    ref = torch.rand(B, Q, 1, 4, device=dev)  # (the decoders detach their boxes)
    go = torch.randn(B, Q, H, D, device=dev).to(sdt)

    def fused():
        return fused_hf_box_core(value, shapes, proj, ref, counts, 0.5, level_shapes=levels, sampling_mode="discrete")

    def parent():
        pts, att = hf_box_sampling_inputs(proj.float(), ref, counts, 0.5)
        out = multiscale_deformable_attention(value, shapes, pts, att, "border", False, level_shapes=levels,
                                              points_per_level=counts, sampling_mode="discrete")
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

    legs = {"fused_fwd": fwd(fused), "parent_fwd": fwd(parent), "fused_fwd_bwd": step(fused), "parent_fwd_bwd": step(parent)}
    times = {k: [] for k in legs}
    for f in legs.values():
        for _ in range(20):
            f()
    torch.cuda.synchronize()
    for _ in range(a.repeats):  # alternated: every repeat visits every leg
        for k, f in legs.items():
            times[k].append(timed(f, a.iters))
    row = {"case": name, "B": B, "Q": Q, "H": H, "D": D, "levels": levels, "points_per_level": counts,
           "storage": str(sdt).replace("torch.", ""), "repeats": a.repeats, "iters": a.iters, "unit": "ms per call"}
    for k, v in times.items():
        row[k] = spread(v)
    for kind in ("fwd", "fwd_bwd"):
        row[f"ratio_{kind}"] = round(row[f"parent_{kind}"]["median"] / row[f"fused_{kind}"]["median"], 3)
        row[f"verdict_{kind}"] = verdict(row[f"fused_{kind}"], row[f"parent_{kind}"])
    results.append(row)
    print(json.dumps(row), flush=True)
    del value, proj, ref, go

if not a.no_model:
    import copy

    from transformers import DFineConfig, DFineModel

    from msda_triton_amd.hf_adapter import replace_hf_msda
    torch.manual_seed(0)
    base = DFineModel(DFineConfig(decoder_method="discrete")).to(dev).train()
    models = {"parent": base, "fused": copy.deepcopy(base)}
    n_parent = replace_hf_msda(models["parent"], discrete=True)
    n_fused = replace_hf_msda(models["fused"], fused=True, discrete=True, fuse_discrete=True)
    x = torch.randn(8, 3, 640, 640, device=dev)
    for autocast in (False, True):
        def train_step(m):
            def run():
                m.zero_grad(set_to_none=True)
                with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                    out = m(pixel_values=x)
                (out.last_hidden_state.float() ** 2).mean().backward()
            return run
        legs = {k: train_step(m) for k, m in models.items()}
        times = {k: [] for k in legs}
        for f in legs.values():
            for _ in range(2):
                f()
        torch.cuda.synchronize()
        for _ in range(a.repeats):
            for k, f in legs.items():
                times[k].append(timed(f, a.steps))
        row = {"case": "dfine_default_discrete_train_step_" + ("bf16_autocast" if autocast else "fp32"), "image": [640, 640],
               "batch": 8, "modules_patched": n_parent, "modules_patched_or_wrapped": n_fused, "repeats": a.repeats,
               "steps": a.steps, "unit": "ms per step (device time between events)"}
        for k, v in times.items():
            row[k] = spread(v)
        row["ratio"] = round(row["parent"]["median"] / row["fused"]["median"], 3)
        row["verdict"] = verdict(row["fused"], row["parent"])
        results.append(row)
        print(json.dumps(row), flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "results": results}, f, indent=1)
