"""The fused prologue for Hugging Face attention modules against the unfused route, in one process and alternated:
    python tools/hf_fused_bench.py [--out profiles/NAME.json] [--repeats 7] [--iters 30] [--steps 3] [--no-model]

"fused"   fused_hf_module_core(...)  — msda_{fwd,bwd}_fused_levelref_<suffix>
"unfused" transformers' prologue as plain PyTorch ops (hf_module_sampling_inputs) + multiscale_deformable_attention: what
          `replace_hf_msda(model)` leaves a Hugging Face model with; it is the yardstick.
Legs: (1) the core at the Deformable-DETR encoder shape (c3: B = 2, Q = I = 17 821, 2-d reference points), fp32;
(2) the core at the Grounding-DINO decoder shape (B = 8, Q = 900, 4-d reference boxes), fp32 and bf16 storage (value +
projection in bf16 next to fp32 reference points: what autocast hands the core); (3) one training step of the
ResNet-50-shaped Deformable-DETR of tools/hf_model_share.py at 800 x 1066, `replace_hf_msda(model)` against
`replace_hf_msda(model, fused=True)` — two models with the same weights, alternated.  Per leg: `repeats` timed runs
between two events after a warm-up; the median and the min / max of the per-call times are reported."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from msda_triton_amd import multiscale_deformable_attention, synth
from msda_triton_amd.functional import fused_hf_module_core, hf_module_sampling_inputs

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--no-model", action="store_true")
a = ap.parse_args()
dev = torch.device("cuda", 0)
c3, c4 = synth.WORKLOADS["c3_ddetr_enc"], synth.WORKLOADS["c4_gdino_dec"]
CASES = [
    ("c3_ddetr_enc_fp32", c3.B, c3.Q, c3.H, c3.D, [tuple(l) for l in c3.levels], 4, 2, torch.float32),
    ("c4_gdino_dec_fp32", c4.B, c4.Q, c4.H, c4.D, [tuple(l) for l in c4.levels], 4, 4, torch.float32),
    ("c4_gdino_dec_bf16_storage", c4.B, c4.Q, c4.H, c4.D, [tuple(l) for l in c4.levels], 4, 4, torch.bfloat16),
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


def verdict(fused, unfused):
    """ahead only when the fused leg's slowest repeat beats the unfused leg's fastest"""
    return "fused ahead of the whole spread" if fused["max"] < unfused["min"] else \
        ("unfused ahead of the whole spread" if unfused["max"] < fused["min"] else "spreads overlap")


results = []
for name, B, Q, H, D, levels, P, rd, sdt in CASES:
    torch.manual_seed(0)
    L = len(levels)
    shapes = torch.tensor(levels, device=dev)
    value = torch.randn(B, sum(h * w for h, w in levels), H, D, device=dev).to(sdt).requires_grad_()
    proj = (torch.randn(B, Q, H, L, P, 3, device=dev) * 1.5).to(sdt).requires_grad_()
    ref = torch.rand(B, Q, L, rd, device=dev).requires_grad_()  # (Deformable-DETR's decoder points take a gradient)
    go = torch.randn(B, Q, H, D, device=dev).to(sdt)

    def fused():
        return fused_hf_module_core(value, shapes, proj, ref, "zeros", False, levels)

    def unfused():
        pts, att = hf_module_sampling_inputs(proj.float(), shapes, ref)
        return multiscale_deformable_attention(value, shapes, pts, att, "zeros", False, level_shapes=levels).to(sdt)

    def step(f):
        def run():
            f().backward(go)
            value.grad = proj.grad = ref.grad = None
        return run

    def fwd(f):
        def run():
            with torch.no_grad():
                f()
        return run

    legs = {"fused_fwd": fwd(fused), "unfused_fwd": fwd(unfused), "fused_fwd_bwd": step(fused), "unfused_fwd_bwd": step(unfused)}
    times = {k: [] for k in legs}
    for f in legs.values():
        for _ in range(10):
            f()
    torch.cuda.synchronize()
    for _ in range(a.repeats):  # alternated: every repeat visits every leg
        for k, f in legs.items():
            times[k].append(timed(f, a.iters))
    row = {"case": name, "B": B, "Q": Q, "H": H, "D": D, "levels": levels, "P": P, "ref_dim": rd,
           "storage": str(sdt).replace("torch.", ""), "repeats": a.repeats, "iters": a.iters, "unit": "ms per call"}
    for k, v in times.items():
        row[k] = spread(v)
    for kind in ("fwd", "fwd_bwd"):
        row[f"speedup_{kind}"] = round(row[f"unfused_{kind}"]["median"] / row[f"fused_{kind}"]["median"], 3)
        row[f"verdict_{kind}"] = verdict(row[f"fused_{kind}"], row[f"unfused_{kind}"])
    results.append(row)
    print(json.dumps(row), flush=True)
    del value, proj, ref, go

if not a.no_model:
    import copy

    from transformers import DeformableDetrConfig, DeformableDetrModel, ResNetConfig

    from msda_triton_amd.hf_adapter import replace_hf_msda
    bb = ResNetConfig(num_channels=3, embedding_size=64, hidden_sizes=[256, 512, 1024, 2048], depths=[3, 4, 6, 3],
                      layer_type="bottleneck", out_features=["stage2", "stage3", "stage4"])
    cfg = DeformableDetrConfig(use_timm_backbone=False, use_pretrained_backbone=False, backbone_config=bb, backbone=None,
                               dropout=0.0, attention_dropout=0.0, activation_dropout=0.0)
    torch.manual_seed(0)
    base = DeformableDetrModel(cfg).to(dev).train()
    with torch.no_grad():
        for n, p in base.named_parameters():
            if n.endswith("sampling_offsets.weight"):
                p.normal_(0, 0.02)
    models = {"unfused": base, "fused": copy.deepcopy(base)}
    n_unfused, n_fused = replace_hf_msda(models["unfused"]), replace_hf_msda(models["fused"], fused=True)
    x = torch.randn(2, 3, 800, 1066, device=dev)
    mask = torch.ones(2, 800, 1066, dtype=torch.long, device=dev)
    for autocast in (False, True):
        def train_step(m):
            def run():
                m.zero_grad(set_to_none=True)
                with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                    out = m(pixel_values=x, pixel_mask=mask)
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
        row = {"case": "deformable_detr_r50_train_step_" + ("bf16_autocast" if autocast else "fp32"),
               "image": [800, 1066], "batch": 2, "modules_replaced": n_unfused, "modules_replaced_or_wrapped": n_fused,
               "repeats": a.repeats, "steps": a.steps, "unit": "ms per step (device time between events)"}
        for k, v in times.items():
            row[k] = spread(v)
        row["speedup"] = round(row["unfused"]["median"] / row["fused"]["median"], 3)
        row["verdict"] = verdict(row["fused"], row["unfused"])
        results.append(row)
        print(json.dumps(row), flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "results": results}, f, indent=1)
