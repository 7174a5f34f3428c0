"""The value padding mask inside the kernels against `masked_fill` in front of them, in one process and alternated:
    python tools/hf_mask_bench.py [--out profiles/NAME.json] [--repeats 7] [--iters 30] [--steps 3] [--no-model]

"parent"  value.masked_fill(~mask[..., None], 0) + fused_hf_module_core(...)  — what the Hugging Face adapter did before
          the value-mask kernels (msda_{fwd,bwd}_fused_levelref_<suffix> behind a pass over the pyramid, and autograd's
          mirror-image pass over grad_value); it is the yardstick.
"masked"  fused_hf_module_core(..., value_mask=mask)  — msda_{fwd,bwd}_fused_levelref_masked_<suffix>
The mask is the rectangular padding mask of a batch whose last element is valid on the left 75 % and top 60 % of every
level.  Legs: (1) the core at the Deformable-DETR encoder shape (c3: B = 2, Q = I = 17 821, 2-d reference points), fp32;
(2) the core at the Grounding-DINO decoder shape (c4: B = 8, Q = 900, 4-d boxes), fp32 and bf16 storage; (3) one training
step of the ResNet-50-shaped Deformable-DETR of tools/hf_model_share.py at 800 x 1066 with a padding `pixel_mask`, fused
wrapper, hf_adapter.MASK_IN_KERNELS False against True — two models with the same weights, alternated.  Per leg:
`repeats` timed runs between two events after a warm-up; the median and the min / max of the per-call times are reported.
The adapter's rule: the kernels take the mask only where the masked leg's slowest repeat is below the
parent leg's fastest, forward plus backward."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from msda_triton_amd import synth
from msda_triton_amd.functional import fused_hf_module_core

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


def padding_mask(B, levels):
    m = torch.ones(B, sum(h * w for h, w in levels), dtype=torch.bool)
    start = 0
    for h, w in levels:
        lv = torch.zeros(h, w, dtype=torch.bool)
        lv[:max(1, int(h * 0.6)), :max(1, int(w * 0.75))] = True
        m[B - 1, start:start + h * w] = lv.reshape(-1)
        start += h * w
    return m


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


def verdict(masked, parent):
    """ahead only when the masked leg's slowest repeat beats the parent leg's fastest"""
    return "masked ahead of the whole spread" if masked["max"] < parent["min"] else \
        ("parent ahead of the whole spread" if parent["max"] < masked["min"] else "spreads overlap")


results = []
for name, B, Q, H, D, levels, P, rd, sdt in CASES:
    torch.manual_seed(0)
    L = len(levels)
    shapes = torch.tensor(levels, device=dev)
    value = torch.randn(B, sum(h * w for h, w in levels), H, D, device=dev).to(sdt).requires_grad_()
    proj = (torch.randn(B, Q, H, L, P, 3, device=dev) * 1.5).to(sdt).requires_grad_()
    ref = torch.rand(B, Q, L, rd, device=dev).requires_grad_()
    go = torch.randn(B, Q, H, D, device=dev).to(sdt)
    mask = padding_mask(B, levels).to(dev)

    def masked():
        return fused_hf_module_core(value, shapes, proj, ref, "zeros", False, levels, value_mask=mask)

    def parent():  # (the adapter's line, on the [B, I, H * D] rows as transformers has them)
        v = value.view(B, -1, H * D).masked_fill(~mask[..., None], float(0)).view(B, -1, H, D)
        return fused_hf_module_core(v, shapes, proj, ref, "zeros", False, levels)

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

    legs = {"masked_fwd": fwd(masked), "parent_fwd": fwd(parent), "masked_fwd_bwd": step(masked), "parent_fwd_bwd": step(parent)}
    times = {k: [] for k in legs}
    for f in legs.values():
        for _ in range(10):
            f()
    torch.cuda.synchronize()
    for _ in range(a.repeats):  # alternated: every repeat visits every leg
        for k, f in legs.items():
            times[k].append(timed(f, a.iters))
    row = {"case": name, "B": B, "Q": Q, "H": H, "D": D, "levels": levels, "P": P, "ref_dim": rd,
           "storage": str(sdt).replace("torch.", ""), "masked_pixels": int((~mask).sum()), "pixels": int(mask.numel()),
           "repeats": a.repeats, "iters": a.iters, "unit": "ms per call"}
    for k, v in times.items():
        row[k] = spread(v)
    for kind in ("fwd", "fwd_bwd"):
        row[f"speedup_{kind}"] = round(row[f"parent_{kind}"]["median"] / row[f"masked_{kind}"]["median"], 3)
        row[f"verdict_{kind}"] = verdict(row[f"masked_{kind}"], row[f"parent_{kind}"])
    results.append(row)
    print(json.dumps(row), flush=True)
    del value, proj, ref, go

if not a.no_model:
    from transformers import DeformableDetrConfig, DeformableDetrModel, ResNetConfig

    from msda_triton_amd import hf_adapter
    bb = ResNetConfig(num_channels=3, embedding_size=64, hidden_sizes=[256, 512, 1024, 2048], depths=[3, 4, 6, 3],
                      layer_type="bottleneck", out_features=["stage2", "stage3", "stage4"])
    cfg = DeformableDetrConfig(use_timm_backbone=False, use_pretrained_backbone=False, backbone_config=bb, backbone=None,
                               dropout=0.0, attention_dropout=0.0, activation_dropout=0.0)
    torch.manual_seed(0)
    model = DeformableDetrModel(cfg).to(dev).train()
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith("sampling_offsets.weight"):
                p.normal_(0, 0.02)
    n_fused = hf_adapter.replace_hf_msda(model, fused=True)
    x = torch.randn(2, 3, 800, 1066, device=dev)
    pixel_mask = torch.ones(2, 800, 1066, dtype=torch.long, device=dev)
    pixel_mask[1, 480:] = 0  # the second image is 480 x 800 inside the 800 x 1066 batch
    pixel_mask[1, :, 800:] = 0
    keep = hf_adapter.MASK_IN_KERNELS
    for autocast in (False, True):
        def train_step(in_kernels):
            def run():
                hf_adapter.MASK_IN_KERNELS = in_kernels  # (one model, the adapter's switch flipped per leg)
                model.zero_grad(set_to_none=True)
                with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                    out = model(pixel_values=x, pixel_mask=pixel_mask)
                (out.last_hidden_state.float() ** 2).mean().backward()
            return run
        legs = {"parent": train_step(False), "masked": train_step(True)}
        times = {k: [] for k in legs}
        for f in legs.values():
            for _ in range(2):
                f()
        torch.cuda.synchronize()
        for _ in range(a.repeats):
            for k, f in legs.items():
                times[k].append(timed(f, a.steps))
        row = {"case": "deformable_detr_r50_train_step_" + ("bf16_autocast" if autocast else "fp32"),
               "image": [800, 1066], "batch": 2, "second_image_valid": [480, 800], "modules_replaced_or_wrapped": n_fused,
               "repeats": a.repeats, "steps": a.steps, "unit": "ms per step (device time between events)"}
        for k, v in times.items():
            row[k] = spread(v)
        row["speedup"] = round(row["parent"]["median"] / row["masked"]["median"], 3)
        row["verdict"] = verdict(row["masked"], row["parent"])
        results.append(row)
        print(json.dumps(row), flush=True)
    hf_adapter.MASK_IN_KERNELS = keep
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "results": results}, f, indent=1)
