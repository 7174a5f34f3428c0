"""The query padding mask in the kernels against the value mask alone, in one process and alternated (the protocol of
tools/hf_mask_bench.py):
    python tools/hf_query_mask_bench.py [--out profiles/NAME.json] [--repeats 7] [--iters 30] [--steps 3] [--no-model]

"parent"  fused_hf_module_core(..., value_mask=mask)  — msda_{fwd,bwd}_fused_levelref_masked_<suffix>, the path before the
          query mask existed; in this build those entry points are the same kernels with query_mask = NULL.  It is the
          yardstick, and its min - max range is the tool's own repeat-to-repeat spread.
"ones"    ... value_mask=mask, query_mask=all ones  — msda_*_fused_levelref_qmasked_<suffix> with nothing to skip: what the
          hooks cost (must stay inside the parent's spread)
"qmask"   ... value_mask=mask, query_mask=mask  — the encoder's case, Q == I: 27.5 % of the queries are padding
The mask is tools/hf_mask_bench.py's rectangle (the last batch element valid on the left 75 % / top 60 % of every level).
Legs: (1) the core at the Deformable-DETR encoder shape (c3: B = 2, Q = I = 17 821, 2-d reference points) in fp32 and with
bf16 value + projection, forward and forward + backward, plus the library's per-kernel times (option "profile") for each
leg; (2) one training step of the ResNet-50-shaped Deformable-DETR of tools/hf_mask_bench.py at 800 x 1066 with a padding
`pixel_mask`, fused wrapper, skip_padded_queries off against on — one model, the modules' flag flipped per leg.  Per leg:
`repeats` timed runs between two events after a warm-up; median and min / max of the per-call times."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from msda_triton_amd import _lib, synth
from msda_triton_amd.functional import fused_hf_module_core

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--no-model", action="store_true")
a = ap.parse_args()
dev = torch.device("cuda", 0)
c3 = synth.WORKLOADS["c3_ddetr_enc"]
CASES = [("c3_ddetr_enc_fp32", torch.float32), ("c3_ddetr_enc_bf16_storage", torch.bfloat16)]


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


def verdict(leg, parent):
    """ahead / behind only when the leg's whole spread lies outside the parent's"""
    return "ahead of the parent's whole spread" if leg["max"] < parent["min"] else \
        ("behind the parent's whole spread" if parent["max"] < leg["min"] else "inside the parent's spread")


def kernel_times(fn, iters=10):
    """the library's own event pair per kernel launch (option "profile"), us per launch"""
    _lib.set_option("profile", 1)
    _lib.profile_read()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    prof = {k: round(v[1], 2) for k, v in _lib.profile_read().items()}
    _lib.set_option("profile", 0)
    return prof


results = []
B, Q, H, D, levels, P, rd = c3.B, c3.Q, c3.H, c3.D, [tuple(l) for l in c3.levels], 4, 2
for name, sdt in CASES:
    torch.manual_seed(0)
    L = len(levels)
    shapes = torch.tensor(levels, device=dev)
    n_pix = sum(h * w for h, w in levels)
    assert Q == n_pix, "the encoder shape: every pixel is a query"
    value = torch.randn(B, n_pix, H, D, device=dev).to(sdt).requires_grad_()
    proj = (torch.randn(B, Q, H, L, P, 3, device=dev) * 1.5).to(sdt).requires_grad_()
    ref = torch.rand(B, Q, L, rd, device=dev).requires_grad_()
    go = torch.randn(B, Q, H, D, device=dev).to(sdt)
    mask = padding_mask(B, levels).to(dev)
    ones = torch.ones_like(mask)

    def core(qm):
        return lambda: fused_hf_module_core(value, shapes, proj, ref, "zeros", False, levels, value_mask=mask, query_mask=qm)

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

    cores = {"parent": core(None), "ones": core(ones), "qmask": core(mask)}
    legs = {f"{k}_fwd": fwd(f) for k, f in cores.items()}
    legs.update({f"{k}_fwd_bwd": step(f) for k, f in cores.items()})
    times = {k: [] for k in legs}
    for f in legs.values():
        for _ in range(10):
            f()
    torch.cuda.synchronize()
    for _ in range(a.repeats):  # alternated: every repeat visits every leg
        for k, f in legs.items():
            times[k].append(timed(f, a.iters))
    row = {"case": name, "B": B, "Q": Q, "H": H, "D": D, "levels": levels, "P": P, "ref_dim": rd,
           "storage": str(sdt).replace("torch.", ""), "masked_queries": int((~mask).sum()), "queries": int(mask.numel()),
           "repeats": a.repeats, "iters": a.iters, "unit": "ms per call"}
    for k, v in times.items():
        row[k] = spread(v)
    for kind in ("fwd", "fwd_bwd"):
        for leg in ("ones", "qmask"):
            row[f"speedup_{leg}_{kind}"] = round(row[f"parent_{kind}"]["median"] / row[f"{leg}_{kind}"]["median"], 3)
            row[f"verdict_{leg}_{kind}"] = verdict(row[f"{leg}_{kind}"], row[f"parent_{kind}"])
    row["kernel_us"] = {k: kernel_times(step(f)) for k, f in cores.items()}
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
    fused = [m for m in model.modules() if isinstance(m, hf_adapter.FusedHFDeformableAttention)]
    x = torch.randn(2, 3, 800, 1066, device=dev)
    pixel_mask = torch.ones(2, 800, 1066, dtype=torch.long, device=dev)
    pixel_mask[1, 480:] = 0  # the second image is 480 x 800 inside the 800 x 1066 batch
    pixel_mask[1, :, 800:] = 0
    for autocast in (False, True):
        def train_step(skip):
            def run():
                for m in fused:  # (one model, the modules' flag flipped per leg)
                    m.skip_padded_queries = skip
                model.zero_grad(set_to_none=True)
                with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                    out = model(pixel_values=x, pixel_mask=pixel_mask)
                (out.last_hidden_state.float() ** 2).mean().backward()
            return run
        legs = {"parent": train_step(False), "skip_padded_queries": train_step(True)}
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
        row["speedup"] = round(row["parent"]["median"] / row["skip_padded_queries"]["median"], 3)
        row["verdict"] = verdict(row["skip_padded_queries"], row["parent"])
        results.append(row)
        print(json.dumps(row), flush=True)
    for m in fused:
        m.skip_padded_queries = False
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "results": results}, f, indent=1)
