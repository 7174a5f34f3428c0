"""Both padding masks inside the nn.Module's fused kernels against their composition, in one process and alternated:
    python tools/module_mask_bench.py [--out profiles/NAME.json] [--repeats 7] [--iters 30]

"composed"  fused_module_core(..., value_mask=, query_mask=, mask_in_kernels=False) — what a masked module call did before
            these kernels: masked_fill over the value pyramid and autograd's mirror pass over grad_value, three where passes
            for the query mask, then the unmasked fused pair (its C++ autograd node where that is built).  It is the yardstick.
"masked"    the same call with mask_in_kernels=True — msda_{fwd,bwd}_fused_masked_<suffix>, with per-level counts
            msda_{fwd,bwd}_fused_ragged_masked_<suffix>, through the Python Function.
The value mask is the rectangular padding mask of a batch whose last element is valid on the left 75 % and top 60 % of
every level (tools/hf_mask_bench.py's).  Cases, each with fp32, with bf16 storage (value, projection and result in bf16,
reference points and arithmetic fp32) and with a bf16 pyramid next to fp32 sampling inputs (the module's `value_dtype`):
  c2_module_q10k   the c2 module shape at 10 000 queries (B 4, H 8, D 32, 64 x 64 ... 8 x 8, P 4, 2-d reference points);
                   the last quarter of every batch element's queries is padding; also with the value mask alone
  encoder_self     an encoder-shaped self-attention call at the Deformable-DETR encoder pyramid (B 2, Q = I = 17 821): the
                   rectangular mask in both roles
  dfine_640        D-FINE at 640 x 640: 80 x 80, 40 x 40, 20 x 20 with points [3, 6, 3], 300 queries with 4-d boxes, B 8; the
                   last quarter of the queries is padding
Per leg: `repeats` timed runs of `iters` calls between two events after a warm-up; median [min - max] of the per-call times.
The module's rule: a storage dtype goes to the kernels only where the masked leg's slowest repeat is below
the composition's fastest, forward plus backward."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from msda_triton_amd import _lib, synth
from msda_triton_amd.functional import fused_module_core

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--iters", type=int, default=30)
a = ap.parse_args()
dev = torch.device("cuda", 0)
c2, c3 = synth.WORKLOADS["c2_q10k"], synth.WORKLOADS["c3_ddetr_enc"]
c3_levels = [tuple(l) for l in c3.levels]
# (name, B, Q, H, D, levels, points (int or per level), ref_dim, query mask: "quarter" | "as_value" | None)
SHAPES = [
    ("c2_module_q10k", c2.B, 10000, c2.H, c2.D, [tuple(l) for l in c2.levels], 4, 2, "quarter"),
    ("c2_module_q10k_value_mask_only", c2.B, 10000, c2.H, c2.D, [tuple(l) for l in c2.levels], 4, 2, None),
    ("encoder_self", c3.B, sum(h * w for h, w in c3_levels), c3.H, c3.D, c3_levels, 4, 2, "as_value"),
    ("dfine_640", 8, 300, 8, 32, [(80, 80), (40, 40), (20, 20)], [3, 6, 3], 4, "quarter"),
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


def verdict(masked, composed):
    """ahead only when the masked leg's slowest repeat beats the composition's fastest"""
    return "masked ahead of the whole spread" if masked["max"] < composed["min"] else \
        ("composed ahead of the whole spread" if composed["max"] < masked["min"] else "spreads overlap")


results = []
for name, B, Q, H, D, levels, points, rd, qkind in SHAPES:
    # (storage of the value pyramid, of the projection / result): fp32; bf16 storage; bf16 pyramid next to fp32 sampling inputs
    for sdt, pdt in ((torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16), (torch.bfloat16, torch.float32)):
        torch.manual_seed(0)
        L = len(levels)
        counts = None if isinstance(points, int) else tuple(points)
        shapes = torch.tensor(levels, device=dev)
        value = torch.randn(B, sum(h * w for h, w in levels), H, D, device=dev).to(sdt).requires_grad_()
        pshape = (B, Q, H, L, points, 3) if counts is None else (B, Q, H, sum(counts), 3)
        proj = (torch.randn(*pshape, device=dev) * 1.5).to(pdt).requires_grad_()
        ref = torch.rand(B, Q, rd, device=dev).requires_grad_()
        go = torch.randn(B, Q, H, D, device=dev).to(pdt)
        vmask = padding_mask(B, levels).to(dev)
        qmask = None
        if qkind == "quarter":
            qmask = torch.ones(B, Q, dtype=torch.bool, device=dev)
            qmask[:, Q - Q // 4:] = False
        elif qkind == "as_value":
            qmask = vmask

        def call(in_kernels):
            return lambda: fused_module_core(value, shapes, proj, ref, "zeros", False, levels, counts, vmask, qmask,
                                             mask_in_kernels=in_kernels)

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

        legs = {"masked_fwd": fwd(call(True)), "composed_fwd": fwd(call(False)), "masked_fwd_bwd": step(call(True)),
                "composed_fwd_bwd": step(call(False))}
        times = {k: [] for k in legs}
        info = {}
        for k, f in legs.items():
            for _ in range(10):
                f()
            torch.cuda.synchronize()
            li = _lib.last_launch_info()
            info[k] = {x: li[x] for x in ("fwd_variant", "sample_variant", "value_path")}
        for _ in range(a.repeats):  # alternated: every repeat visits every leg
            for k, f in legs.items():
                times[k].append(timed(f, a.iters))
        row = {"case": name, "B": B, "Q": Q, "H": H, "D": D, "levels": levels, "points": points, "ref_dim": rd,
               "storage": str(sdt).replace("torch.", ""), "projection_storage": str(pdt).replace("torch.", ""), "masked_pixels": int((~vmask).sum()), "pixels": int(vmask.numel()),
               "masked_queries": 0 if qmask is None else int((~qmask).sum()), "queries": B * Q, "variants": info,
               "repeats": a.repeats, "iters": a.iters, "unit": "ms per call"}
        for k, v in times.items():
            row[k] = spread(v)
        for kind in ("fwd", "fwd_bwd"):
            row[f"speedup_{kind}"] = round(row[f"composed_{kind}"]["median"] / row[f"masked_{kind}"]["median"], 3)
            row[f"verdict_{kind}"] = verdict(row[f"masked_{kind}"], row[f"composed_{kind}"])
        results.append(row)
        print(json.dumps(row), flush=True)
        del value, proj, ref, go

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "results": results}, f, indent=1)
