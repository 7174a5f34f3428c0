"""The Hugging Face adapter's three ways from `hidden_states` to the attended values, in one process and alternated:
    python tools/levelref_split_bench.py [--out profiles/NAME.json] [--repeats 7] [--iters 30]

"one_gemm"   (a) today's route for plain layers: the two layers' weights concatenated and re-ordered, ONE GEMM that
             writes [B, Q, H, L, P, 3], the interleaved kernels (msda_{fwd,bwd}_fused_levelref_<suffix>; their C++ autograd
             node where that is built).  Context only: it stays the default for plain nn.Linear pairs whatever comes out here.
"split"      (b) the two layers CALLED (what a LoRA wrapper, a hook or a quantised replacement needs) and their outputs, as
             they are, to msda_{fwd,bwd}_fused_levelref_split_<suffix> (fused_hf_module_core_split).
"cat"        (c) the two layers called, `torch.cat` into [B, Q, H, L, P, 3] (and its mirror in the backward), the
             interleaved kernels — fused_hf_module_core_split(..., split_in_kernels=False): what fixing the adapter in
             Python alone would cost.
Shapes, each in fp32 and with bf16 storage (hidden states, layers, value, projections and result in bf16; reference points
and arithmetic fp32), forward and forward + backward, d_model = H * D = 256:
  ddetr_encoder   the Deformable-DETR encoder: B 2, Q = I = 17 821, L 4, P 4, H 8, D 32
  gdino_decoder   the Grounding-DINO decoder: B 8, Q 900 over the 64 x 64 ... 8 x 8 pyramid
Per leg: `repeats` timed runs of `iters` calls between two events after a warm-up; median [min - max] of the per-call times.
The rule: the adapter's non-plain route takes (b) for a storage dtype only where (b)'s slowest repeat is
below (c)'s fastest, forward + backward."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from msda_triton_amd import synth
from msda_triton_amd.functional import fused_hf_module_core, fused_hf_module_core_split

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--iters", type=int, default=30)
a = ap.parse_args()
dev = torch.device("cuda", 0)
c3, c4 = synth.WORKLOADS["c3_ddetr_enc"], synth.WORKLOADS["c4_gdino_dec"]
SHAPES = [("ddetr_encoder", c3.B, c3.Q, c3.H, c3.D, [tuple(l) for l in c3.levels], 4),
          ("gdino_decoder", c4.B, c4.Q, c4.H, c4.D, [tuple(l) for l in c4.levels], 4)]


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


def verdict(split, cat):
    """ahead only when the split leg's slowest repeat beats the cat leg's fastest"""
    return "split ahead of the whole spread" if split["max"] < cat["min"] else \
        ("cat ahead of the whole spread" if cat["max"] < split["min"] else "spreads overlap")


results = []
for name, B, Q, H, D, levels, P in SHAPES:
    for sdt in (torch.float32, torch.bfloat16):
        torch.manual_seed(0)
        L, n, dm = len(levels), H * len(levels) * P, H * D
        shapes = torch.tensor(levels, device=dev)
        value = torch.randn(B, sum(h * w for h, w in levels), H, D, device=dev).to(sdt).requires_grad_()
        hidden = torch.randn(B, Q, dm, device=dev).to(sdt).requires_grad_()
        so, aw = torch.nn.Linear(dm, 2 * n).to(dev, sdt), torch.nn.Linear(dm, n).to(dev, sdt)
        with torch.no_grad():
            so.weight.mul_(3.0)  # (offsets of a pixel or two, as a trained module's)
        ref = torch.rand(B, Q, L, 2, device=dev).requires_grad_()  # (fp32 in both storages)
        go = torch.randn(B, Q, H, D, device=dev).to(sdt)
        s = torch.arange(n, device=dev)
        rows = torch.stack([2 * s, 2 * s + 1, 2 * n + s], -1).reshape(-1)
        leaves = [value, hidden, ref] + list(so.parameters()) + list(aw.parameters())

        def one_gemm():
            weight = torch.cat([so.weight, aw.weight], 0).index_select(0, rows)
            bias = torch.cat([so.bias, aw.bias], 0).index_select(0, rows)
            proj = torch.nn.functional.linear(hidden, weight, bias).view(B, Q, H, L, P, 3)
            return fused_hf_module_core(value, shapes, proj, ref, "zeros", False, level_shapes=levels)

        def two_layers(in_kernels):
            return lambda: fused_hf_module_core_split(value, shapes, so(hidden), aw(hidden), ref, "zeros", False,
                                                      level_shapes=levels, split_in_kernels=in_kernels)

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

        calls = {"one_gemm": one_gemm, "split": two_layers(True), "cat": two_layers(False)}
        legs = {f"{k}_fwd": fwd(f) for k, f in calls.items()}
        legs.update({f"{k}_fwd_bwd": step(f) for k, f in calls.items()})
        times = {k: [] for k in legs}
        for f in legs.values():
            for _ in range(10):
                f()
        torch.cuda.synchronize()
        for _ in range(a.repeats):  # alternated: every repeat visits every leg
            for k, f in legs.items():
                times[k].append(timed(f, a.iters))
        row = {"case": name, "B": B, "Q": Q, "H": H, "D": D, "levels": levels, "points": P, "ref_dim": 2,
               "storage": str(sdt).replace("torch.", ""), "repeats": a.repeats, "iters": a.iters, "unit": "ms per call"}
        for k, v in times.items():
            row[k] = spread(v)
        for kind in ("fwd", "fwd_bwd"):
            row[f"split_over_cat_{kind}"] = round(row[f"cat_{kind}"]["median"] / row[f"split_{kind}"]["median"], 3)
            row[f"verdict_{kind}"] = verdict(row[f"split_{kind}"], row[f"cat_{kind}"])
        results.append(row)
        print(json.dumps(row), flush=True)
        del value, hidden, ref, go, so, aw

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "results": results}, f, indent=1)
