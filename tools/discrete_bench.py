"""Discrete (nearest-pixel) sampling against this project's bilinear call and against transformers' own discrete core:
steady-state public-API forward and forward + backward time on the same inputs, and the per-kernel times of the
library's profile option.

    python tools/discrete_bench.py [--reps 50] [--repeats 5] [--legs discrete,bilinear,hf_discrete] [--out FILE.json]

Shapes (those of tools/ragged_points_bench.py): D-FINE's decoder at 640 x 640 (B = 8, Q = 300, H = 8, D = 32,
80x80 / 40x40 / 20x20, [3, 6, 3], fp32) and c2's shape at Q = 10 000 with [2, 4, 6, 4] (the sorted grad_value pipeline).
Every leg is timed ``--repeats`` times (each the mean of ``--reps`` back-to-back calls after 5 warm-up calls, CUDA
events); the record keeps min / median / max, and max - min of a leg is its run-to-run spread.  ``--legs bilinear`` uses
nothing of the discrete mode, so the same file measures the bilinear leg on a checkout that predates it.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from msda_triton_amd import _lib, multiscale_deformable_attention  # noqa: E402

CASES = [
    ("dfine_640_fp32", 8, 300, 8, 32, ((80, 80), (40, 40), (20, 20)), (3, 6, 3)),
    ("c2_q10k_2464", 4, 10000, 8, 32, ((64, 64), (32, 32), (16, 16), (8, 8)), (2, 4, 6, 4)),
]


def inputs(B, Q, H, D, shapes, counts, dev):
    g = torch.Generator(device="cpu").manual_seed(0)
    I = sum(h * w for h, w in shapes)  # noqa: E741
    S = sum(counts)
    img = torch.randn(B, I, H, D, generator=g).to(dev)
    loc = torch.rand(B, Q, H, S, 2, generator=g).to(dev)
    attn = torch.rand(B, Q, H, S, generator=g).to(dev)
    return img, torch.tensor(shapes, device=dev), loc, attn


def timed(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def stats(fn, reps, repeats):
    xs = sorted(timed(fn, reps) for _ in range(repeats))
    return {"min": round(xs[0], 4), "median": round(statistics.median(xs), 4), "max": round(xs[-1], 4)}


def kernels(fn):
    _lib.set_option("profile", 1)
    _lib.profile_read()
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    prof = _lib.profile_read()
    _lib.set_option("profile", 0)
    return {k: round(v[1], 2) for k, v in prof.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--legs", default="discrete,bilinear,hf_discrete")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    legs = args.legs.split(",")
    hf_core = None
    if "hf_discrete" in legs:
        try:
            from transformers.models.d_fine.modeling_d_fine import multi_scale_deformable_attention_v2 as hf_core
        except Exception as e:  # not measured, and said so
            print(f"hf_discrete leg unmeasured: {e}", file=sys.stderr)
            legs.remove("hf_discrete")
    dev = torch.device("cuda:0")
    rows = []
    for name, B, Q, H, D, shapes, counts in CASES:
        img, shp, loc, attn = inputs(B, Q, H, D, shapes, counts, dev)
        grad = torch.randn(B, Q, H, D, device=dev)
        row = {"case": name, "B": B, "Q": Q, "H": H, "D": D, "shapes": shapes, "points_per_level": counts,
               "reps": args.reps, "repeats": args.repeats}
        v, p, a = (t.detach().requires_grad_(True) for t in (img, loc, attn))
        for leg in legs:
            if leg == "hf_discrete":
                def call(vv, pp, aa):
                    return hf_core(vv, [list(s) for s in shapes], pp, aa, list(counts), "discrete")
                g = grad.flatten(2)
            else:
                kw = {"sampling_mode": "discrete"} if leg == "discrete" else {}
                pm = "border" if leg == "discrete" else "zeros"

                def call(vv, pp, aa, kw=kw, pm=pm):
                    return multiscale_deformable_attention(vv, shp, pp, aa, pm, False, level_shapes=shapes,
                                                           points_per_level=list(counts), **kw)
                g = grad

            def fwd():
                with torch.no_grad():
                    return call(img, loc, attn)

            def fwd_bwd():
                call(v, p, a).backward(g)

            row[f"{leg}_fwd_ms"] = stats(fwd, args.reps, args.repeats)
            row[f"{leg}_fwd_bwd_ms"] = stats(fwd_bwd, args.reps, args.repeats)
            if leg != "hf_discrete":
                row[f"{leg}_kernels_us"] = kernels(fwd_bwd)
        for other in ("bilinear", "hf_discrete"):
            if "discrete" in legs and other in legs:
                for k in ("fwd", "fwd_bwd"):
                    row[f"discrete_over_{other}_{k}"] = round(row[f"discrete_{k}_ms"]["median"] / row[f"{other}_{k}_ms"]["median"], 3)
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
