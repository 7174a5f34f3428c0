"""Per-level point counts against zero padding: steady-state public-API forward and forward + backward time, and the
per-kernel times of the library's profile option, for the ragged call (``points_per_level``) and for the zero-padded
dense call on the same inputs.

    python tools/ragged_points_bench.py [--reps 50] [--out FILE.json]

Shapes: D-FINE's decoder at 640 x 640 (B = 8, Q = 300, H = 8, D = 32, 80x80 / 40x40 / 20x20, [3, 6, 3]) with fp32 and
bf16 values next to fp32 points, and c2's shape at Q = 10 000 with [2, 4, 6, 4] (the sorted grad_value pipeline).
Two paddings: "padded" puts every padded point at (0.5, 0.5) (one bilinear cell per level collects all of them), and
"padded_spread" at the locations of the level's own points — the like-for-like comparison for the gather kernels.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from msda_triton_amd import _lib, multiscale_deformable_attention  # noqa: E402

CASES = [
    ("dfine_640_fp32", 8, 300, 8, 32, ((80, 80), (40, 40), (20, 20)), (3, 6, 3), torch.float32),
    ("dfine_640_vbf16", 8, 300, 8, 32, ((80, 80), (40, 40), (20, 20)), (3, 6, 3), torch.bfloat16),
    ("c2_q10k_2464", 4, 10000, 8, 32, ((64, 64), (32, 32), (16, 16), (8, 8)), (2, 4, 6, 4), torch.float32),
]


def inputs(B, Q, H, D, shapes, counts, vdt, dev, spread=False):
    g = torch.Generator(device="cpu").manual_seed(0)
    I = sum(h * w for h, w in shapes)  # noqa: E741
    S = sum(counts)
    img = torch.randn(B, I, H, D, generator=g).to(dev, vdt)
    loc = torch.rand(B, Q, H, S, 2, generator=g).to(dev)
    attn = torch.rand(B, Q, H, S, generator=g).to(dev)
    L, Pm = len(counts), max(counts)
    ploc = torch.full((B, Q, H, L, Pm, 2), 0.5, device=dev)
    patt = torch.zeros((B, Q, H, L, Pm), device=dev)
    s0 = 0
    for lvl, p in enumerate(counts):
        ploc[:, :, :, lvl, :p] = loc[:, :, :, s0:s0 + p]
        patt[:, :, :, lvl, :p] = attn[:, :, :, s0:s0 + p]
        if spread:  # padded points at the locations of the level's real points (cycled), not all at (0.5, 0.5)
            for k in range(p, Pm):
                ploc[:, :, :, lvl, k] = loc[:, :, :, s0 + (k - p) % p]
        s0 += p
    return img, torch.tensor(shapes, device=dev), loc, attn, ploc, patt


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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for name, B, Q, H, D, shapes, counts, vdt in CASES:
        img, shp, loc, attn, ploc, patt = inputs(B, Q, H, D, shapes, counts, vdt, dev)
        _, _, _, _, sloc, _ = inputs(B, Q, H, D, shapes, counts, vdt, dev, spread=True)
        grad = torch.randn(B, Q, H, D, device=dev)
        row = {"case": name, "B": B, "Q": Q, "H": H, "D": D, "shapes": shapes, "points_per_level": counts,
               "value_dtype": str(vdt)}
        for tag, pts, att, kw in (("ragged", loc, attn, {"points_per_level": list(counts)}), ("padded", ploc, patt, {}),
                                  ("padded_spread", sloc, patt, {})):
            v, p, a = img.detach().requires_grad_(True), pts.detach().requires_grad_(True), att.detach().requires_grad_(True)

            def fwd():
                with torch.no_grad():
                    return multiscale_deformable_attention(img, shp, pts, att, "zeros", False, level_shapes=shapes, **kw)

            def fwd_bwd():
                out = multiscale_deformable_attention(v, shp, p, a, "zeros", False, level_shapes=shapes, **kw)
                out.backward(grad)

            row[f"{tag}_fwd_ms"] = round(timed(fwd, args.reps), 4)
            row[f"{tag}_fwd_bwd_ms"] = round(timed(fwd_bwd, args.reps), 4)
            row[f"{tag}_kernels_us"] = kernels(fwd_bwd)
        row["fwd_ratio"] = round(row["ragged_fwd_ms"] / row["padded_fwd_ms"], 3)
        row["fwd_bwd_ratio"] = round(row["ragged_fwd_bwd_ms"] / row["padded_fwd_bwd_ms"], 3)
        row["fwd_ratio_spread"] = round(row["ragged_fwd_ms"] / row["padded_spread_fwd_ms"], 3)
        row["fwd_bwd_ratio_spread"] = round(row["ragged_fwd_bwd_ms"] / row["padded_spread_fwd_bwd_ms"], 3)
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
