"""Hostile sampling inputs: case builders shared by tests/test_hostile_cases.py (CPU: the expectations belong to the
operation) and tests/test_gpu_hostile_inputs.py (GPU: the kernels keep them).  DESIGN.md §5a states the contract.

A case starts from ``test_gpu_parity.rand_case`` on a shape with B >= 2 (a B = 1 shape of the suite's tables is taken with
B = 2) and plants hostile values into the samples of a chosen set of queries of BATCH ELEMENT 0 ONLY — at most
``MAX_HOSTILE_FRACTION`` (a quarter) of its queries, asserted by every builder.  The base case is the "benign replacement".

FAR — finite, far out of range or at the edge of a number format: +-1e30, +-3.0e38, +-65504, -0.0, 1e-45 and +-2^k / n for
k in {24, 31, 32, 33, 63, 64}, n the level's size on that axis (w_l for x, h_l for y): with power-of-two level sizes the
pixel coordinate lands exactly on the marks at which a 32- or 64-bit conversion before the clamp would wrap to a
valid-looking pixel.  NONFINITE — NaN, +Inf, -Inf; in x only, in y only, in both (cycling over the samples of a hostile
query) and, separately, in the attention weight.  Values that do not fit float16 become +-Inf on the cast: that is the AMP
case, kept and classified as non-finite (``classify``).  The same holds one step later: the kernels, the float32 oracle and
the reference compute the PIXEL coordinate ``x * w - 0.5`` in float32 for every storage type but float64, and for +-3.0e38
that product overflows to +-Inf for every w >= 2 — the bilinear fraction is then ``inf - inf``.  Such a value is finite as
an input and non-finite in the operation's own arithmetic, so it is kept and classified as non-finite too
(``overflow_case``: containment is what is asserted for it); with float64 arithmetic it stays a FAR value.

For the fused families the same values go into ``proj``'s offset channels, its logit channel, or one coordinate of the
reference point / box of the hostile queries.
"""
import zlib

import numpy as np
import torch

MAX_HOSTILE_FRACTION = 0.25
WRAP_EXPONENTS = (24, 31, 32, 33, 63, 64)
FAR_CONSTANTS = (1e30, -1e30, 3.0e38, -3.0e38, 65504.0, -65504.0, -0.0, 1e-45)
NONFINITE = {"nan": float("nan"), "pinf": float("inf"), "ninf": float("-inf")}
NP_DTYPE = {torch.float32: np.float32, torch.float64: np.float64, torch.float16: np.float32, torch.bfloat16: np.float32}


def hostile_queries(Q, seed=0):
    """the hostile queries of batch element 0: a seeded, sorted choice of floor(Q / 4) of them (at least one)"""
    n = max(1, int(Q * MAX_HOSTILE_FRACTION))
    assert Q >= 4 and n <= Q * MAX_HOSTILE_FRACTION, f"Q = {Q}: cannot keep the hostile queries to a quarter"
    hq = np.sort(np.random.default_rng(seed).choice(Q, size=n, replace=False))
    assert len(hq) <= MAX_HOSTILE_FRACTION * Q
    return hq


def base_case(B, Q, H, D, levels, P, seed, dtype=np.float32):
    from test_gpu_parity import rand_case
    assert B >= 2
    return rand_case(np.random.default_rng(seed), B, Q, H, D, levels, P, dtype=dtype)


def far_values(n):
    """the FAR list for an axis of n pixels"""
    return list(FAR_CONSTANTS) + [sgn * 2.0 ** k / n for k in WRAP_EXPONENTS for sgn in (1.0, -1.0)]


def rounds_finite(v, storage):
    """does the value stay finite when it is stored as `storage` (a torch dtype)"""
    return bool(torch.isfinite(torch.tensor(v, dtype=torch.float64).to(storage)))


def arithmetic_of(storage):
    """the type the operation computes coordinates in: float64 for float64 storage, float32 for everything else"""
    return torch.float64 if storage == torch.float64 else torch.float32


def stays_far(v, n, storage):
    """is `v` a FAR coordinate on an axis of n pixels when stored as `storage`: finite in storage, and its pixel
    coordinate (at most |v| * n) finite in the arithmetic type"""
    t = torch.tensor(v, dtype=torch.float64).to(storage).to(arithmetic_of(storage))
    return bool(torch.isfinite(t)) and bool(torch.isfinite(t * n))


def _plant_coordinates(c, hq, storage, far):
    """the values of the FAR list that stay far in `storage` (`far` true) or that do not, into the coordinates of the hostile
    queries' samples, cycling through the list of the sample's level and axis; every third coordinate stays benign (a far x
    next to an in-range y is the case "border" interpolates).  -> (case, coordinates planted)"""
    c = {k: v.copy() for k, v in c.items()}
    loc = c["loc"]
    _, _, H, L, P, _ = loc.shape
    planted = 0
    for l in range(L):
        h, w = (int(x) for x in c["shapes"][l])
        for axis, n in ((0, w), (1, h)):
            vals = [v for v in far_values(n) if stays_far(v, n, storage) == far]
            if not vals:
                continue
            k = l + axis  # (another phase per level and axis: every value meets every position over the queries)
            for q in hq:
                for hd in range(H):
                    for p in range(P):
                        k += 1
                        if k % 3 == 0:
                            continue
                        loc[0, q, hd, l, p, axis] = vals[k % len(vals)]
                        planted += 1
    assert np.isfinite(loc).all()  # finite as an input, whatever the operation makes of it
    return c, planted


def far_case(c, hq, storage=torch.float32):
    """FAR values into the hostile queries: only those that stay FAR in `storage` (``stays_far``; the rest is
    ``overflow_case``)."""
    c, planted = _plant_coordinates(c, hq, storage, True)
    assert planted > 0
    return c


def nonfinite_case(c, hq, value, where):
    """`value` (NaN / +-Inf) into the hostile queries: where = "loc": x only, y only, both, cycling over a query's samples,
    every fourth sample benign; where = "attn": the attention weight of every second sample.
    -> (case, planted): planted is the bool mask [B, Q, H, L, P] of the samples that were touched."""
    c = {k: v.copy() for k, v in c.items()}
    B, Q, H, L, P, _ = c["loc"].shape
    planted = np.zeros((B, Q, H, L, P), dtype=bool)
    k = 0
    for q in hq:
        for hd in range(H):
            for l in range(L):
                for p in range(P):
                    k += 1
                    if where == "attn":
                        if k % 2:
                            c["attn"][0, q, hd, l, p] = value
                            planted[0, q, hd, l, p] = True
                        continue
                    m = k % 4
                    if m == 3:
                        continue
                    if m in (0, 2):
                        c["loc"][0, q, hd, l, p, 0] = value
                    if m in (1, 2):
                        c["loc"][0, q, hd, l, p, 1] = value
                    planted[0, q, hd, l, p] = True
    assert planted[0].any() and not planted[1:].any()
    return c, planted


def neutralised(c, planted):
    """item 4's reference input: the planted samples replaced by (loc 0.5, weight 0)"""
    c = {k: v.copy() for k, v in c.items()}
    c["loc"][planted] = 0.5
    c["attn"][planted] = 0.0
    return c


def overflow_case(c, hq, storage):
    """The FAR values that do NOT stay far in `storage` — finite float32 inputs that become +-Inf on the cast to the
    storage type (float16 under AMP) or whose pixel coordinate overflows the arithmetic type (+-3.0e38 in float32).  None
    where every value stays far (float64)."""
    c, planted = _plant_coordinates(c, hq, storage, False)
    return c if planted else None


def classify(c, storage=torch.float32):
    """-> bool [B, Q]: the queries with a location or weight that is non-finite once the case is stored as `storage`, or
    whose pixel coordinate is non-finite in the arithmetic type"""
    arith = arithmetic_of(storage)
    loc = torch.from_numpy(c["loc"]).to(storage).to(arith)
    attn = torch.from_numpy(c["attn"]).to(storage)
    size = torch.from_numpy(np.asarray(c["shapes"])[:, ::-1].copy()).to(arith)[:, None, :]     # [L, 1, (w, h)]
    ok = torch.isfinite(loc) & torch.isfinite(loc * size)
    return (~(ok.flatten(2).all(-1) & torch.isfinite(attn).flatten(2).all(-1))).numpy()


def check_plant(c, base, hq):
    """what every builder promises: batch elements other than 0 and the clean queries of element 0 are untouched"""
    clean = np.ones(base["loc"].shape[1], dtype=bool)
    clean[hq] = False
    assert len(hq) <= MAX_HOSTILE_FRACTION * base["loc"].shape[1]
    for k in ("loc", "attn"):
        assert np.array_equal(c[k][1:], base[k][1:], equal_nan=True), k
        assert np.array_equal(c[k][0][clean], base[k][0][clean], equal_nan=True), k
    for k in ("value", "grad_out", "shapes"):
        assert np.array_equal(c[k], base[k]), k
    return clean


# ----------------------------------------------------------------------------------------- the fused families
def plant_fused(proj, ref, hq, values, where):
    """hostile values into the hostile queries of batch element 0 of a fused family's inputs (torch tensors, any layout
    whose first two axes are [B, Q]; `proj`'s last axis is (x offset, y offset, logit)).  where = "offset": cycling over the
    offset channels, every third one benign; "logit": every second sample's logit; "ref": coordinate 0 of the reference
    point / box (every level's, for per-level reference points).  Returns new tensors."""
    proj, ref = proj.clone(), ref.clone()
    values = list(values)
    hq_t = torch.as_tensor(np.asarray(hq), dtype=torch.int64)
    if where == "ref":
        for i, q in enumerate(hq):
            ref[0, int(q)].reshape(-1, ref.shape[-1])[:, 0] = values[i % len(values)]
        return proj, ref
    rows = proj[0, hq_t]                                  # [n, H, ..., 3] (a copy)
    flat = rows.reshape(len(hq), -1, 3)
    n_s = flat.shape[1]
    k = torch.arange(len(hq) * n_s).reshape(len(hq), n_s)
    vals = torch.tensor(values, dtype=torch.float64)
    if where == "logit":
        sel = (k % 2) == 1
        flat[..., 2] = torch.where(sel, vals[k % len(vals)].to(flat.dtype), flat[..., 2])
    else:
        assert where == "offset"
        for ch in (0, 1):
            kk = 2 * k + ch
            sel = (kk % 3) != 0
            flat[..., ch] = torch.where(sel, vals[kk % len(vals)].to(flat.dtype), flat[..., ch])
    proj[0, hq_t] = flat.reshape(rows.shape)
    return proj, ref


def fused_far_values(storage=torch.float32, overflowing=False):
    """the FAR list (wrap marks for a level size of 16) for the fused inputs, as stored in `storage`.  The kernels form
    the coordinate from it (ref + offset / size, ...) and then the pixel coordinate, in float32 unless everything is
    float64; +-3.0e38 overflows there on some level and axis (a factor h / w > 1.13 is enough), so with float32 arithmetic
    it belongs to the other list — `overflowing=True`: the values that become non-finite."""
    far = [v for v in far_values(16) if stays_far(v, 32, storage)]
    return [v for v in far_values(16) if v not in far] if overflowing else far


def seed_of(*parts):
    return zlib.crc32("/".join(str(p) for p in parts).encode())


# ----------------------------------------------------------------------------------------- the shapes: one per code path
def plain_shapes():
    """name -> (B, Q, H, D, levels, P, storage dtype): the suite's own shapes, B raised to 2 where the table has 1"""
    from test_gpu_lds_levels import CASES
    from test_gpu_parity import SHAPE_MATRIX
    out = {k: SHAPE_MATRIX[k] + (torch.float32,) for k in ("d32_vec_g8", "d5_scalar")}
    out.update({k: CASES[k] for k in ("c2_like_f32", "bf16_g4", "fp16_d64", "f64")})
    return {k: (max(2, v[0]),) + tuple(v[1:]) for k, v in out.items()}


def plain_case(name):
    """-> (base case as numpy in the arithmetic dtype, hostile queries, storage dtype)"""
    B, Q, H, D, levels, P, storage = plain_shapes()[name]
    c = base_case(B, Q, H, D, levels, P, seed_of("hostile", name), NP_DTYPE[storage])
    return c, hostile_queries(Q, seed_of("hq", name)), storage
