"""Inputs on which the operator is EXACT, so DESIGN.md §5 (float coordinates, weights and accumulation for every
storage type, one rounding on store) can be held with no tolerance.  A helper module, not a conftest.

Every input is a short dyadic number: sampling points are odd multiples of 2^-loc_bits, attention weights multiples of
2^-attn_bits in [0, 1], `value` and `grad_out` small integers (or multiples of 2^-value_bits / 2^-grad_bits).  Every
intermediate quantity of a correct evaluation is then a multiple of 2^-f (f: `fractional_bits` below) bounded by the
condition sum S of absolute values, i.e. it has at most f + ceil(log2 S) significant bits.  While that `budget` stays
within float32's 24 bits nothing rounds — in any summation order, with or without FMA — and the fp64 oracle IS the
float32 result.  The only rounding left is the store to a 16-bit type, which `expected` applies once (torch's CPU
conversion: round to nearest even).

`checked_reference(name, pm, ac)` is what the GPU tests compare against: it asserts the precondition (budget <= 24 for
every tensor, float32 oracle == float64 oracle bitwise, no sample on an integer pixel coordinate) before it hands out
the cached fp64 reference.  A case that fails it is a broken fixture: nothing is dropped at run time.

The pixel lattice itself — samples ON integer pixel coordinates, where grad_loc jumps and the padding modes switch
corners and gradients off — has a kind of its own, "lattice" (`lattice_case`): there the precondition asks for the
opposite, at least half of the samples with a coordinate on an integer, and tests/test_lattice_cases.py shows that three
independent references agree on them bit for bit."""
import functools
import math
import zlib

import numpy as np
import torch

MODES = [("zeros", False), ("zeros", True), ("border", False), ("border", True)]
TENSORS = ("out", "grad_value", "grad_loc", "grad_attn")
F32_BITS = 24
F32, F64, BF16, F16 = torch.float32, torch.float64, torch.bfloat16, torch.float16


# ----------------------------------------------------------------------------------------- the generator
def _odd_multiples(rng, shape, bits, lo, hi):
    scale = 2 ** bits
    kmin, kmax = math.ceil((lo * scale - 1) / 2), math.floor((hi * scale - 1) / 2)
    return (2 * rng.integers(kmin, kmax + 1, size=shape) + 1) / scale


def _grid(rng, shape, vmax, bits):
    scale = 2 ** bits
    return rng.integers(-vmax * scale, vmax * scale + 1, size=shape) / scale


def exact_case(rng, B, Q, H, D, levels, P, *, loc_bits=7, attn_bits=2, vmax=3, gmax=3, lo=-0.3, hi=1.3, value_bits=0,
               grad_bits=0, dtype=np.float64):
    """The usual dict (value, shapes, loc, attn, grad_out) plus the generator's bit counts under "bits".

    `P` an int: loc [B, Q, H, L, P, 2], attn [B, Q, H, L, P].  `P` a list of per-level counts (the ragged
    `points_per_level` layout, also used by the discrete mode): loc [B, Q, H, S, 2], attn [B, Q, H, S] and "counts"."""
    I = sum(h * w for h, w in levels)  # noqa: E741
    L = len(levels)
    counts = None if isinstance(P, int) else [int(p) for p in P]
    pts = (L, P) if counts is None else (sum(counts),)
    attn = rng.integers(0, 2 ** attn_bits + 1, size=(B, Q, H) + pts) / 2 ** attn_bits
    attn.reshape(-1)[0] = 1.0   # 0 and 1 are always there, however small the tensor
    attn.reshape(-1)[-1] = 0.0
    c = dict(
        value=_grid(rng, (B, I, H, D), vmax, value_bits).astype(dtype),
        shapes=np.asarray(levels, dtype=np.int64),
        loc=_odd_multiples(rng, (B, Q, H) + pts + (2,), loc_bits, lo, hi).astype(dtype),
        attn=attn.astype(dtype),
        grad_out=_grid(rng, (B, Q, H, D), gmax, grad_bits).astype(dtype),
        bits=dict(loc=loc_bits, attn=attn_bits, value=value_bits, grad=grad_bits),
    )
    if counts is not None:
        c["counts"] = counts
    return c


def flood_case(rng, B, Q, H, D, levels, P, coords, **kw):
    """`exact_case` with every sample of level l moved into ONE bilinear cell: x and y drawn from coords[l] = (xs, ys),
    odd multiples of 2^-loc_bits that land in the same cell under both align modes."""
    c = exact_case(rng, B, Q, H, D, levels, P, **kw)
    for lvl, (xs, ys) in enumerate(coords):
        c["loc"][:, :, :, lvl, :, 0] = rng.choice(np.asarray(xs, dtype=np.float64), size=(B, Q, H, P))
        c["loc"][:, :, :, lvl, :, 1] = rng.choice(np.asarray(ys, dtype=np.float64), size=(B, Q, H, P))
    return c


# ----------------------------------------------------------------------------------------- ON the pixel lattice
# Full-lattice pyramids: power-of-two axes for align_corners=False, 2^k + 1 axes for align_corners=True (one-pixel axes
# included), so that every pixel coordinate -2, -1.5, ..., n + 1.5 is a short dyadic sampling point.
LATTICE_LEVELS = {False: [(4, 8), (2, 2), (1, 1), (1, 4)], True: [(5, 9), (3, 3), (2, 2), (1, 5)]}
UNIVERSAL_LEVELS = [(7, 5), (3, 6), (1, 3)]
# coordinates that sit on a kink whatever the size: 0 and 1 are px = 0 and px = n - 1 under align_corners, 0.5 is an integer
# pixel coordinate of every odd-sized axis in either mode; (value, share) and the off-lattice dyadic neighbours of the rest
UNIVERSAL_VALUES = ((0.0, 0.15), (0.5, 0.40), (1.0, 0.15), (-0.0, 0.15))
UNIVERSAL_NEIGHBOURS = (-1 / 32, 1 / 32, 15 / 32, 17 / 32, 31 / 32, 33 / 32)
LATTICE_LOC_BITS = {False: 4, True: 4, None: 5}  # pixel coordinates in halves on axes up to 8 (+ 1) pixels; the neighbours


def lattice_axis(n, align):
    """The sampling coordinates whose pixel coordinate on an axis of n pixels is -2, -1.5, ..., n + 1.5, exactly."""
    px = np.arange(-4, 2 * n + 4) / 2.0
    if align:
        assert n == 1 or (n - 1) & (n - 2) == 0, n
        return px / max(n - 1, 1)  # (one pixel: the coordinate is x * 0 whatever x)
    assert n & (n - 1) == 0, n
    return (px + 0.5) / n


def lattice_case(rng, B, Q, H, D, levels, P, *, align, attn_bits=2, vmax=3, gmax=3, dtype=np.float64):
    """`exact_case` whose sampling points sit ON the pixel lattice, where grad_loc is discontinuous and the padding modes
    switch corners and gradients off.  align False / True: a full lattice for that align_corners — per level every (x, y)
    pair of pixel coordinates -2, -1.5, ..., n + 1.5 at least once, dealt over batch, queries, heads and points.
    align None: levels of any size, most coordinates from UNIVERSAL_VALUES, the rest their off-lattice neighbours."""
    c = exact_case(rng, B, Q, H, D, levels, P, loc_bits=LATTICE_LOC_BITS[align], attn_bits=attn_bits, vmax=vmax, gmax=gmax, dtype=dtype)
    counts = c.get("counts") or [P] * len(levels)
    loc, s0 = c["loc"], 0
    for lvl, ((h, w), p) in enumerate(zip(levels, counts)):
        n = B * Q * H * p
        if align is None:
            vals = np.asarray([v for v, _ in UNIVERSAL_VALUES] + list(UNIVERSAL_NEIGHBOURS))
            rest = 1.0 - sum(s for _, s in UNIVERSAL_VALUES)
            prob = [s for _, s in UNIVERSAL_VALUES] + [rest / len(UNIVERSAL_NEIGHBOURS)] * len(UNIVERSAL_NEIGHBOURS)
            pts = vals[rng.choice(len(vals), size=(n, 2), p=prob)]  # (by index: -0.0 keeps its sign)
        else:
            xs, ys = lattice_axis(w, align), lattice_axis(h, align)
            pairs = np.stack(np.meshgrid(xs, ys, indexing="ij"), -1).reshape(-1, 2)
            assert n >= len(pairs), f"level {lvl}: {len(pairs)} lattice pairs, {n} samples"
            pts = np.resize(pairs, (n, 2))[rng.permutation(n)]
        pts = pts.reshape(B, Q, H, p, 2).astype(dtype)
        if "counts" in c:
            loc[:, :, :, s0:s0 + p] = pts
        else:
            loc[:, :, :, lvl] = pts
        s0 += p
    c["align"] = align
    return c


# ----------------------------------------------------------------------------------------- the cases the GPU file uses
PYRAMID = [(16, 16), (8, 8), (4, 4), (2, 2)]
# name: (kind, (B, Q, H, D, levels, P), generator keywords, 16-bit storage types the GPU file runs the case in)
CASES = {
    # the shape matrix (tests/test_gpu_parity.py: SHAPE_MATRIX), L * P <= 16
    # (points in [0, 1]: pixel coordinates still reach half a pixel beyond the first / last centre at every level, so the
    #  masked and clamped corners are there; with +-0.3 border padding zeroes so many location gradients of this
    #  power-of-two pyramid that under 5 % of fp16 grad_loc would round.  lds_q200 keeps +-0.3 on the same pyramid.)
    "d32_vec_g8": ("bilinear", (2, 70, 8, 32, PYRAMID, 4), dict(attn_bits=3, lo=0.0, hi=1.0), (F16, BF16)),
    "d64_vec_g16": ("bilinear", (1, 33, 4, 64, [(9, 7), (5, 4)], 3), dict(gmax=1, attn_bits=3), (F16, BF16)),
    "d8_vec_g4": ("bilinear", (2, 19, 3, 8, [(7, 9), (3, 4)], 5), {}, (F16, BF16)),
    "d5_scalar": ("bilinear", (2, 13, 3, 5, [(6, 4), (3, 2), (2, 5)], 3), dict(attn_bits=4), (F16, BF16)),
    "d1": ("bilinear", (1, 23, 2, 1, [(5, 6), (2, 3)], 3), dict(vmax=7, gmax=7, attn_bits=4), (F16, BF16)),
    "one_query": ("bilinear", (1, 1, 1, 32, [(4, 4), (3, 5)], 3), dict(vmax=5, gmax=5, attn_bits=3), (F16, BF16)),
    "many_levels": ("bilinear", (1, 6, 2, 8, [(7, 6), (3, 3), (5, 3), (1, 1), (3, 5), (2, 3), (5, 1), (1, 5)], 2),
                    dict(attn_bits=4),
                    (F16, BF16)),
    # forced kernel variants
    "lds_q200": ("bilinear", (2, 200, 4, 32, PYRAMID, 4), {}, (BF16,)),
    "b4_passes": ("bilinear", (4, 40, 4, 32, [(9, 7), (5, 4)], 4), {}, (BF16,)),
    "unaligned": ("bilinear", (1, 9, 2, 32, [(4, 4), (3, 2)], 2), {}, (BF16,)),
    # thousands of samples in one cell per level (level 0: cell (2, 2) of 6 x 7, level 1: cell (1, 1) of 4 x 4, under
    # both align modes); sizes chosen so that the weights keep more than 6 fractional bits in every mode
    # (vmax = gmax = 3, not 1: with +-1 values fewer than 5 % of `out` need rounding in bf16; the budget is 19 bits)
    "flood": ("flood", (2, 1024, 2, 32, [(6, 7), (4, 4)], 2),
              dict(loc_bits=4, attn_bits=1, vmax=3, gmax=3,
                   coords=[((7 / 16,), (7 / 16, 9 / 16)), ((7 / 16, 9 / 16),) * 2]), (BF16,)),
    # per-level point counts
    "ragged_363": ("bilinear", (2, 37, 2, 32, [(6, 5), (3, 4), (2, 2)], [3, 6, 3]), {}, (BF16,)),
    "ragged_125": ("bilinear", (2, 37, 2, 32, [(6, 5), (3, 4), (2, 2)], [1, 2, 5]), {}, (BF16,)),
    # discrete sampling: no bilinear weights, so value / grad_out carry the fractional bits that make the store round
    "discrete_363": ("discrete", (2, 37, 2, 32, [(8, 8), (4, 4), (2, 2)], [3, 6, 3]),
                     dict(attn_bits=5, value_bits=3, grad_bits=3), (BF16,)),
    "discrete_sorted": ("discrete", (1, 1200, 2, 32, [(32, 32), (16, 16), (8, 8)], [2, 4, 2]),
                        dict(attn_bits=5, value_bits=3, grad_bits=3, loc_bits=6), (BF16,)),
}
BILINEAR = [n for n, c in CASES.items() if c[0] in ("bilinear", "flood")]
DISCRETE = [n for n, c in CASES.items() if c[0] == "discrete"]

# the pixel lattice (kind "lattice", a precondition of its own below): B = 2, H = 2, Q = 384 — every (x, y) pair of level 0
# (24 x 16 and 25 x 17 pixel coordinates) at least three times.  "f" / "t": the full lattice of align_corners False / True,
# "u": the universal values; D = 32 (16-byte pieces) and D = 5 (the scalar path); "_c": per-level point counts
_ALL16 = (F16, BF16)
for _tag, _al in (("f", False), ("t", True)):
    _lv = LATTICE_LEVELS[_al]
    CASES[f"lat_{_tag}_d32"] = ("lattice", (2, 384, 2, 32, _lv, 1), dict(align=_al), _ALL16)
    CASES[f"lat_{_tag}_d5"] = ("lattice", (2, 384, 2, 5, _lv, 1), dict(align=_al), _ALL16)
    CASES[f"lat_{_tag}_d4"] = ("lattice", (2, 384, 2, 4, _lv, 1), dict(align=_al), _ALL16)
    CASES[f"lat_{_tag}_c"] = ("lattice", (2, 384, 2, 32, _lv, [2, 5, 1, 3]), dict(align=_al), _ALL16)
CASES["lat_u_d32"] = ("lattice", (2, 200, 2, 32, UNIVERSAL_LEVELS, 4), dict(align=None), _ALL16)
CASES["lat_u_d5"] = ("lattice", (2, 200, 2, 5, UNIVERSAL_LEVELS, 4), dict(align=None), _ALL16)
CASES["lat_u_c"] = ("lattice", (2, 200, 2, 32, UNIVERSAL_LEVELS, [2, 5, 3]), dict(align=None), _ALL16)
LATTICE = [n for n, c in CASES.items() if c[0] == "lattice"]


def lattice_modes(name):
    """The modes a lattice case is ON the lattice in: its own align_corners for a full lattice, all four otherwise."""
    align = CASES[name][2]["align"]
    return [(pm, ac) for pm, ac in MODES if align is None or ac == align]


LATTICE_RUNS = [(n, pm, ac) for n in LATTICE for pm, ac in lattice_modes(n)]
LATTICE_MIN_SHARE = 0.5

# the head-dimension sweep (tests/head_dim_cases.py says which template instantiation each D reaches in each storage type):
# the smallest shape that has two batch elements, two heads, two levels and a last workgroup that is not full, with
# three points per level ("hd<D>_p3"), with per-level counts [2, 5] ("hd<D>_c25") and sampled discretely ("hd<D>_disc").
# value and grad_out in {-1, 0, 1}: grad_loc sums D of them per sample, so D = 520 leaves no room for more (21 of 24 bits)
HEAD_DIMS = (17, 33, 34, 65, 66, 68, 72, 130, 132, 136, 260, 264, 520)
HEAD_DIM_BASE = (2, 11, 2, [(5, 4), (3, 2)])  # B, Q, H, levels
HEAD_DIM_COUNTS = [2, 5]
HEAD_DIM = []
for _d in HEAD_DIMS + (128, 256):  # (128, 256: the one-wave-per-unit forward's D / VEC of 32 and 64 in float32)
    _B, _Q, _H, _lv = HEAD_DIM_BASE
    _kw = dict(loc_bits=5, attn_bits=2, vmax=1, gmax=1)
    CASES[f"hd{_d}_p3"] = ("bilinear", (_B, _Q, _H, _d, _lv, 3), _kw, (F16, BF16))
    CASES[f"hd{_d}_c25"] = ("bilinear", (_B, _Q, _H, _d, _lv, HEAD_DIM_COUNTS), _kw, (F16, BF16))
    CASES[f"hd{_d}_disc"] = ("discrete", (_B, _Q, _H, _d, _lv, HEAD_DIM_COUNTS),
                             dict(attn_bits=5, value_bits=3, grad_bits=3), (BF16,))
    HEAD_DIM += [f"hd{_d}_p3", f"hd{_d}_c25", f"hd{_d}_disc"]
# the LDS-served levels at G = 32 and G = 64: Q as in lds_q200 (the variant's workgroups hold 1024 / G units)
for _d in (68, 132):
    CASES[f"hd{_d}_lds"] = ("bilinear", (2, 200, 2, _d, [(5, 4), (3, 2)], 3), dict(loc_bits=5, attn_bits=2, vmax=1, gmax=1), (BF16,))
    HEAD_DIM.append(f"hd{_d}_lds")
SHAPE_MATRIX = ["d32_vec_g8", "d64_vec_g16", "d8_vec_g4", "d5_scalar", "d1", "one_query", "many_levels"]


# name: f(case, rng) -> case, applied after the draw by a helper module that registers cases of its own here
# (tests/large_pyramid_cases.py re-draws the sampling points and plants samples at its trip cuts)
FINISH = {}


@functools.lru_cache(maxsize=None)
def get_case(name):
    """The case's fp64 inputs (cached; treat as read-only)."""
    kind, dims, kw, _ = CASES[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    c = {"flood": flood_case, "lattice": lattice_case}.get(kind, exact_case)(rng, *dims, **kw)
    if name in FINISH:
        c = FINISH[name](c, rng)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def storage_types(name):
    return CASES[name][3]


# ----------------------------------------------------------------------------------------- ragged layout <-> dense
def dense(c):
    """A ragged case zero-padded to max(P_l) points per level (weight 0, a location off the pixel grid); a uniform case
    as it is."""
    if "counts" not in c:
        return c
    counts, lb = c["counts"], c["bits"]["loc"]
    B, Q, H, _, _ = c["loc"].shape
    L, Pm = len(counts), max(counts)
    loc = np.full((B, Q, H, L, Pm, 2), (2 ** (lb - 1) + 1) / 2 ** lb, dtype=c["loc"].dtype)
    attn = np.zeros((B, Q, H, L, Pm), dtype=c["attn"].dtype)
    s0 = 0
    for lvl, p in enumerate(counts):
        loc[:, :, :, lvl, :p] = c["loc"][:, :, :, s0:s0 + p]
        attn[:, :, :, lvl, :p] = c["attn"][:, :, :, s0:s0 + p]
        s0 += p
    return dict(c, loc=loc, attn=attn)


def _unpad(t, counts):
    return np.concatenate([t[:, :, :, lvl, :p] for lvl, p in enumerate(counts)], axis=3)


def _oracle_all(oracle, c, pm, ac, dtype):
    d = dense(c)
    v, l, a, g = (np.asarray(d[k], dtype=dtype) for k in ("value", "loc", "attn", "grad_out"))
    out = oracle.forward(v, d["shapes"], l, a, pm, ac)
    gv, gl, ga = oracle.backward(g, v, d["shapes"], l, a, pm, ac)
    if "counts" in c:
        gl, ga = _unpad(gl, c["counts"]), _unpad(ga, c["counts"])
    return dict(out=out, grad_value=gv, grad_loc=gl, grad_attn=ga)


def _oracle():
    from oracle import msda_oracle
    msda_oracle.build()
    return msda_oracle


# ----------------------------------------------------------------------------------------- discrete: reference
def _discrete_all(c, fn, dtype):
    """out / grad_value / grad_attn of `fn(value, levels, loc, attn, counts)` (differentiable in value and attn)."""
    v = torch.from_numpy(np.array(c["value"])).to(dtype).requires_grad_(True)
    a = torch.from_numpy(np.array(c["attn"])).to(dtype).requires_grad_(True)
    loc = torch.from_numpy(np.array(c["loc"])).to(dtype)
    out = fn(v, [tuple(s) for s in c["shapes"].tolist()], loc, a, c["counts"])
    out.backward(torch.from_numpy(np.array(c["grad_out"])).to(out.dtype))
    return dict(out=out.detach().numpy(), grad_value=v.grad.numpy(), grad_attn=a.grad.numpy())


def _ref_discrete(value, levels, loc, attn, counts):
    from test_discrete_sampling import ref_discrete  # that file's own fp64 index formulation
    return ref_discrete(value, levels, loc, attn, counts)


def _index_discrete(value, levels, loc, attn, counts):
    """This module's own index formulation, every operation in the inputs' dtype (float32 for the precondition): sample
    by sample, out += attn * value[pixel]."""
    B, _, H, D = value.shape
    bi, hi = torch.arange(B).reshape(B, 1, 1), torch.arange(H).reshape(1, 1, H)
    out = torch.zeros(B, loc.shape[1], H, D, dtype=value.dtype)
    start = s0 = 0
    for (h, w), n in zip(levels, counts):
        for s in range(s0, s0 + n):
            ix = torch.clamp(torch.trunc(loc[..., s, 0] * w + 0.5), 0, w - 1).to(torch.int64)
            iy = torch.clamp(torch.trunc(loc[..., s, 1] * h + 0.5), 0, h - 1).to(torch.int64)
            out = out + attn[..., s, None] * value[bi, start + iy * w + ix, hi]
        start += h * w
        s0 += n
    return out


# ----------------------------------------------------------------------------------------- budget and precondition
def fractional_bits(bits):
    lb, ab, vb, gb = bits["loc"], bits["attn"], bits["value"], bits["grad"]
    return dict(out=ab + 2 * lb + vb, grad_value=ab + 2 * lb + gb, grad_attn=2 * lb + vb + gb, grad_loc=ab + lb + vb + gb)


def _magnitude_bits(s):
    s = float(np.max(s)) if np.size(s) else 0.0
    return max(0, math.ceil(math.log2(s))) if s > 0 else 0


def condition_sums(c, pm, ac):
    """The largest sum of absolute values behind an element of each result (bilinear cases)."""
    absd = dict(c, value=np.abs(c["value"]), attn=np.abs(c["attn"]), grad_out=np.abs(c["grad_out"]))
    r = _oracle_all(_oracle(), absd, pm, ac, np.float64)  # the bilinear weights are >= 0: these ARE the condition sums
    d = dense(c)
    size = d["shapes"].max(axis=1).astype(np.float64).reshape(1, 1, 1, -1, 1)
    g1 = np.abs(d["grad_out"]).sum(-1)[..., None, None]
    # grad_loc: max(h, w) * |a| * sum_d |g_d| * (4 corners) * max |v|  (an upper bound of the sum the issue names)
    gl = size * np.abs(d["attn"]) * g1 * 4.0 * float(np.abs(c["value"]).max())
    return dict(out=float(r["out"].max()), grad_value=float(r["grad_value"].max()), grad_attn=float(r["grad_attn"].max()),
                grad_loc=float(gl.max()))


def budget(c, pm, ac):
    """Significant bits each result needs, for any evaluation order: fractional bits + ceil(log2(condition sum))."""
    frac = fractional_bits(c["bits"])
    return {k: frac[k] + _magnitude_bits(s) for k, s in condition_sums(c, pm, ac).items()}


def pixel_coordinates(c, ac):
    """fp64 pixel-space coordinates of every sample of the (dense) case, [..., L, P, 2]."""
    d = dense(c)
    size = np.stack([d["shapes"][:, 1], d["shapes"][:, 0]], -1).astype(np.float64).reshape(1, 1, 1, -1, 1, 2)
    return d["loc"] * (size - 1) if ac else d["loc"] * size - 0.5


def real_samples(c, t):
    """A per-sample array of the dense layout ([B, Q, H, L, P, ...]) without the padding `dense` added, samples flattened."""
    t = _unpad(t, c["counts"]) if "counts" in c else t.reshape(t.shape[:3] + (-1,) + t.shape[5:])
    return t.reshape((-1,) + t.shape[4:])


def lattice_share(c, ac):
    """The share of the case's samples with x or y ON an integer pixel coordinate."""
    pix = pixel_coordinates(c, ac)
    return float(real_samples(c, (pix == np.round(pix)).any(-1)).mean())


POSITION_CLASSES = ("px < -1", "px = -1", "-1 < px < 0", "px = 0", "interior integer", "interior half", "px = n - 1",
                    "n - 1 < px < n", "px = n", "px > n")


def position_classes(px, n):
    """Per coordinate, a bool [10, ...]: which of POSITION_CLASSES the pixel coordinate px belongs to on an axis of n
    pixels (on one pixel, px = 0 is px = n - 1 as well, and -1 is never `n`: the classes are tested one by one)."""
    whole = px == np.round(px)
    inside = (px > 0) & (px < n - 1)
    return np.stack([px < -1, px == -1, (px > -1) & (px < 0), px == 0, inside & whole, inside & ~whole, px == n - 1,
                     (px > n - 1) & (px < n), px == n, px > n])


@functools.lru_cache(maxsize=None)
def reference(name, pm="border", ac=False):
    """The fp64 reference of a case (cached): the CPU oracle, or test_discrete_sampling.ref_discrete."""
    c = get_case(name)
    if CASES[name][0] == "discrete":
        return _discrete_all(c, _ref_discrete, F64)
    return _oracle_all(_oracle(), c, pm, ac, np.float64)


@functools.lru_cache(maxsize=None)
def precondition(name, pm="border", ac=False):
    """Asserts that the case is exact in float32; returns its budget."""
    c = get_case(name)
    ref = reference(name, pm, ac)
    if CASES[name][0] == "discrete":
        absd = dict(c, value=np.abs(c["value"]), attn=np.abs(c["attn"]), grad_out=np.abs(c["grad_out"]))
        sums = _discrete_all(absd, _ref_discrete, F64)
        b = c["bits"]
        frac = dict(out=b["attn"] + b["value"], grad_value=b["attn"] + b["grad"], grad_attn=b["value"] + b["grad"])
        bud = {k: frac[k] + _magnitude_bits(sums[k]) for k in frac}
        f32 = _discrete_all(c, _index_discrete, F32)  # evaluated in float32, independent of the package
    elif CASES[name][0] == "lattice":
        # The lattice has a kind of its own: its samples sit ON integer pixel coordinates by construction, where the
        # oracle, grid_sample's autograd and the gather formulation agree bit for bit (tests/test_lattice_cases.py), so
        # the rule below is replaced by its opposite — at least half of the samples have a coordinate on an integer, in
        # the modes the case is made for — and the inputs must survive every 16-bit storage type the case is run in.
        assert (pm, ac) in lattice_modes(name), f"{name}: not a lattice case under {pm} {ac}"
        share = lattice_share(c, ac)
        assert share >= LATTICE_MIN_SHARE, f"{name} {ac}: only {share:.1%} of the samples have a coordinate on an integer"
        for k in ("value", "loc", "attn", "grad_out"):
            t = torch.from_numpy(np.array(c[k]))
            for dt in storage_types(name) + (F32,):
                assert torch.equal(t.to(dt).double(), t), f"{name}: {k} does not survive {dt}"
        bud = budget(c, pm, ac)
        f32 = _oracle_all(_oracle(), c, pm, ac, np.float32)
    else:
        # no sample on an integer pixel coordinate, where grad_loc is discontinuous; an axis of ONE pixel under
        # align_corners is no exception to the rule but outside it: its coordinate is x * 0, zero in any arithmetic
        # (the lattice itself is held by the cases of kind "lattice", which have the branch above to themselves)
        pix = pixel_coordinates(c, ac)
        wh = np.stack([c["shapes"][:, 1], c["shapes"][:, 0]], -1).reshape(1, 1, 1, -1, 1, 2)
        on_grid = (pix == np.round(pix)) & ~((wh == 1) & bool(ac))
        assert not on_grid.any(), f"{name}: a sample sits on an integer pixel coordinate (grad_loc kink)"
        bud = budget(c, pm, ac)
        f32 = _oracle_all(_oracle(), c, pm, ac, np.float32)
    assert max(bud.values()) <= F32_BITS, f"{name} {pm} {ac}: budget {bud} exceeds float32's {F32_BITS} bits"
    for k, r in ref.items():
        assert f32[k].dtype == np.float32 and np.array_equal(f32[k].astype(np.float64), r), \
            f"{name} {pm} {ac}: the float32 and float64 references differ in {k}"
    return bud


def checked_reference(name, pm="border", ac=False):
    precondition(name, pm, ac)
    return reference(name, pm, ac)


def masked_reference(name, pm, ac, mask):
    """The reference of a value-mask call (`mask` [B, I] bool, True = real pixel): the oracle on where(mask, value, 0),
    grad_value zeroed in the padding rows.  Exact whenever the unmasked case is — the condition sums only shrink — and the
    float32 oracle is again held to the float64 one."""
    precondition(name, pm, ac)
    c = get_case(name)
    m = np.asarray(mask, dtype=bool)[:, :, None, None]
    pre = dict(c, value=np.where(m, c["value"], 0.0))
    ref = _oracle_all(_oracle(), pre, pm, ac, np.float64)
    f32 = _oracle_all(_oracle(), pre, pm, ac, np.float32)
    for k, r in ref.items():
        assert np.array_equal(f32[k].astype(np.float64), r), f"{name} {pm} {ac} masked: float32 and float64 differ in {k}"
    ref["grad_value"] = np.where(m, ref["grad_value"], 0.0)
    return ref


def expected(ref64, torch_dtype):
    """ref64 -> float32 (exact, by the precondition) -> the storage type, rounded to nearest even ONCE."""
    t = torch.from_numpy(np.array(ref64))
    if torch_dtype == F64:
        return t
    f32 = t.to(F32)
    assert torch.equal(f32.double(), t), "the reference is not a float32 number: the precondition was not checked"
    return f32.to(torch_dtype)


# ----------------------------------------------------------------------------------------- emulated wrong kernels (CPU)
def truncate(t32, dtype):
    """float32 -> 16-bit storage by TRUNCATION (toward zero) instead of round-to-nearest-even."""
    t32 = t32.to(F32).contiguous()
    if dtype == BF16:
        return (t32.view(torch.int32) & -65536).view(F32).to(BF16)
    r = t32.to(dtype)
    over = r.float().abs() > t32.abs()
    toward_zero = (r.view(torch.int16) - 1).view(dtype)  # sign-magnitude: one step smaller in magnitude
    return torch.where(over, toward_zero, r)


def taps(c, pm, ac, pix=None, cell=None):
    """The oracle's bilinear taps in numpy fp64 for the (dense) case: (index [4][B, Q, H, L, P] into the pyramid, mask
    [4], weight [4]), corners ordered 00, 01, 10, 11 (y, x).  pix / cell ([..., 2]): a mutant's pixel coordinates and its
    cell's corner 00 in place of the oracle's `pixel_coordinates` and their floor."""
    d = dense(c)
    pix = pixel_coordinates(c, ac) if pix is None else pix
    h = d["shapes"][:, 0].reshape(1, 1, 1, -1, 1)
    w = d["shapes"][:, 1].reshape(1, 1, 1, -1, 1)
    start = (np.cumsum(d["shapes"][:, 0] * d["shapes"][:, 1]) - d["shapes"][:, 0] * d["shapes"][:, 1]).reshape(1, 1, 1, -1, 1)
    x0, y0 = (np.floor(pix[..., 0]), np.floor(pix[..., 1])) if cell is None else (cell[..., 0], cell[..., 1])
    dx, dy = pix[..., 0] - x0, pix[..., 1] - y0
    idx, mask, wgt = [], [], []
    for oy, ox in ((0, 0), (0, 1), (1, 0), (1, 1)):
        x, y = x0 + ox, y0 + oy
        ok = (x >= 0) & (x <= w - 1) & (y >= 0) & (y <= h - 1) if pm == "zeros" else np.ones(x.shape, bool)
        xc, yc = np.clip(x, 0, w - 1).astype(np.int64), np.clip(y, 0, h - 1).astype(np.int64)
        idx.append(start + yc * w + xc)
        mask.append(ok)
        wgt.append((dy if oy else 1 - dy) * (dx if ox else 1 - dx))
    return idx, mask, wgt


def contributions(c, pm, ac, weight_fn=None, drop=None):
    """attn * bilinear sample per (b, q, h, l, p), fp64 [B, Q, H, L, P, D]; the forward sums them over (l, p).
    weight_fn: applied to each corner weight (a mutant's quantisation); drop = (corner, flat sample index): that corner
    of that sample contributes nothing."""
    d = dense(c)
    idx, mask, wgt = taps(c, pm, ac)
    B, _, H, D = d["value"].shape
    bi, hi = np.arange(B).reshape(B, 1, 1, 1, 1), np.arange(H).reshape(1, 1, H, 1, 1)
    total = 0.0
    for k in range(4):
        wk = wgt[k] if weight_fn is None else weight_fn(wgt[k])
        wk = np.where(mask[k], wk, 0.0)
        if drop is not None and drop[0] == k:
            wk = wk.copy()
            wk.reshape(-1)[drop[1]] = 0.0
        total = total + wk[..., None] * d["value"][bi, idx[k], hi]
    return d["attn"][..., None] * total


def smallest_corner_of_one_sample(c, pm, ac):
    """(corner, flat sample index): among the samples' smallest-weight corners (unmasked, weight > 0), the one that
    carries most — largest attention weight x corner weight x |value| — so that dropping it is as visible as dropping
    ONE smallest corner can be; chosen from the inputs alone."""
    d = dense(c)
    idx, mask, wgt = taps(c, pm, ac)
    B, _, H, D = d["value"].shape
    bi, hi = np.arange(B).reshape(B, 1, 1, 1, 1), np.arange(H).reshape(1, 1, H, 1, 1)
    w4 = np.stack([np.where(m & (w > 0), w, np.inf) for m, w in zip(mask, wgt)])
    k = np.argmin(w4, axis=0)
    wmin = np.take_along_axis(w4, k[None], 0)[0]
    rows = np.stack([np.abs(d["value"][bi, i, hi]).max(-1) for i in idx])
    carried = np.where(np.isfinite(wmin), wmin, 0.0) * np.take_along_axis(rows, k[None], 0)[0] * np.abs(d["attn"])
    flat = int(np.argmax(carried.reshape(-1)))
    assert carried.reshape(-1)[flat] > 0, "no sample whose smallest corner matters: the fixture has no teeth"
    return int(k.reshape(-1)[flat]), flat


# ----------------------------------------------------------------------------------------- location gradients, and wrong ones
# Emulated kernels that are right everywhere but ON the pixel lattice (tests/test_lattice_cases.py): the padding mode each
# can show in, None = both
LATTICE_MUTANTS = {
    # the reference's Triton kernel: the clamped-corner formula with no gate, which is `px >= 0` where the oracle has `>`
    "border_gradient_alive_at_zero": "border",
    # the left-hand cell at integer coordinates: x0 = ceil(px) - 1, dx = 1
    "left_cell_at_integers": None,
    # "zeros" treating the cell x0 = -1 as outside when dx = 0: px = -1 loses its gradient (its weights ARE all zero)
    "zeros_drops_minus_one": "zeros",
    # "border" with the coordinate clamped FIRST and cell and fraction taken from the clamped coordinate, the cell kept
    # inside the image (x0 <= n - 2), the gradient alive wherever the clamp left the coordinate alone: alive at 0 and n - 1
    "border_gradient_after_clamp": "border",
}


def location_gradients(c, pm, ac, rule=None):
    """grad_loc of the (dense) case in numpy fp64, [B, Q, H, L, P, 2], by the oracle's expression; rule: one of
    LATTICE_MUTANTS in its place."""
    assert rule is None or rule in LATTICE_MUTANTS, rule
    d = dense(c)
    pix = pixel_coordinates(c, ac)
    n = np.stack([d["shapes"][:, 1], d["shapes"][:, 0]], -1).astype(np.float64).reshape(1, 1, 1, -1, 1, 2)
    border = pm == "border"
    alive = ((pix > 0) & (pix < n - 1)) if border else np.ones(pix.shape, bool)
    at, cell = pix, None
    if rule == "border_gradient_alive_at_zero" and border:
        alive = np.ones(pix.shape, bool)
    elif rule == "left_cell_at_integers":
        cell = np.ceil(pix) - 1
    elif rule == "zeros_drops_minus_one" and not border:
        alive = np.broadcast_to((pix > -1).all(-1, keepdims=True), pix.shape)
    elif rule == "border_gradient_after_clamp" and border:
        at = np.clip(pix, 0, n - 1)
        cell = np.maximum(np.minimum(np.floor(at), n - 2), 0)
        alive = at == pix
    idx, mask, _ = taps(c, pm, ac, at, cell)
    x0, y0 = (np.floor(at[..., 0]), np.floor(at[..., 1])) if cell is None else (cell[..., 0], cell[..., 1])
    dx, dy = (at[..., 0] - x0)[..., None], (at[..., 1] - y0)[..., None]
    B, _, H, D = d["value"].shape
    bi, hi = np.arange(B).reshape(B, 1, 1, 1, 1), np.arange(H).reshape(1, 1, H, 1, 1)
    v00, v01, v10, v11 = (np.where(m[..., None], d["value"][bi, i, hi], 0.0) for i, m in zip(idx, mask))
    g = d["grad_out"][:, :, :, None, None, :]
    gx = (g * ((1 - dy) * (v01 - v00) + dy * (v11 - v10))).sum(-1)
    gy = (g * ((1 - dx) * (v10 - v00) + dx * (v11 - v01))).sum(-1)
    scale = n - 1 if ac else n
    return np.where(alive, d["attn"][..., None] * scale * np.stack([gx, gy], -1), 0.0)


def real_grad_loc(c, gl):
    """`location_gradients`' dense result in the case's own layout (the oracle's grad_loc)."""
    return _unpad(gl, c["counts"]) if "counts" in c else gl
