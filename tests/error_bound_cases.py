"""Generic (rounding) inputs with a DERIVED per-element error bound, between the bit-for-bit fixtures of
tests/exact_cases.py (nothing rounds) and the smoke tolerances of tests/test_gpu_parity.py.  A helper module, not a conftest.

The evaluator (`Ev`) is a running first-order error analysis in numpy fp64: `val` is the fp64 value, `err` a bound on
|computed - val| for an evaluation in a working precision of unit roundoff `U` = 2^-24 (float arithmetic, which the
kernels use for every storage type).  Inputs carry err = 0 — the fixtures are rounded to their storage type
first, so they are exactly what the kernel reads — every operation propagates its operands' errors to first order and adds
U * |val| for its own rounding, a sum of n terms in ANY order or tree adds (n - 1) * U * sum |val_i|, and the final bound is
multiplied by 1 + 2^-10 for the second-order terms (`Ev.sum` asserts n * U <= 2^-10, which makes that factor enough).
The error of a sample's pixel coordinate (and the 20-bit quantisation of the sorted grad_value records) enters through the
ANALYTIC derivative of each result with respect to that coordinate — the correlated first-order term, not the triangle
inequality over the four corners.

A formula written as a fully distributed sum of products bounds every factored form of it (`w * (a + b)` rounds once where
`w * a + w * b` rounds twice on parts whose magnitudes sum to at least as much), so one model covers the all-reduce and the
reduce-scatter bodies of the sample-gradient kernel, FMA chains and packed FMAs alike.  No operation count or constant
below comes from a GPU result: each cites the kernel line or the DESIGN.md section it models.

fp64 kernels are out of scope: an fp64 reference cannot bound an fp64 kernel."""
import functools
import zlib

import numpy as np
import torch

import exact_cases as ec
from exact_cases import BF16, F16, F32, MODES  # noqa: F401  (re-exported for the test files)

U = 2.0 ** -24               # unit roundoff of float arithmetic (round to nearest)
SECOND_ORDER = 1.0 + 2.0 ** -10
QUANT20 = 2.0 ** -21         # half a step of the sorted records' 20-bit fractions (msda_value_sorted.hpp:65-66: "+ 0.5f", truncating cast)
KINK_MARGIN = 4.0            # a sample within KINK_MARGIN * e_px of a discontinuity is left out of the affected tensors
MAX_EXCLUDED = 0.01          # ... and at most this share of a fixture's samples may be (a CONDITION on the fixture)
# storage name: (value / grad_value storage, storage of everything else) — tests/test_gpu_exact_numerics.py: STORAGE, less f64
STORAGE = {"f32": (F32, F32), "fp16": (F16, F16), "bf16": (BF16, BF16), "f32_vbf16": (BF16, F32), "f32_vf16": (F16, F32)}


# ----------------------------------------------------------------------------------------- the evaluator
class Ev:
    """A value with a first-order error bound (numpy fp64 arrays, broadcasting like numpy)."""
    __slots__ = ("val", "err")

    def __init__(self, val, err=0.0):
        self.val = np.asarray(val, dtype=np.float64)
        self.err = np.broadcast_to(np.asarray(err, dtype=np.float64), self.val.shape)

    @staticmethod
    def of(x):
        return x if isinstance(x, Ev) else Ev(x)

    def _rounded(self, val, err):
        return Ev(val, err + U * np.abs(val))

    def __add__(self, o):
        o = Ev.of(o)
        return self._rounded(self.val + o.val, self.err + o.err)

    def __sub__(self, o):
        o = Ev.of(o)
        return self._rounded(self.val - o.val, self.err + o.err)

    def __rsub__(self, o):
        return Ev.of(o) - self

    def __mul__(self, o):
        o = Ev.of(o)
        return self._rounded(self.val * o.val, np.abs(self.val) * o.err + np.abs(o.val) * self.err)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Ev.of(o)
        q = self.val / o.val
        return self._rounded(q, self.err / np.abs(o.val) + np.abs(q) * o.err / np.abs(o.val))

    def __neg__(self):
        return Ev(-self.val, self.err)

    def __getitem__(self, i):
        return Ev(self.val[i], self.err[i])

    def where(self, keep):
        """The value where `keep`, an exact 0 elsewhere (a masked corner, a gradient the border gate switched off)."""
        return Ev(np.where(keep, self.val, 0.0), np.where(keep, self.err, 0.0))

    @staticmethod
    def check_terms(n):
        assert np.max(n) * U <= 2.0 ** -10, f"a sum of {np.max(n)} terms: the second-order factor 1 + 2^-10 would not cover it"

    def sum(self, axes, n=None):
        """The sum over `axes` in any order and tree: sum err_i + (n - 1) * U * sum |val_i|.  n: the number of real terms
        where the array holds padding (exact zeros) next to them; default: the number of summed elements."""
        axes = (axes,) if isinstance(axes, int) else tuple(axes)
        if n is None:
            n = int(np.prod([self.val.shape[a] for a in axes]))
        Ev.check_terms(n)
        return Ev(self.val.sum(axes), self.err.sum(axes) + (n - 1) * U * np.abs(self.val).sum(axes))


def stack(evs, axis=-1):
    return Ev(np.stack([e.val for e in evs], axis), np.stack([np.broadcast_to(e.err, e.val.shape) for e in evs], axis))


def bound(e):
    """What a test compares against: the first-order bound times the second-order factor."""
    return e.err * SECOND_ORDER


def half_spacing(mag, dtype):
    """Half the spacing of `dtype` at the magnitude `mag` (fp64, >= 0): the one rounding on store.  Taken from the cast
    value's own neighbour (integer step on the bit pattern), so it is right in the subnormal range; `mag` is first rounded
    UP to float32 and then truncated to `dtype`, which names the binade the unrounded result lies in."""
    if dtype == F32:
        return np.zeros_like(mag)
    m32 = np.nextafter(np.asarray(mag, dtype=np.float64).astype(np.float32), np.float32(np.inf))
    t = ec.truncate(torch.from_numpy(np.ascontiguousarray(m32)), dtype)
    up = (t.view(torch.int16) + 1).view(dtype)
    sp = (up.double() - t.double()).numpy()
    assert np.isfinite(sp).all(), "a result at the top of the storage type's range: the fixture must stay below half of it"
    return 0.5 * sp


# ----------------------------------------------------------------------------------------- fixtures
LEVELS = [(6, 5), (3, 4), (1, 7)]  # (h, w): no power-of-two axis but the one-pixel one, so x * w and off / w round
# name: dict(B, Q, H, D, levels, P (int or per-level counts), kind)
FIXTURES = {
    "d32": dict(B=2, Q=37, H=3, D=32, levels=LEVELS, P=2, kind="plain"),      # the vector path
    "d5": dict(B=2, Q=37, H=3, D=5, levels=LEVELS, P=2, kind="plain"),        # the scalar path
    "d64": dict(B=2, Q=37, H=3, D=64, levels=LEVELS, P=2, kind="plain"),      # 16 lanes per unit
    "counts": dict(B=2, Q=37, H=3, D=32, levels=LEVELS, P=[3, 1, 2], kind="plain"),
    # grad_value sums of hundreds of terms on 16 pixels; every sample strictly inside the image under both align modes
    "long_sum": dict(B=4, Q=512, H=2, D=32, levels=[(4, 4)], P=4, kind="interior"),
    # magnitudes over 24 binades, random signs: heavy cancellation.  "range_h": the same within what fp16 can hold
    "range": dict(B=2, Q=37, H=3, D=32, levels=LEVELS, P=2, kind="range", vexp=(-12, 12), gexp=(-12, 12)),
    "range_h": dict(B=2, Q=37, H=3, D=32, levels=LEVELS, P=2, kind="range", vexp=(-12, 4), gexp=(-12, 0)),
    "discrete": dict(B=2, Q=37, H=3, D=32, levels=LEVELS, P=[3, 1, 2], kind="discrete"),
}
PLAIN = [n for n, f in FIXTURES.items() if f["kind"] != "discrete"]
# Added to a fixture's seed where the first draw left more than MAX_EXCLUDED of its samples near a discontinuity in some
# storage type.  Chosen on the CPU from the fp64 reference alone (tests/test_error_bound_cases.py asserts the cap for every
# fixture).
SEEDS = {"discrete": 3}


def _log_uniform(rng, shape, lo, hi):
    return np.exp2(rng.uniform(lo, hi, size=shape)) * rng.choice([-1.0, 1.0], size=shape)


@functools.lru_cache(maxsize=None)
def raw_case(name):
    """The fixture's inputs before they are rounded to a storage type (fp64, read-only)."""
    f = FIXTURES[name]
    rng = np.random.default_rng(zlib.crc32(("error_bound_" + name).encode()) + SEEDS.get(name, 0))
    B, Q, H, D, levels = f["B"], f["Q"], f["H"], f["D"], f["levels"]
    counts = None if isinstance(f["P"], int) else list(f["P"])
    pts = (len(levels), f["P"]) if counts is None else (sum(counts),)
    I = sum(h * w for h, w in levels)  # noqa: E741
    lo, hi = (0.2, 0.8) if f["kind"] == "interior" else (-0.15, 1.15)
    if f["kind"] == "range":
        value = _log_uniform(rng, (B, I, H, D), *f["vexp"])
        grad = _log_uniform(rng, (B, Q, H, D), *f["gexp"])
        attn = np.exp2(rng.uniform(-6, 0, size=(B, Q, H) + pts))
    else:
        value = rng.standard_normal((B, I, H, D))
        grad = rng.standard_normal((B, Q, H, D))
        attn = rng.uniform(0.02, 1.0, size=(B, Q, H) + pts)
    c = dict(value=value, shapes=np.asarray(levels, dtype=np.int64), loc=rng.uniform(lo, hi, size=(B, Q, H) + pts + (2,)),
             attn=attn, grad_out=grad)
    if counts is not None:
        c["counts"] = counts
        c["bits"] = dict(loc=5)  # (exact_cases.dense pads with weight 0 at the location 17 / 32, on no pixel boundary here)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def _through(a, dtype):
    return torch.from_numpy(np.array(a)).to(dtype).double().numpy()


@functools.lru_cache(maxsize=None)
def get_case(name, storage="f32"):
    """The fixture rounded to the storage types of `storage`, in fp64: exactly the numbers the kernel reads."""
    vdt, cdt = STORAGE[storage]
    c = dict(raw_case(name))
    c["value"] = _through(c["value"], vdt)
    for k in ("loc", "attn", "grad_out"):
        c[k] = _through(c[k], cdt)
    if cdt != F32 and FIXTURES[name]["kind"] != "discrete":
        c["loc"] = _off_the_lattice(c, cdt)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def _off_the_lattice(c, dtype):
    """16-bit sampling points have 8 or 11 significant bits, so on an axis of 4 pixels x * 4 - 0.5 is an INTEGER for one
    bf16 coordinate in 64: far more than MAX_EXCLUDED of the samples would sit on a kink (tests/exact_cases.py's lattice
    cases hold those).  A coordinate that does, under either align mode, moves to the next number of its storage type —
    decided from the fp64 pixel coordinates alone, before anything is evaluated."""
    loc = np.array(c["loc"])
    for _ in range(4):
        cc = dict(c, loc=loc)
        d = ec.dense(cc)
        near = np.zeros(d["loc"].shape, bool)
        for ac in (False, True):
            pix = ec.pixel_coordinates(cc, ac)
            near |= np.abs(pix - np.round(pix)) < KINK_MARGIN * pixel_error(d, ac)
        near = ec.real_grad_loc(cc, near) if "counts" in c else near
        if not near.any():
            break
        t = torch.from_numpy(loc).to(dtype)
        loc = torch.where(torch.from_numpy(near), (t.view(torch.int16) + 1).view(dtype), t).double().numpy()
    return loc


def masked_case(c, vmask=None, qmask=None):
    """The pre-masked problem of a value_mask / query_mask call: padded pixels hold zeros, a padded query's weights and
    grad_out rows are zero (its out rows and gradients are then zero, and it adds nothing to grad_value)."""
    c = dict(c)
    if vmask is not None:
        c["value"] = np.where(np.asarray(vmask, bool)[:, :, None, None], c["value"], 0.0)
    if qmask is not None:
        qm = np.asarray(qmask, bool)
        c["attn"] = np.where(qm.reshape(qm.shape + (1,) * (c["attn"].ndim - 2)), c["attn"], 0.0)
        c["grad_out"] = np.where(qm[:, :, None, None], c["grad_out"], 0.0)
    return c


# ----------------------------------------------------------------------------------------- coordinates and their error
def _sizes(d):
    """(w, h) per level, broadcast over [B, Q, H, L, P, 2]."""
    return np.stack([d["shapes"][:, 1], d["shapes"][:, 0]], -1).astype(np.float64).reshape(1, 1, 1, -1, 1, 2)


def _dense_like(c, t, fill=0.0):
    """A per-sample array in the case's own layout ([B, Q, H, S, ...] with counts) in the dense one ([B, Q, H, L, Pmax, ...])."""
    if "counts" not in c:
        return t
    counts = c["counts"]
    out = np.full(t.shape[:3] + (len(counts), max(counts)) + t.shape[4:], fill, dtype=t.dtype)
    s0 = 0
    for lvl, p in enumerate(counts):
        out[:, :, :, lvl, :p] = t[:, :, :, s0:s0 + p]
        s0 += p
    return out


def pixel_error(d, ac, loc_err=None):
    """e_px, [B, Q, H, L, P, 2]: the error of the float pixel coordinate; loc_err: the error the sampling point itself
    arrives with (a fused prologue formed it), scaled by the level's size on top.  align_corners: `x * (W - 1)`, one rounded
    multiply (W - 1 is exact) — U |x| (W - 1).  Otherwise `x * W - 0.5` (msda_common.hpp:305-306), a rounded multiply and a
    rounded subtraction, or under -ffp-contract=fast one FMA (msda_value_sorted.hpp:133-134 spells it out): both are within
    U |x| W + U |x W - 0.5| <= 2 U (|x| W + 0.5)."""
    n = _sizes(d)
    x = np.abs(d["loc"])
    own = U * x * (n - 1) if ac else 2 * U * (x * n + 0.5)
    return own if loc_err is None else own + loc_err * (n - 1 if ac else n)


def kink_samples(c, ac, loc_err=None):
    """bool [B, Q, H, L, P] of the (dense) case: the sample's fp64 pixel coordinate lies within KINK_MARGIN * e_px of an
    integer in x or y — where the cell changes, grad_loc jumps and the border gate switches.  (An axis of one pixel under
    align_corners has the coordinate x * 0 = 0 in any arithmetic: e_px = 0 and nothing is near.)"""
    d = ec.dense(c)
    pix = ec.pixel_coordinates(c, ac)
    le = None if loc_err is None else _dense_like(c, loc_err)
    return (np.abs(pix - np.round(pix)) < KINK_MARGIN * pixel_error(d, ac, le)).any(-1)


def excluded_share(c, ac, loc_err=None):
    return float(ec.real_samples(c, kink_samples(c, ac, loc_err)).mean())


# ----------------------------------------------------------------------------------------- the plain operator
def _gather(d, idx):
    B, _, H, _ = d["value"].shape
    bi, hi = np.arange(B).reshape(B, 1, 1, 1, 1), np.arange(H).reshape(1, 1, H, 1, 1)
    return d["value"][bi, idx, hi]


def _real_terms(c):
    return sum(c["counts"]) if "counts" in c else c["loc"].shape[3] * c["loc"].shape[4]


def _unpad_ev(c, e):
    return Ev(ec.real_grad_loc(c, e.val), ec.real_grad_loc(c, np.broadcast_to(e.err, e.val.shape))) if "counts" in c else e


def _scatter(shape, idx4, terms, deriv):
    """grad_value: per pixel the sum of `terms` (Ev [4][B, Q, H, L, P, D], exact zeros where the corner is no pixel) at the
    pixel indices idx4, in any order — count, scan, place, windows, continuation rows, rounds and passes only regroup it
     — plus `deriv` (the coordinate / quantisation part, summed in absolute value over the hits)."""
    B, I, H, D = shape
    val, err, mag, cnt = (np.zeros(shape) for _ in range(4))
    bi, hi = np.arange(B).reshape(B, 1, 1, 1, 1), np.arange(H).reshape(1, 1, H, 1, 1)
    for k in range(4):
        ix = (np.broadcast_to(bi, idx4[k].shape), idx4[k], np.broadcast_to(hi, idx4[k].shape))
        live = terms[k].val != 0
        np.add.at(val, ix, terms[k].val)
        np.add.at(err, ix, terms[k].err + deriv[k])
        np.add.at(mag, ix, np.abs(terms[k].val))
        np.add.at(cnt, ix, live.astype(np.float64))
    Ev.check_terms(cnt)
    return Ev(val, err + np.maximum(cnt - 1, 0) * U * mag)


def plain_formulas(c, pm, ac, records="float", loc_err=None, attn_err=None):
    """out, grad_value, grad_loc, grad_attn of the plain operator as (val, err) per element, in the case's own layout.
    records: "float" — grad_value by the single-launch kernel, full float fractions; "q20" — by the sorted pipeline, whose
    records carry dx, dy in 20 fractional bits.  loc_err / attn_err (the case's layout): the errors the sampling points
    and attention weights arrive with when a fused prologue formed them; inputs read from memory have none."""
    d = ec.dense(c)
    zeros = pm == "zeros"
    n = _sizes(d)
    pix = ec.pixel_coordinates(c, ac)
    e_px = pixel_error(d, ac, None if loc_err is None else _dense_like(c, loc_err))
    a_err = 0.0 if attn_err is None else _dense_like(c, attn_err)
    idx, mask, _ = ec.taps(c, pm, ac)
    cell = np.floor(pix)
    frac = pix - cell
    # t.dx = px - x0 (msda_common.hpp:341-342): exact for px >= 0, a rounding for -1 < px < 0 — counted always
    e_x, e_y = e_px[..., 0] + U * frac[..., 0], e_px[..., 1] + U * frac[..., 1]
    dx, dy = Ev(frac[..., 0, None]), Ev(frac[..., 1, None])       # [..., 1]: broadcast over D
    wx0, wy0 = 1.0 - dx, 1.0 - dy                                 # msda_kernels.hpp:877, 1496
    a = Ev(d["attn"][..., None], a_err[..., None] if attn_err is not None else 0.0)
    v = [np.where(m[..., None], _gather(d, i), 0.0) for i, m in zip(idx, mask)]  # 00, 01, 10, 11; masked corners read zeros
    g = d["grad_out"][:, :, :, None, None, :]
    S, D = _real_terms(c), d["value"].shape[-1]
    # d out / d px and d out / d py per channel, without the attention weight
    GX = wy0.val * (v[1] - v[0]) + dy.val * (v[3] - v[2])
    GY = wx0.val * (v[2] - v[0]) + dx.val * (v[3] - v[1])

    # ---- out (msda_kernels.hpp:877-882: w_k = a * (wy * wx); 915-925 / msda_common.hpp:86-109: four chained FMAs per sample)
    wyx = [wy0 * wx0, wy0 * dx, dy * wx0, dy * dx]
    terms = stack([(a * w) * Ev(vk) for w, vk in zip(wyx, v)], 0)  # [4, B, Q, H, L, P, D]
    out = terms.sum((0, 4, 5), n=4 * S)
    out = Ev(out.val, out.err + (np.abs(d["attn"][..., None]) * (np.abs(GX) * e_x[..., None] + np.abs(GY) * e_y[..., None])).sum((3, 4)))

    # ---- grad_attn (msda_kernels.hpp:1494-1505: four dot products with grad_out, combined with the corner weights and
    # summed over the unit's lanes: 4 D products in all, in either body's order)
    gv = [Ev(g) * Ev(vk) for vk in v]                              # msda_kernels.hpp:1588-1593, 1702-1705 (FMA: counted as rounded)
    ga = stack([w * t for w, t in zip(wyx, gv)], 0).sum((0, -1), n=4 * D)
    ga = Ev(ga.val, ga.err + np.abs((g * GX).sum(-1)) * e_x + np.abs((g * GY).sum(-1)) * e_y)

    # ---- grad_loc (msda_kernels.hpp:1498-1499: gX = wy0 (d1 - d0) + dy (d3 - d2); 1453-1454: a * sx behind the gate;
    # 1506-1507: their product)
    gX = stack([wy0 * gv[1], -(wy0 * gv[0]), dy * gv[3], -(dy * gv[2])], 0).sum((0, -1), n=4 * D)
    gY = stack([wx0 * gv[2], -(wx0 * gv[0]), dx * gv[3], -(dx * gv[1])], 0).sum((0, -1), n=4 * D)
    cross = np.abs((g * (v[3] - v[2] - v[1] + v[0])).sum(-1))     # d gX / d py = d gY / d px
    gX = Ev(gX.val, gX.err + cross * e_y)
    gY = Ev(gY.val, gY.err + cross * e_x)
    scale = n - 1 if ac else n                                    # msda_kernels.hpp:1448-1449 (exact integers)
    alive = np.ones(pix.shape, bool) if zeros else (pix > 0) & (pix < n - 1)  # msda_common.hpp:338-339
    a1 = Ev(d["attn"], a_err)
    gl = stack([((a1 * scale[..., 0]) * gX).where(alive[..., 0]), ((a1 * scale[..., 1]) * gY).where(alive[..., 1])], -1)

    # ---- grad_value.  The cell passes clamp the coordinate FIRST under "border" (msda_value_sorted.hpp:142-148), so a
    # clamped sample has dx = 0 on the edge cell; "zeros" keeps the cells x0 = -1 .. W - 1 and drops the corners outside.
    if zeros:
        cpix = pix
        inside = np.ones(pix.shape, bool)
    else:
        cpix = np.clip(pix, 0, n - 1)
        inside = (pix > -KINK_MARGIN * e_px) & (pix < n - 1 + KINK_MARGIN * e_px)  # clamped: the coordinate error cannot move it
    c0 = np.floor(cpix)
    fr = cpix - c0
    qerr = 0.0
    if records == "q20":
        # round to nearest on 20 bits, capped at 0xFFFFF (msda_value_sorted.hpp:65-66): half a step, a whole one where the
        # fraction rounds up to 1; the product `dx * 2^20 + 0.5` itself is rounded in float (U relative to it)
        qerr = np.where(fr * 2.0 ** 20 + 0.5 >= 2.0 ** 20 - 1, 2 * QUANT20, QUANT20) + 2 * U * fr
    ex = np.where(inside[..., 0], e_px[..., 0], 0.0) + U * fr[..., 0] + (qerr[..., 0] if records == "q20" else 0.0)
    ey = np.where(inside[..., 1], e_px[..., 1], 0.0) + U * fr[..., 1] + (qerr[..., 1] if records == "q20" else 0.0)
    fx, fy = Ev(fr[..., 0, None]), Ev(fr[..., 1, None])
    if records == "q20":  # msda_value_sorted.hpp:647-652
        ax1 = a * fx
        ax0 = a - ax1
        w3, w2 = ax1 * fy, ax0 * fy
        w4 = [ax0 - w2, ax1 - w3, w2, w3]
    else:                 # msda_value_small.hpp:438-447: (a * wy) * wx
        ay0, ay1 = a * (1.0 - fy), a * fy
        w4 = [ay0 * (1.0 - fx), ay0 * fx, ay1 * (1.0 - fx), ay1 * fx]
    h_, w_ = d["shapes"][:, 0].reshape(1, 1, 1, -1, 1), d["shapes"][:, 1].reshape(1, 1, 1, -1, 1)
    start = (np.cumsum(d["shapes"][:, 0] * d["shapes"][:, 1]) - d["shapes"][:, 0] * d["shapes"][:, 1]).reshape(1, 1, 1, -1, 1)
    ag = np.abs(d["attn"][..., None] * g)
    dwx = [1 - fr[..., 1], 1 - fr[..., 1], fr[..., 1], fr[..., 1]]  # |d w_k / d dx| without a
    dwy = [1 - fr[..., 0], fr[..., 0], 1 - fr[..., 0], fr[..., 0]]
    idx4, terms4, deriv4 = [], [], []
    for k, (oy, ox) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        x, y = c0[..., 0] + ox, c0[..., 1] + oy
        ok = (x >= 0) & (x <= w_ - 1) & (y >= 0) & (y <= h_ - 1)    # msda_value_sorted.hpp:151-153: the corner is a pixel
        idx4.append(start + np.clip(y, 0, h_ - 1).astype(np.int64) * w_ + np.clip(x, 0, w_ - 1).astype(np.int64))
        terms4.append((w4[k] * Ev(g)).where(ok[..., None]))         # msda_value_sorted.hpp:20: one FMA per corner and channel
        deriv4.append(np.where(ok[..., None], ag * (dwx[k] * ex + dwy[k] * ey)[..., None], 0.0))
    gval = _scatter(d["value"].shape, idx4, terms4, deriv4)
    return dict(out=out, grad_value=gval, grad_loc=_unpad_ev(c, gl), grad_attn=_unpad_ev(c, ga))


def plain_keep(c, ac, loc_err=None):
    """Per tensor, which elements are compared (bool, broadcastable): everything of out, grad_value and grad_attn — they
    are continuous — and grad_loc away from the kinks."""
    k = ~kink_samples(c, ac, loc_err)
    k = ec.real_grad_loc(c, k) if "counts" in c else k
    return dict(out=True, grad_value=True, grad_attn=True, grad_loc=k[..., None])


@functools.lru_cache(maxsize=None)
def plain_reference(name, storage, pm, ac, records="float"):
    """(formulas, keep) of a fixture, cached: shared by every test that needs them, never modified."""
    c = get_case(name, storage)
    return plain_formulas(c, pm, ac, records), plain_keep(c, ac)


# ----------------------------------------------------------------------------------------- discrete sampling
def _discrete_axis(x, n, x_err=0.0):
    """t = x * n + 0.5 in fp64 and the error of its float evaluation: a rounded multiply followed by a rounded add, kept
    apart on purpose (msda_kernels.hpp:171-177); x_err: the error the point arrives with (a fused prologue formed it)."""
    t = x * n + 0.5
    return t, U * np.abs(x * n) + U * np.abs(t) + n * x_err


def discrete_formulas(c, loc_err=None, attn_err=None):
    """out, grad_value, grad_attn of discrete sampling as Ev, plus `near` — bool [B, Q, H, S], the samples whose pixel
    choice a float evaluation may make differently — and the candidate pixels of those samples."""
    B, I, H, D = c["value"].shape
    levels, counts = [tuple(s) for s in c["shapes"].tolist()], c["counts"]
    Q, S = c["loc"].shape[1], sum(counts)
    bi, hi = np.arange(B).reshape(B, 1, 1), np.arange(H).reshape(1, 1, H)
    pixel = np.zeros((B, Q, H, S), dtype=np.int64)
    near = np.zeros((B, Q, H, S), dtype=bool)
    cand = []
    start = s0 = 0
    for (h, w), npts in zip(levels, counts):
        for s in range(s0, s0 + npts):
            tx, ex = _discrete_axis(c["loc"][..., s, 0], w, 0.0 if loc_err is None else loc_err[..., s, 0])
            ty, ey = _discrete_axis(c["loc"][..., s, 1], h, 0.0 if loc_err is None else loc_err[..., s, 1])
            px = lambda t, n: np.clip(np.trunc(t), 0, n - 1).astype(np.int64)  # noqa: E731
            pixel[..., s] = start + px(ty, h) * w + px(tx, w)
            near[..., s] = (np.abs(tx - np.round(tx)) < KINK_MARGIN * ex) | (np.abs(ty - np.round(ty)) < KINK_MARGIN * ey)
            for sx in (-1, 1):
                for sy in (-1, 1):
                    cand.append((s, start + px(ty + sy * KINK_MARGIN * ey, h) * w + px(tx + sx * KINK_MARGIN * ex, w)))
        start += h * w
        s0 += npts
    rows = c["value"][bi[..., None], pixel, hi[..., None]]                    # [B, Q, H, S, D]
    a, g = Ev(c["attn"][..., None], 0.0 if attn_err is None else attn_err[..., None]), Ev(c["grad_out"][:, :, :, None, :])
    out = (a * Ev(rows)).sum(3, n=S)                                          # msda_discrete.hpp:79: one FMA per sample and channel
    ga = (g * Ev(rows)).sum(-1, n=D)                                          # msda_discrete.hpp:147-158
    t = a * g                                                                 # the record's weight times the grad_out row
    val, err, mag, cnt = (np.zeros((B, I, H, D)) for _ in range(4))
    ix = (np.broadcast_to(bi[..., None], pixel.shape), pixel, np.broadcast_to(hi[..., None], pixel.shape))
    np.add.at(val, ix, t.val)
    np.add.at(err, ix, t.err)
    np.add.at(mag, ix, np.abs(t.val))
    np.add.at(cnt, ix, 1.0)
    Ev.check_terms(cnt)
    gval = Ev(val, err + np.maximum(cnt - 1, 0) * U * mag)
    # what is left out: every tensor of a unit with a `near` sample, and the grad_value rows of its candidate pixels
    unit = near.any(-1)
    keep_gv = np.ones((B, I, H), dtype=bool)
    for s, pix in cand:
        hit = near[..., s]
        keep_gv[np.broadcast_to(bi, hit.shape)[hit], pix[hit], np.broadcast_to(hi, hit.shape)[hit]] = False
    keep = dict(out=~unit[..., None], grad_attn=~unit[..., None], grad_value=keep_gv[..., None])
    return dict(out=out, grad_value=gval, grad_attn=ga), keep, near


@functools.lru_cache(maxsize=None)
def discrete_reference(name, storage):
    return discrete_formulas(get_case(name, storage))


# ----------------------------------------------------------------------------------------- the comparison
def ratios(got, form, keep):
    """Per tensor: (elements beyond the bound, largest |got - val| / (err * (1 + 2^-10) + r)) over the kept elements; r is
    half the spacing of the type `got` came back in at |val| + err (0 for float32).  A bound of exactly 0 asks for
    equality (ratio 0 when met, inf when not)."""
    res = {}
    for k, e in form.items():
        t = got[k]
        dtype = t.dtype if isinstance(t, torch.Tensor) else F32
        x = t.double().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)
        assert x.shape == e.val.shape, (k, x.shape, e.val.shape)
        lim = bound(e) + half_spacing(np.abs(e.val) + e.err, dtype)
        diff = np.abs(x - e.val)
        diff = np.where(np.isnan(diff), np.inf, diff)
        kp = np.broadcast_to(keep[k], x.shape)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(diff <= lim, np.where(lim > 0, diff / lim, 0.0), np.where(lim > 0, diff / lim, np.inf))
        r = np.where(kp, r, 0.0)
        res[k] = (int((r > 1).sum()), float(r.max()) if r.size else 0.0)
    return res


def assert_within(got, form, keep, what):
    """Every kept element of every tensor within its bound; all tensors are compared before the assertion, so a failure
    names each one that is off (count, largest error / bound).  Prints the largest ratio per tensor."""
    res = ratios(got, form, keep)
    print(f"{what}: " + ", ".join(f"{k} {r:.3f}" for k, (_, r) in res.items()) + "  (largest error / bound)")
    wrong = {k: v for k, v in res.items() if v[0]}
    assert not wrong, (what, wrong)
    return res


# ----------------------------------------------------------------------------------------- the fused prologues
# exp: the device expf (msda_common.hpp:446, ::expf — the translation units are built without fast-math, Makefile).  HIP's
# math API documentation lists expf with a maximum error of 1 ulp; no copy of that table ships with this repository, so the
# figure used is the ASSUMED 2 ulp, as a relative error: 2 ulp <= 2 * 2^-23 = 4 U.
EXP_C = 4.0
FUSED_STORAGE = {"f32": (F32, F32), "f32_sbf16": (BF16, F32), "f32_sf16": (F16, F32)}  # (value / proj / grad_out, reference points)
HFBOX_SCALE = 0.3   # transformers' offset_scale; not a float32 number, so the kernel's (float)0.3 is part of the model
# name: (rule, ref_dim, P or counts)
FUSED = {
    "module2": ("module", 2, 2), "module4": ("module", 4, 2),
    "module2_c": ("module", 2, [3, 1, 2]), "module4_c": ("module", 4, [3, 1, 2]),
    "levelref2": ("levelref", 2, 2), "levelref4": ("levelref", 4, 2),
    "hfbox": ("hfbox", 4, [3, 1, 2]), "hfbox_discrete": ("hfbox", 4, [3, 1, 2]),
}
FUSED_DIMS = dict(B=2, Q=37, H=3, D=32)
# ... and the names a helper module registers (tests/sample_level_cases.py), in tables of their own so that what iterates
# FUSED sees the same names whatever was imported before: name -> FUSED's tuple, name -> (dims as FUSED_DIMS, levels)
FUSED_MORE = {}
FUSED_SHAPES = {}
FUSED_DISCRETE = {"hfbox_discrete"}  # the names whose operator behind the prologue is discrete sampling


def fused_entry(name):
    """(rule, ref_dim, P or counts) of a name of FUSED or FUSED_MORE"""
    return FUSED[name] if name in FUSED else FUSED_MORE[name]


def ev_exp(z):
    v = np.exp(z.val)
    return Ev(v, v * (z.err + EXP_C * U))


def ev_scaled(e, c):
    """e * c for a power of two c: exact."""
    return Ev(e.val * c, e.err * abs(c))


def ev_reshape(e, shape):
    return Ev(e.val.reshape(shape), np.broadcast_to(e.err, e.val.shape).reshape(shape))


def _sample_levels(proj, counts):
    """(level, point count of the level) per sample, broadcastable over proj[..., 0]; the sample axes; S."""
    if counts is None:
        L, P = proj.shape[3:5]
        lvl = np.arange(L).reshape(1, 1, 1, L, 1)
        return lvl, np.full(lvl.shape, P), (3, 4), L * P
    lvl = np.repeat(np.arange(len(counts)), counts).reshape(1, 1, 1, -1)
    return lvl, np.repeat(counts, counts).reshape(lvl.shape), (3,), sum(counts)


@functools.lru_cache(maxsize=None)
def fused_raw_case(name):
    rule, ref_dim, P = fused_entry(name)
    rng = np.random.default_rng(zlib.crc32(("error_bound_fused_" + name).encode()) + SEEDS.get(name, 0))
    dims, levels = FUSED_SHAPES.get(name, (FUSED_DIMS, LEVELS))
    B, Q, H, D = (dims[k] for k in "BQHD")
    counts = None if isinstance(P, int) else list(P)
    shapes = np.asarray(levels, dtype=np.int64)
    pts = (len(levels), P) if counts is None else (sum(counts),)
    lvl, npts, _, _ = _sample_levels(np.zeros((B, Q, H) + pts + (3,)), counts)
    ref_shape = (B, Q, len(levels), ref_dim) if rule == "levelref" else (B, Q, ref_dim)
    ref = rng.uniform(0.1, 0.9, size=ref_shape)
    if ref_dim == 4:
        ref[..., 2:] = rng.uniform(0.2, 0.6, size=ref_shape[:-1] + (2,))
    r = ref[:, :, None, :, None, :] if rule == "levelref" else ref.reshape((B, Q, 1) + (1,) * len(pts) + (ref_dim,))
    move = rng.uniform(-0.25, 0.25, size=(B, Q, H) + pts + (2,))  # where the offset takes the point: [-0.15, 1.15] in all
    hs, ws = shapes[lvl, 0].astype(np.float64), shapes[lvl, 1].astype(np.float64)
    if ref_dim == 2:
        div = np.stack([ws, hs], -1) if rule == "levelref" else np.stack([hs, ws], -1)
        off = move * div
    elif rule == "hfbox":
        off = move / (r[..., 2:] * HFBOX_SCALE) * npts[..., None]
    elif rule == "levelref":
        off = move / (r[..., 2:] * 0.5) * npts[..., None]
    else:
        off = move / r[..., 2:] * (2 * npts[..., None])
    logit = rng.uniform(-4.0, 4.0, size=(B, Q, H) + pts)        # |z - max| <= 8
    c = dict(value=rng.standard_normal((B, int((shapes[:, 0] * shapes[:, 1]).sum()), H, D)), shapes=shapes,
             proj=np.concatenate([off, logit[..., None]], -1), ref=ref, grad_out=rng.standard_normal((B, Q, H, D)))
    if counts is not None:
        c["counts"] = counts
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def fused_case(name, storage="f32"):
    sdt, rdt = FUSED_STORAGE[storage]
    c = dict(fused_raw_case(name))
    for k in ("value", "proj", "grad_out"):
        c[k] = _through(c[k], sdt)
    c["ref"] = _through(c["ref"], rdt)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def softmax_ev(z, exp_fn=ev_exp, shift=True):
    """exp(z - max) * (1 / sum exp(z - max)) over the last axis (msda_kernels.hpp:813-821 and 841, 1390-1398 and 1421;
    msda_hfbox_discrete.hpp:30-45): the max is exact, the subtraction, every exp, the sum of S terms, the reciprocal and the
    product round."""
    mx = z.max(-1, keepdims=True) if shift else 0.0
    e = exp_fn(Ev(z) - mx)
    inv = Ev(1.0) / e.sum(-1)
    return e * inv[..., None]


def prologue(fc, name, scale_fn=None):
    """The sampling points (x, y), the attention weights, d point / d offset (kx, ky), the parked offsets the box-size
    gradient multiplies and the factor applied behind its sum — each an Ev in the layout of proj[..., 0].  scale_fn: a
    mutant's rounding of the box rule's float32(1 / P_l)."""
    rule, ref_dim, _ = fused_entry(name)
    proj, counts = fc["proj"], fc.get("counts")
    lvl, npts, _, S = _sample_levels(proj, counts)
    hs, ws = fc["shapes"][lvl, 0].astype(np.float64), fc["shapes"][lvl, 1].astype(np.float64)
    ox, oy, z = Ev(proj[..., 0]), Ev(proj[..., 1]), proj[..., 2]
    a = ev_reshape(softmax_ev(z.reshape(z.shape[:3] + (S,))), z.shape)
    ref = fc["ref"]
    r = ref[:, :, None, :, None, :] if rule == "levelref" else ref.reshape(ref.shape[:2] + (1,) * (proj.ndim - 3) + (ref_dim,))
    rx, ry = r[..., 0], r[..., 1]
    oq = post = None
    if ref_dim == 2:
        # module: (x, y) offsets over img_shapes in its stored (h, w) order (msda_kernels.hpp:795-796, 1366-1367; d point /
        # d offset 1847-1848); transformers: over (w, h) (787-788, 1355-1358; 1840-1841).  One division, one addition.
        dx_, dy_ = (ws, hs) if rule == "levelref" else (hs, ws)
        x, y = Ev(rx) + ox / dx_, Ev(ry) + oy / dy_
        kx, ky = Ev(1.0) / dx_, Ev(1.0) / dy_
    else:
        rw, rh = r[..., 2], r[..., 3]
        if rule == "module":
            # ref + o * size / (2 P_l) (msda_kernels.hpp:801-805) in the forward, ref + o * size * (1 / (2 P_l)) in the
            # backward and for grad_value's parked points (1373-1380, 1885-1889): product, ROUNDED reciprocal, product, sum
            # bounds both
            hip = Ev(1.0) / (2.0 * npts)
            x, y = Ev(rx) + (ox * rw) * hip, Ev(ry) + (oy * rh) * hip
            kx, ky = Ev(rw) * hip, Ev(rh) * hip                                   # 1851-1855
            if counts is None:
                oq, post = (ox, oy), hip                                          # 1784-1785 on raw offsets, 1806-1807
            else:
                oq, post = (ox * hip, oy * hip), None                             # 1375-1377: parked scaled
        elif rule == "levelref":
            # levelref_box_point (msda_kernels.hpp:266-272): q = o / P, t = q * size, t * 0.5 (exact), ref + t
            qx, qy = ox / npts, oy / npts                                         # 790-791, 1360-1361
            x, y = Ev(rx) + ev_scaled(qx * rw, 0.5), Ev(ry) + ev_scaled(qy * rh, 0.5)
            hip = Ev(1.0) / (2.0 * npts)                                          # 1185
            kx, ky = Ev(rw) * hip, Ev(rh) * hip                                   # 1843-1844
            oq, post = (qx, qy), 0.5                                              # 1763-1764, 1770-1771
        else:
            # hfbox_point (msda_kernels.hpp:318-324): q = o * s_l, t = q * size, t * offset_scale, ref + t; s_l is the
            # host's float32(1 / P_l) (functional.hf_box_level_scale), offset_scale converted to float (782)
            s = np.float32(1.0) / npts.astype(np.float32)
            s = (s if scale_fn is None else scale_fn(s)).astype(np.float64)
            os_ = Ev(HFBOX_SCALE, abs(HFBOX_SCALE - float(np.float32(HFBOX_SCALE))))
            qx, qy = ox * s, oy * s                                               # 1345-1346
            x, y = Ev(rx) + (qx * rw) * os_, Ev(ry) + (qy * rh) * os_
            kx, ky = (Ev(s) * rw) * os_, (Ev(s) * rh) * os_                       # 1836-1837
            oq, post = (qx, qy), os_                                              # 1784-1785, 1802-1803
    return dict(x=x, y=y, a=a, kx=kx, ky=ky, oq=oq, post=post)


def fused_operator_case(fc, pro):
    """The plain operator's case behind the prologue: its points and weights as fp64 values."""
    c = dict(value=fc["value"], shapes=fc["shapes"], loc=np.stack([pro["x"].val, pro["y"].val], -1), attn=pro["a"].val,
             grad_out=fc["grad_out"])
    if "counts" in fc:
        c["counts"], c["bits"] = fc["counts"], dict(loc=5)
    return c


def fused_formulas(fc, name, pm, ac, records="float", pro=None):
    """out, grad_value, grad_proj and grad_ref of a fused family as Ev, and what to keep of them."""
    rule, ref_dim, _ = fused_entry(name)
    pro = prologue(fc, name) if pro is None else pro
    c = fused_operator_case(fc, pro)
    loc_err = np.stack([pro["x"].err, pro["y"].err], -1)
    _, _, saxes, S = _sample_levels(fc["proj"], fc.get("counts"))
    H = fc["value"].shape[2]
    a = pro["a"]
    if name in FUSED_DISCRETE:
        base, keep0, near = discrete_formulas(c, loc_err, a.err)
        gA = base["grad_attn"]
        dot = (a * gA).sum(3, n=S)                                                # msda_hfbox_discrete.hpp:251-255
        g2 = a * (gA - dot[..., None])                                            # msda_hfbox_discrete.hpp:260
        zero = Ev(np.zeros(g2.val.shape))
        form = dict(out=base["out"], grad_value=base["grad_value"], grad_proj=stack([zero, zero, g2], -1))
        return form, dict(out=keep0["out"], grad_value=keep0["grad_value"], grad_proj=keep0["grad_attn"][..., None]), near
    base = plain_formulas(c, pm, ac, records, loc_err=loc_err, attn_err=a.err)
    gl, gA = base["grad_loc"], base["grad_attn"]
    glx, gly = gl[..., 0], gl[..., 1]
    dot = (a * gA).sum(saxes, n=S)                                                # msda_kernels.hpp:1752 / 1781, 1787
    dot = dot[(Ellipsis,) + (None,) * len(saxes)]
    gp = stack([glx * pro["kx"], gly * pro["ky"], a * (gA - dot)], -1)            # msda_kernels.hpp:1895-1897
    # the reference point's gradient: per-head partial sums over the unit's samples (1782-1789; per level 1756-1765), which
    # the caller sums over the heads — H * S (H * P) terms in any order
    raxes, n = ((2, 4), H * fc["proj"].shape[4]) if rule == "levelref" else ((2,) + saxes, H * S)
    parts = [glx.sum(raxes, n=n), gly.sum(raxes, n=n)]
    if ref_dim == 4:
        for g_, o_ in zip((glx, gly), pro["oq"]):
            t = (g_ * o_).sum(raxes, n=n)
            post = pro["post"]
            parts.append(t if post is None else ev_scaled(t, post) if isinstance(post, float) else t * _squeeze(post, raxes))
    kink = kink_samples(c, ac, loc_err)
    kink = ec.real_grad_loc(c, kink) if "counts" in c else kink
    keep = dict(out=True, grad_value=True, grad_proj=np.stack([~kink, ~kink, np.ones_like(kink)], -1),
                grad_ref=~kink.any(raxes)[..., None])
    return dict(out=base["out"], grad_value=base["grad_value"], grad_proj=gp, grad_ref=stack(parts, -1)), keep, kink


def _squeeze(e, axes):
    """A factor that is constant along `axes` (size-1 or broadcast there), without them."""
    v, r = np.asarray(e.val), np.broadcast_to(e.err, np.shape(e.val))
    if v.ndim == 0:
        return e
    ix = tuple(0 if a in axes else slice(None) for a in range(v.ndim))
    return Ev(v[ix], r[ix])


@functools.lru_cache(maxsize=None)
def fused_reference(name, storage, pm, ac, records="float"):
    return fused_formulas(fused_case(name, storage), name, pm, ac, records)


def fused_torch(fc, name, pm, ac, dtype):
    """The composition in plain PyTorch on the host, in `dtype`, with autograd: the package's prologue functions in front
    of the host operator (as tests/test_gpu_hf_box_fused.py and tests/test_gpu_hf_box_discrete.py build their references)."""
    from msda_triton_amd import functional as F, ragged
    from msda_triton_amd.functional import multiscale_deformable_attention
    rule, _, _ = fused_entry(name)
    t = {k: torch.from_numpy(np.array(fc[k])).to(dtype).requires_grad_(True) for k in ("value", "proj", "ref")}
    shapes, counts = torch.from_numpy(np.array(fc["shapes"])), fc.get("counts")
    if rule == "hfbox":
        pts, att = F.hf_box_sampling_inputs(t["proj"], t["ref"], counts, HFBOX_SCALE)
    elif rule == "levelref":
        pts, att = F.hf_module_sampling_inputs(t["proj"], shapes, t["ref"])
    elif counts is not None:
        pts, att = ragged.ragged_module_sampling_inputs(t["proj"], shapes, t["ref"], counts)
    else:
        pts, att = F.module_sampling_inputs(t["proj"], shapes, t["ref"])
    kw = dict(points_per_level=counts) if counts is not None else {}
    if name in FUSED_DISCRETE:
        out = multiscale_deformable_attention(t["value"], shapes, pts, att, "border", False, sampling_mode="discrete", **kw)
    else:
        out = multiscale_deformable_attention(t["value"], shapes, pts, att, pm, ac, **kw)
    out.backward(torch.from_numpy(np.array(fc["grad_out"])).to(dtype))
    res = dict(out=out.detach(), grad_value=t["value"].grad, grad_proj=t["proj"].grad)
    if name not in FUSED_DISCRETE:
        res["grad_ref"] = t["ref"].grad
    return res


# ----------------------------------------------------------------------------------------- emulated wrong kernels (CPU, fp64)
def emulated_grad_value(c, pm, ac, frac_fn=None):
    """grad_value in numpy fp64 by the cell passes' formulation (clamp first under "border", msda_value_sorted.hpp:137-148);
    frac_fn: applied to the cell fractions (dx, dy) — a mutant's record format."""
    d = ec.dense(c)
    n = _sizes(d)
    pix = ec.pixel_coordinates(c, ac)
    cpix = pix if pm == "zeros" else np.clip(pix, 0, n - 1)
    c0 = np.floor(cpix)
    fr = cpix - c0
    fr = fr if frac_fn is None else frac_fn(fr)
    h_, w_ = d["shapes"][:, 0].reshape(1, 1, 1, -1, 1), d["shapes"][:, 1].reshape(1, 1, 1, -1, 1)
    start = (np.cumsum(d["shapes"][:, 0] * d["shapes"][:, 1]) - d["shapes"][:, 0] * d["shapes"][:, 1]).reshape(1, 1, 1, -1, 1)
    B, I, H, D = d["value"].shape
    bi, hi = np.arange(B).reshape(B, 1, 1, 1, 1), np.arange(H).reshape(1, 1, H, 1, 1)
    ag = d["attn"][..., None] * d["grad_out"][:, :, :, None, None, :]
    out = np.zeros((B, I, H, D))
    for oy, ox in ((0, 0), (0, 1), (1, 0), (1, 1)):
        x, y = c0[..., 0] + ox, c0[..., 1] + oy
        ok = (x >= 0) & (x <= w_ - 1) & (y >= 0) & (y <= h_ - 1)
        idx = start + np.clip(y, 0, h_ - 1).astype(np.int64) * w_ + np.clip(x, 0, w_ - 1).astype(np.int64)
        wgt = (fr[..., 1] if oy else 1 - fr[..., 1]) * (fr[..., 0] if ox else 1 - fr[..., 0])
        np.add.at(out, (np.broadcast_to(bi, idx.shape), idx, np.broadcast_to(hi, idx.shape)), np.where(ok, wgt, 0.0)[..., None] * ag)
    return out


def quantised(bits):
    """Fractions rounded to nearest on `bits` fractional bits, capped below 1, as Entry<float>::pack does with 20."""
    return lambda fr: np.minimum(np.floor(fr * 2.0 ** bits + 0.5), 2.0 ** bits - 1) / 2.0 ** bits


def rounded_to(dtype):
    return lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype).double().numpy()


def out_from_taps(c, pm, ac, pix):
    """`out` in fp64 from a mutant's pixel coordinates (cell and fractions taken from them)."""
    d = ec.dense(c)
    idx, mask, wgt = ec.taps(c, pm, ac, pix=pix, cell=np.floor(pix))
    total = 0.0
    for k in range(4):
        total = total + np.where(mask[k], wgt[k], 0.0)[..., None] * _gather(d, idx[k])
    return (d["attn"][..., None] * total).sum((3, 4))
