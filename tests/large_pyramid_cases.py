"""Exact fixtures on pyramids LARGER than the sorted grad_value pipeline's LDS tables ("Larger than the
tables"): a plane with more cells than the count pass holds (kCellLdsInts) is walked in several trips, a level with more
cells than the level-major place pass holds (kPlaceCellsTwoPerCu) too.  A helper module, not a conftest; the cases are
registered in `exact_cases.CASES`, so `ec.get_case`, `ec.checked_reference` and `ec.precondition` (budget <= 24 bits,
float32 oracle == float64 oracle, no sample on the pixel lattice) apply to them as to every other exact case.

Sampling points.  The cases are run in bf16 storage as well, and an odd multiple k / 2^9 with k > 256 is no bf16 number
(nine significant bits), so the points are drawn from the multiples of 2^-9 in [lo, hi] that HAVE at most eight
significant bits and sit on no integer pixel coordinate of their level's axis under either align_corners — still closer
together than one pixel of a 200-wide axis, so every cell that a bf16 coordinate can reach can be aimed at, and the bit
budget (fractional bits of a multiple of 2^-9) is that of `loc_bits=9`.  `precondition` below adds the check that every
input survives bf16.

Cuts.  `cuts(levels, cell_cap, place_cells)`: the plane-relative cell ids at which a count trip starts (k * cell_cap) and
at which a place trip starts (cstart_l + k * place_cells).  The hook registered in `ec.FINISH` overwrites a few samples so that, in every mode, a
sample of weight 1 with a grad_out row that is not zero sits in the last cell before and in the first cell after every
cut (where that cell cannot hold a sample in the mode — x0 = -1 under "border", a last column that no bf16 coordinate
reaches under "zeros" — in the nearest cell on that side that can).

Emulated wrong pipelines.  `gather_grad_value(c, pm, ac, mult)`: grad_value as a gather over samples in numpy fp64 with
a per-sample multiplicity; `MUTANTS` are the multiplicities of pipelines that cut a trip one cell off, leave a level
out of a later trip or re-base a ragged trip's slots by the wrong level."""
import functools
import os
import re

import numpy as np
import torch

import exact_cases as ec
from exact_cases import BF16, F32, MODES

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "msda_triton_amd", "csrc")
LOC_BITS = 9
LO, HI = -0.02, 1.02


@functools.lru_cache(maxsize=None)
def pipeline_constants():
    """the `constexpr int k... = N;` table sizes of the kernels' sources (as query_mask_cases.pipeline_constants reads them)"""
    text = "".join(open(os.path.join(_CSRC, f)).read() for f in ("msda_value_sorted.hpp", "msda_value_place.hpp"))
    found = {k: int(v) for k, v in re.findall(r"constexpr int (k[A-Za-z]+) = (\d+);", text)}
    return {k: found[k] for k in ("kCellLdsInts", "kPlaceCellsTwoPerCu", "kScanCells", "kCellBlock", "kPlaceBlock",
                                  "kPlaceBlockSmall")}


def table_sizes():
    """(cells of the count table, cells of the level-major place table) as the launcher sizes them for these planes: the
    count table is kCellLdsInts rounded down to whole scan blocks, the place table kPlaceCellsTwoPerCu"""
    k = pipeline_constants()
    return k["kCellLdsInts"] // k["kScanCells"] * k["kScanCells"], k["kPlaceCellsTwoPerCu"]


# ----------------------------------------------------------------------------------------- the cases
PYR = [(150, 160), (120, 130), (24, 20), (12, 10)]
_KW = dict(loc_bits=LOC_BITS, attn_bits=1, vmax=1, gmax=1, lo=LO, hi=HI)
_KW_D = dict(loc_bits=LOC_BITS, attn_bits=5, value_bits=3, grad_bits=3, lo=LO, hi=HI)
# name: (kind, (B, Q, H, D, levels, P), generator keywords, the modes the case is run in, count trips it is for)
BIG = {
    "big_u": ("bilinear", (2, 1200, 2, 8, PYR, 4), _KW, MODES, 2),
    "big_c": ("bilinear", (1, 1200, 2, 8, PYR, [5, 6, 3, 2]), _KW, MODES, 2),
    "big_d": ("discrete", (1, 1200, 2, 8, PYR, [5, 6, 3, 2]), _KW_D, [("border", False)], 2),
    "big_aligned": ("bilinear", (1, 1200, 2, 8, [(191, 191), (60, 64), (20, 24)], 4), _KW, MODES, 2),
    "big_three": ("bilinear", (1, 1500, 2, 8, [(200, 200), (180, 190)], 6), _KW, MODES, 3),
    "big_wide": ("bilinear", (1, 16, 2, 8, [(150, 160), (120, 130)], 600), dict(_KW, loc_bits=7, attn_bits=0), MODES, 2),
}
NAMES = list(BIG)
RUNS = [(n, pm, ac) for n in NAMES for pm, ac in BIG[n][3]]
RUN_IDS = [f"{n}-{pm}_{int(ac)}" for n, pm, ac in RUNS]


def levels_of(name):
    return [tuple(x) for x in BIG[name][1][4]]


def is_discrete(name):
    return BIG[name][0] == "discrete"


def cell_starts(levels):
    """cstart_l of every level and the plane's cell count: the exclusive cumsum of (h + 1) * (w + 1)"""
    n = [(h + 1) * (w + 1) for h, w in levels]
    return [int(x) for x in np.cumsum([0] + n[:-1])], int(sum(n))


def cuts(levels, cell_cap, place_cells):
    """-> (count cuts, place cuts): the plane-relative cell ids at which a count trip (k * cell_cap, k >= 1) and a place
    trip (cstart_l + k * place_cells, k >= 1) start"""
    cs, total = cell_starts(levels)
    count = list(range(cell_cap, total, cell_cap))
    place = [cs[l] + k for l, (h, w) in enumerate(levels) for k in range(place_cells, (h + 1) * (w + 1), place_cells)]
    return count, place


def trips(levels, cell_cap, place_cells):
    """-> (count trips of the plane, place trips per level)"""
    cs, total = cell_starts(levels)
    return -(-total // cell_cap), [-(-(h + 1) * (w + 1) // place_cells) for h, w in levels]


def level_of_cell(levels, cell):
    cs, total = cell_starts(levels)
    assert 0 <= cell < total, cell
    return max(l for l in range(len(levels)) if cs[l] <= cell)


# ----------------------------------------------------------------------------------------- sample -> cell
def axis_cell(x, n, pm, ac, discrete=False):
    """x0 (the cell's corner 00 on an axis of n pixels) of sampling coordinates x, fp64; np.nan where "zeros" drops it"""
    x = np.asarray(x, dtype=np.float64)
    if discrete:
        return np.clip(np.trunc(x * n + 0.5), 0, n - 1)
    px = x * (n - 1) if ac else x * n - 0.5
    if pm == "border":
        return np.floor(np.clip(px, 0, n - 1))
    x0 = np.floor(px)
    return np.where((x0 >= -1) & (x0 <= n - 1), x0, np.nan)


def sample_cells(c, pm, ac, discrete=False):
    """The plane-relative cell id of every sample of the (dense) case, int64 [B, Q, H, L, P]; -1: the sample touches no
    pixel ("zeros": no corner inside).  cell = cstart_l + (y0 + 1) * (w + 1) + (x0 + 1), x0 = floor(px) after the clamp
    under "border" (msda_value_sorted.hpp); discrete: the cell whose corner 00 is the sample's one pixel."""
    d = ec.dense(c)
    levels = [tuple(s) for s in d["shapes"].tolist()]
    cs, _ = cell_starts(levels)
    if not discrete:  # the oracle's own pixel coordinates
        pix = ec.pixel_coordinates(c, ac)
    out = np.empty(d["loc"].shape[:-1], dtype=np.int64)
    for l, (h, w) in enumerate(levels):
        if discrete:
            x0, y0 = axis_cell(d["loc"][:, :, :, l, :, 0], w, pm, ac, True), axis_cell(d["loc"][:, :, :, l, :, 1], h, pm, ac, True)
        else:
            px, py = pix[:, :, :, l, :, 0], pix[:, :, :, l, :, 1]
            if pm == "border":
                x0, y0 = np.floor(np.clip(px, 0, w - 1)), np.floor(np.clip(py, 0, h - 1))
            else:
                x0, y0 = np.floor(px), np.floor(py)
                gone = ~((x0 >= -1) & (x0 <= w - 1) & (y0 >= -1) & (y0 <= h - 1))
                x0, y0 = np.where(gone, np.nan, x0), np.where(gone, np.nan, y0)
        cell = cs[l] + (y0 + 1) * (w + 1) + (x0 + 1)
        out[:, :, :, l] = np.where(np.isnan(cell), -1, cell).astype(np.int64)
    return out


def real_mask(c):
    """bool [B, Q, H, L, P] of the dense layout: the samples the case really has (a ragged case's padding is False)"""
    d = ec.dense(c)
    m = np.zeros(d["attn"].shape, dtype=bool)
    counts = c.get("counts") or [d["attn"].shape[4]] * d["attn"].shape[3]
    for l, p in enumerate(counts):
        m[:, :, :, l, :p] = True
    return m


# ----------------------------------------------------------------------------------------- the sampling points
@functools.lru_cache(maxsize=None)
def coordinates(n, bits=LOC_BITS):
    """The multiples of 2^-bits in [LO, HI] that are bf16 numbers and sit on no integer pixel coordinate of an axis of n
    pixels under either align_corners, ascending (fp64)."""
    k = np.arange(int(np.ceil(LO * 2 ** bits)), int(np.floor(HI * 2 ** bits)) + 1)
    x = k / 2.0 ** bits
    t = torch.from_numpy(x)
    ok = (t.to(BF16).double() == t).numpy().copy()
    for px in (x * (n - 1), x * n - 0.5):
        ok &= px != np.round(px)
    return x[ok]


def _axis_table(n, pm, ac, discrete, bits):
    """{x0: a coordinate that lands there} on an axis of n pixels in the mode (the middle one of those that do)"""
    xs = coordinates(n, bits)
    x0 = axis_cell(xs, n, pm, ac, discrete)
    table = {}
    for v in np.unique(x0[~np.isnan(x0)]):
        hits = xs[x0 == v]
        table[int(v)] = float(hits[len(hits) // 2])
    return table


def holdable_cell(levels, cell, side, pm, ac, discrete=False, bits=LOC_BITS):
    """The cell nearest to `cell` on its `side` of a cut ("before": at or below, "after": at or above) and inside its
    level that a sample can sit in under the mode, with the sampling point that puts it there: -> (cell, level, x, y)."""
    cs, _ = cell_starts(levels)
    l = level_of_cell(levels, cell)
    h, w = levels[l]
    tx, ty = _axis_table(w, pm, ac, discrete, bits), _axis_table(h, pm, ac, discrete, bits)
    step = -1 if side == "before" else 1
    rel = cell - cs[l]
    while 0 <= rel < (h + 1) * (w + 1):
        y0, x0 = rel // (w + 1) - 1, rel % (w + 1) - 1
        if x0 in tx and y0 in ty:
            return cs[l] + rel, l, tx[x0], ty[y0]
        rel += step
    raise AssertionError(f"no cell {side} {cell} of level {l} can hold a sample under {pm} {ac}")


def planted_targets(name, pm, ac):
    """[(cut, side, cell, level, x, y)] for every count and place cut of the case in the mode"""
    levels = levels_of(name)
    count, place = cuts(levels, *table_sizes())
    bits = BIG[name][2]["loc_bits"]
    out = []
    for cut in sorted(set(count + place)):
        for side, cell in (("before", cut - 1), ("after", cut)):
            out.append((cut, side) + holdable_cell(levels, cell, side, pm, ac, is_discrete(name), bits))
    return out


def _finish(name):
    def finish(c, rng):
        """re-draws the sampling points from `coordinates` and plants the samples at the cuts"""
        levels = levels_of(name)
        bits = c["bits"]["loc"]
        counts = c.get("counts")
        loc, attn, gout = c["loc"], c["attn"], c["grad_out"]
        B, Q, H = loc.shape[:3]
        s0 = 0
        for l, (h, w) in enumerate(levels):
            p = counts[l] if counts else loc.shape[4]
            for axis, n in ((0, w), (1, h)):
                xs = coordinates(n, bits)
                # (uniform over the axis, not over the numbers: bf16's grid is twice as wide from 0.5 on, four times from 1)
                gap = np.where(np.abs(xs) < 0.5, 1.0, np.where(np.abs(xs) < 1.0, 2.0, 4.0))
                draw = rng.choice(xs, size=(B, Q, H, p), p=gap / gap.sum())
                if counts:
                    loc[:, :, :, s0:s0 + p, axis] = draw
                else:
                    loc[:, :, :, l, :, axis] = draw
            s0 += p
        units, i = B * Q * H, 0
        starts = np.cumsum([0] + list(counts or []))
        for pm, ac in BIG[name][3]:
            for _, _, _, l, x, y in planted_targets(name, pm, ac):
                u, pt = (i * 37 + 5) % units, i // units  # (37 is coprime to every case's unit count)
                b, q, hd = u // (Q * H), u // H % Q, u % H
                if counts:
                    assert pt == 0
                    loc[b, q, hd, starts[l]] = (x, y)
                    attn[b, q, hd, starts[l]] = 1.0
                else:
                    loc[b, q, hd, l, pt] = (x, y)
                    attn[b, q, hd, l, pt] = 1.0
                if not gout[b, q, hd].any():
                    gout[b, q, hd, 0] = 1.0
                i += 1
        return c
    return finish


for _n, (_kind, _dims, _kw, _modes, _) in BIG.items():
    ec.CASES[_n] = (_kind, _dims, {k: v for k, v in _kw.items()}, (BF16,))
    ec.FINISH[_n] = _finish(_n)


def precondition(name, pm, ac):
    """`ec.precondition` (budget <= 24 bits, float32 oracle == float64 oracle, no sample on the lattice — asserted there,
    unchanged) and: every input is a bf16 number, so the case is the same case in every storage type.  -> the budget."""
    assert (pm, ac) in BIG[name][3], (name, pm, ac)
    c = ec.get_case(name)
    for k in ("value", "loc", "attn", "grad_out"):
        t = torch.from_numpy(np.array(c[k]))
        assert torch.equal(t.to(BF16).double(), t) and torch.equal(t.to(F32).double(), t), f"{name}: {k} does not survive bf16"
    return ec.precondition(name, pm, ac)


def checked_reference(name, pm="border", ac=False):
    precondition(name, pm, ac)
    return ec.reference(name, pm, ac)


# ----------------------------------------------------------------------------------------- grad_value as a gather
def gather_grad_value(c, pm, ac, mult=None, discrete=False):
    """grad_value of the case in numpy fp64, sample by sample: every corner's pixel row receives
    mult * attn * corner weight * grad_out row.  mult [B, Q, H, L, P] (dense layout): how often the pipeline under test
    delivers the sample — 1 everywhere is the operator."""
    d = ec.dense(c)
    B, I, H, D = d["value"].shape  # noqa: E741
    real = real_mask(c)
    m = np.ones(real.shape) if mult is None else np.asarray(mult, dtype=np.float64)
    a = np.where(real, d["attn"], 0.0) * m
    if discrete:
        levels = [tuple(s) for s in d["shapes"].tolist()]
        start = np.cumsum([0] + [h * w for h, w in levels[:-1]])
        idx = np.empty(real.shape, dtype=np.int64)
        for l, (h, w) in enumerate(levels):
            ix = axis_cell(d["loc"][:, :, :, l, :, 0], w, pm, ac, True)
            iy = axis_cell(d["loc"][:, :, :, l, :, 1], h, pm, ac, True)
            idx[:, :, :, l] = (start[l] + iy * w + ix).astype(np.int64)
        taps = [(idx, np.ones(real.shape, bool), np.ones(real.shape))]
    else:
        taps = list(zip(*ec.taps(c, pm, ac)))
    gv = np.zeros((B, I, H, D))
    bi = np.broadcast_to(np.arange(B).reshape(B, 1, 1, 1, 1), real.shape)
    hi = np.broadcast_to(np.arange(H).reshape(1, 1, H, 1, 1), real.shape)
    g = np.broadcast_to(d["grad_out"][:, :, :, None, None, :], real.shape + (D,))
    for idx, mask, wgt in taps:
        wk = np.where(mask, wgt, 0.0) * a
        np.add.at(gv, (bi, idx, hi), wk[..., None] * g)
    return gv


# ----------------------------------------------------------------------------------------- emulated wrong pipelines
MUTANTS = ("first_cell_after_a_cut_dropped", "first_cell_after_a_cut_twice", "last_cell_before_a_cut_dropped",
           "straddling_level_loses_its_later_trip", "levels_after_the_straddling_one_skipped", "ragged_slot_base_off_by_a_level")


def mutants_of(name):
    """the mutants that can show on the case: a straddled level needs a count cut inside a level, the slot base per-level
    counts (the issue names big_c) — the aligned cut has none of either, and its later trip's FIRST level is all it walks
    under mutant 5"""
    levels = levels_of(name)
    cs, _ = cell_starts(levels)
    count, _ = cuts(levels, *table_sizes())
    out = list(MUTANTS[:3])
    if any(c not in cs for c in count):
        out.append(MUTANTS[3])
    if any(level_of_cell(levels, c) < len(levels) - 1 for c in count):
        out.append(MUTANTS[4])
    if name == "big_c":
        out.append(MUTANTS[5])
    return out


def multiplicity(name, pm, ac, mutant):
    """-> mult [B, Q, H, L, P] of the emulated wrong pipeline on the case in the mode"""
    c = ec.get_case(name)
    levels = levels_of(name)
    cs, total = cell_starts(levels)
    cell_cap, place_cells = table_sizes()
    count, _ = cuts(levels, cell_cap, place_cells)
    cells = sample_cells(c, pm, ac, is_discrete(name))
    lvl = np.broadcast_to(np.arange(len(levels)).reshape(1, 1, 1, -1, 1), cells.shape)
    mult = np.ones(cells.shape)
    targets = planted_targets(name, pm, ac)
    if mutant in MUTANTS[:3]:
        side = "before" if mutant == MUTANTS[2] else "after"
        hit = np.isin(cells, [t[2] for t in targets if t[1] == side])
        mult[hit] = 2.0 if mutant == MUTANTS[1] else 0.0
    elif mutant == MUTANTS[3]:
        for cut in count:
            l = level_of_cell(levels, cut)
            if cs[l] != cut:
                mult[(lvl == l) & (cells >= cut)] = 0.0
    elif mutant == MUTANTS[4]:  # a later trip walks only the level that holds its first cell
        for cut in count:
            l = level_of_cell(levels, cut)
            mult[(lvl > l) & (cells >= cut) & (cells < cut + cell_cap)] = 0.0
    elif mutant == MUTANTS[5]:  # the later trip's first slot is l_lo * max P where lvl_start(l_lo) belongs
        counts = c["counts"]
        pt = np.broadcast_to(np.arange(cells.shape[4]).reshape(1, 1, 1, 1, -1), cells.shape)
        for cut in count:
            l_lo = level_of_cell(levels, cut)
            skipped = l_lo * max(counts) - sum(counts[:l_lo])  # slots between the right base and the wrong one
            assert skipped > 0, (name, counts)
            left, gone = skipped, np.zeros(cells.shape, bool)
            for l in range(l_lo, len(levels)):
                gone |= (lvl == l) & (pt < min(left, counts[l]))
                left -= min(left, counts[l])
            mult[gone & (cells >= cut) & (cells < cut + cell_cap)] = 0.0
    else:
        raise ValueError(mutant)
    return mult
