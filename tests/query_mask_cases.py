"""Query padding masks: the generators and sanitisers shared by tests/test_query_mask.py (CPU: the contract belongs to the
operation, and the generators' own promises are checked there) and tests/test_gpu_query_mask.py (GPU: the kernels keep it).

A query mask is ``[B, Q]`` bool, True = the query is real.  KINDS:

    bernoulli        every query real with p = 0.5
    tail             the last 40 % of the LAST batch element's queries are masked (the rectangle a Hugging Face encoder sees:
                     the padded part of an image is a suffix of every level's rows)
    element0_masked  batch element 0 has no real query
    all_ones         no query masked
    all_zeros        no query real
    one_real_query   exactly one query of the whole batch is real
    slice_edges      the mask flips exactly at, one before and one after every boundary in ``slice_boundaries``: the
                     multiples (below Q) of the query counts at which one of the pipeline's passes hands the queries of a
                     plane from one wave, workgroup or slice to the next

Every kind except ``all_ones`` leaves at most ``max_real_share`` of the queries real (asserted by ``make_query_mask``), so a
kernel that ignores the mask cannot pass by luck.

``sanitised`` is the issue's reference input: masked queries get points 0.5, weights (or logits and offsets) 0 and a zero
``grad_out`` row."""
import os
import re

import numpy as np
import torch

KINDS = ("bernoulli", "tail", "element0_masked", "all_ones", "all_zeros", "one_real_query", "slice_edges")
MAX_REAL_SHARE = {"bernoulli": 0.75, "tail": 0.8, "element0_masked": 0.75, "all_zeros": 0.0, "one_real_query": 0.5,
                  "slice_edges": 0.75}
TAIL_SHARE = 0.4


def max_real_share(kind, B, Q):
    """the stated share; `tail` masks 40 % of ONE element's queries (rounded to a whole query), so its share depends on B"""
    return 1 - TAIL_SHARE / B + 1 / (B * Q) if kind == "tail" else MAX_REAL_SHARE[kind]

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "msda_triton_amd", "csrc")


def pipeline_constants():
    """the `constexpr int k... = N;` constants of the kernels' sources that decide which queries share a wave, a workgroup
    or a slice — read from the sources, so that the boundaries below move with them"""
    text = "".join(open(os.path.join(_CSRC, f)).read() for f in ("msda_common.hpp", "msda_value_sorted.hpp",
                                                                 "msda_value_place.hpp", "msda_value_small.hpp"))
    found = {k: int(v) for k, v in re.findall(r"constexpr int (k[A-Za-z]+) = (\d+);", text)}
    return {k: found[k] for k in ("kWave", "kBlock", "kBlockLds", "kCellBlock", "kPlaceBlock", "kPlaceBlockSmall",
                                  "kSmallBlock", "kWinMax", "kWinMin", "kScanCells")}


def pick_group(lanes):
    """msda_launch.hpp: lanes of a unit for a row of `lanes` pieces"""
    return next(g for g in (4, 8, 16, 32, 64) if lanes <= g or g == 64)


def unit_lanes(D, elem_size):
    """the G of the gather kernels for rows of D elements: 16-byte pieces when D allows them, else one element per lane"""
    vec = 16 // elem_size
    return pick_group(D // vec if D % vec == 0 else D)


def cell_slices(B, I, H, Q, LP):  # noqa: E741
    """sorted_ws_layout's `nsplit` for one round over the queries: the query slices of the count and place passes"""
    pairs, samples = B * H, Q * LP
    ns = min((256 + pairs - 1) // pairs, (samples + 2047) // 2048, (9 * samples) // (2 * I), 64, Q)
    return max(1, ns)


def slice_boundaries(B, Q, H, D, levels, P, elem_size=4):
    """-> sorted query indices b (0 < b < Q) at which a pass of the pipeline changes hands, each with the reason:

    * the forward / sample-gradient kernels: a wave's kWave / G units, a workgroup's kBlock / G and kBlockLds / G units
    * the count and place passes of the sorted pipeline: the query slices (ceil(Q / nsplit) queries each), the
      kCellBlock / (L * P) queries a count workgroup covers per trip and the kPlaceBlock / P, kPlaceBlockSmall / P queries a
      place workgroup covers per round
    * the single-launch kernel: kSmallBlock / P queries per round of its walks
    * the gather's windows of kWinMax records, in queries: kWinMax / P and kWinMax / (L * P) where those are whole numbers
      (the records of one cell are in query order, P or L * P of a query's samples at a time)
    Only the first two multiples of each step are kept: the mask stays short of dense."""
    k = pipeline_constants()
    L = len(levels)
    I = sum(h * w for h, w in levels)  # noqa: E741
    G = unit_lanes(D, elem_size)
    steps = {"wave units": k["kWave"] // G, "workgroup units": k["kBlock"] // G, "lds workgroup units": k["kBlockLds"] // G,
             "count trip": max(1, k["kCellBlock"] // (L * P)), "place round": max(1, k["kPlaceBlock"] // P),
             "small place round": max(1, k["kPlaceBlockSmall"] // P), "single-launch round": max(1, k["kSmallBlock"] // P),
             "query slice": -(-Q // cell_slices(B, I, H, Q, L * P))}
    for name, per in (("window / P", P), ("window / LP", L * P)):
        if k["kWinMax"] % per == 0:
            steps[name] = k["kWinMax"] // per
    out = {}
    for name, step in steps.items():
        for mult in (1, 2):
            b = step * mult
            if 0 < b < Q:
                out.setdefault(b, name)
    return dict(sorted(out.items()))


def make_query_mask(kind, B, Q, seed, shape=None):
    """[B, Q] bool on the host, True = real query; seeded.  `shape` = (B, Q, H, D, levels, P[, elem_size]) for slice_edges."""
    g = torch.Generator().manual_seed(seed)
    m = torch.ones(B, Q, dtype=torch.bool)
    if kind == "bernoulli":
        m = torch.rand(B, Q, generator=g) < 0.5
    elif kind == "tail":
        m[B - 1, Q - max(1, int(round(Q * TAIL_SHARE))):] = False
    elif kind == "element0_masked":
        m[0] = False
        if B > 1:  # (the other elements keep a seeded half, so that the share holds for B = 2 as well)
            m[1:] = torch.rand(B - 1, Q, generator=g) < 0.5
    elif kind == "all_zeros":
        m[:] = False
    elif kind == "one_real_query":
        m[:] = False
        m[int(torch.randint(B, (1,), generator=g)), int(torch.randint(Q, (1,), generator=g))] = True
    elif kind == "slice_edges":
        # runs of real / masked queries that flip at b - 1, b and b + 1 of every boundary: ... 1 0 | 1 0 ... around b
        # (q = b - 1 real, b masked, b + 1 real in element 0; the complement in element 1, so both polarities meet every edge)
        m = torch.rand(B, Q, generator=g) < 0.3
        for b in slice_boundaries(*shape):
            for e in range(B):
                pol = e % 2 == 0
                for q, v in ((b - 2, not pol), (b - 1, pol), (b, not pol), (b + 1, pol)):
                    if 0 <= q < Q:
                        m[e, q] = v
    elif kind != "all_ones":
        raise ValueError(kind)
    if kind in MAX_REAL_SHARE and B * Q >= 8:
        assert m.float().mean().item() <= max_real_share(kind, B, Q), (kind, m.float().mean().item())
    return m


def sanitised(c, qm):
    """numpy case dict (value, shapes, loc, attn, grad_out) -> the same with the masked queries' points 0.5, weights 0 and
    grad_out rows 0"""
    real = np.asarray(qm, dtype=bool)
    c = {k: np.array(v, copy=True) for k, v in c.items()}
    c["loc"][~real] = 0.5
    c["attn"][~real] = 0.0
    c["grad_out"][~real] = 0.0
    return c


def sanitised_fused(proj, ref, gout, qm):
    """torch tensors of a fused family -> masked queries' projection (offsets and logits) 0, reference points 0.5, grad_out 0"""
    sel = qm.to(proj.device)
    return (torch.where(sel.reshape(sel.shape + (1,) * (proj.dim() - 2)), proj, torch.zeros_like(proj)),
            torch.where(sel.reshape(sel.shape + (1,) * (ref.dim() - 2)), ref, torch.full_like(ref, 0.5)),
            torch.where(sel.reshape(sel.shape + (1,) * (gout.dim() - 2)), gout, torch.zeros_like(gout)))


def hostile_fill(t, qm, values):
    """torch tensor [B, Q, ...] -> the masked queries' entries replaced by `values`, cycling (NaN, +Inf, 1e30 ...)"""
    vals = torch.tensor(list(values), dtype=torch.float64)
    flat_idx = torch.arange(t.numel(), device="cpu").reshape(t.shape)
    fill = vals[flat_idx % len(vals)].to(t.dtype).to(t.device)
    sel = qm.to(t.device).reshape(qm.shape + (1,) * (t.dim() - 2))
    return torch.where(sel, t, fill)


# ----------------------------------------------------------------------------------------- exact inputs under a query mask
EXACT = ("d32_vec_g8", "d5_scalar", "d8_vec_g4", "lds_q200", "b4_passes", "flood")  # tests/exact_cases.py, uniform point counts


def exact_query_mask(name, kind):
    import exact_cases as ec
    B, Q, H, D, levels, P = ec.CASES[name][1]
    return make_query_mask(kind, B, Q, zlib_seed(name, kind), (B, Q, H, D, levels, P))


def zlib_seed(*parts):
    import zlib
    return zlib.crc32("/".join(str(p) for p in parts).encode())


def exact_reference(name, pm, ac, qm):
    """The fp64 reference of an exact case (tests/exact_cases.py) under a query mask: the oracle on the sanitised inputs.
    Exact whenever the unmasked case is — every result is a sum over a SUBSET of the unmasked case's terms (a masked query
    contributes nothing), so each condition sum can only shrink and the bit budget with it; both are asserted here, and the
    float32 oracle is again held to the float64 one bit for bit.  -> (sanitised case, reference dict)"""
    import exact_cases as ec
    full = ec.precondition(name, pm, ac)  # (the unmasked case's budget; asserts that case's own exactness)
    c = ec.get_case(name)
    s = sanitised({k: v for k, v in c.items() if isinstance(v, np.ndarray)}, qm)
    s["bits"] = c["bits"]
    bud = ec.budget(s, pm, ac)
    for k in ("out", "grad_value", "grad_attn", "grad_loc"):
        assert bud[k] <= full[k] <= ec.F32_BITS, (name, pm, ac, k, bud, full)
    ref = ec._oracle_all(ec._oracle(), s, pm, ac, np.float64)
    f32 = ec._oracle_all(ec._oracle(), s, pm, ac, np.float32)
    for k, r in ref.items():
        assert np.array_equal(f32[k].astype(np.float64), r), f"{name} {pm} {ac} query-masked: float32 and float64 differ in {k}"
    return s, ref
