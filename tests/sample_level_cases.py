"""The two structural axes besides the head dimension that choose different CODE, not different sizes: the samples of a
(b, q, h) unit (S = L * P, or the sum of points_per_level) and the level count L.  A helper module, not a conftest.

S decides how many TRIPS a kernel makes over a unit's samples — the refill of the parked records, the partial last trip,
the per-trip exchange batches of the reduce-scatter sample gradients — and which kernel runs at all (the one-wave-per-unit
forward up to 1024 samples, the level-major place passes up to 256 and 1024 points per level).  L decides the scan of
`load_level_table` (a DPP row scan with a step more at L > 2, 4, 8; a shuffle loop beyond 16), how far the unrolled scans
over the per-level-count starts run, and the level field of grad_value's cell words.

The rules below are RESTATED from msda_launch.hpp (plan_gather, lds_levels_plan_rt, launch_gather) the way
head_dim_cases.fused_lp_limit restates its rule; the GPU tests hold `msda_last_launch_info` ("fwd_trips",
"sample_trips", the variants, the groups, the grad_value path and place-pass variant) to them, so a moved threshold fails
a test instead of quietly turning it into a duplicate.  The cases themselves are exact inputs, registered in
exact_cases.CASES: "sc_*" (trips of the 256-thread kernels), "lds_*" (of the LDS-served-level kernels), "uf_*" (the
one-wave-per-unit forward's boundaries), "pl_*" (the place pass's) and "lv<L>_*" (the level counts)."""
import numpy as np

import exact_cases as ec
import head_dim_cases as hd

# ----------------------------------------------------------------------------------------- msda_launch.hpp, restated
KIB = 1024
RECORD_BUDGET = 48 * KIB          # kRecordLdsBudget: parked sample records of a 256-thread workgroup
LDS_RECORD_BUDGET = 72 * KIB      # kRecordLdsBudgetLds: ... of a 1024-thread workgroup with LDS-served levels
LDS_RECORD_BUDGET_AUX = 100 * KIB  # ... the fused backward's larger records
BLOCK, BLOCK_LDS, WAVE = 256, 1024, 64
MAX_LEVELS = 32                   # kMaxLevels: the last entry of every [kMaxLevels] table is level 31
FUSED_RAGGED_MAX_LEVELS = 8       # kFusedRaggedMaxLevels: the fused per-level-count / box kernels' level scan
UNIT_FWD_MAX_SAMPLES = 1024       # launch_gather: p.LP <= 1024
UNIT_FWD_MAX_UNITS = 12288        # kUnitFwdMaxUnits (option unit_fwd = 1; 2 lifts it)
PLACE_BLOCK_SMALL, PLACE_BLOCK = 256, 1024  # kPlaceBlockSmall, kPlaceBlock
ERR_BAD_ARG, ERR_UNSUPPORTED = -1, -5  # include/msda_hip.h

ACC_BYTES = {"f32": 4, "f64": 8, "fp16": 4, "bf16": 4, "f32_vbf16": 4, "f32_vf16": 4}  # Traits<T>::acc
MODES = ec.MODES
SAMPLE_MODES = [("zeros", False), ("border", True)]


def ceil_div(a, b):
    return -(-a // b)


def record_bytes(acc, aux=False):
    """plan_gather's `rec`: 16 bytes of offsets plus 4 accumulators, 7 for the fused backward's (a, ox, oy) per slot"""
    return 16 + (7 if aux else 4) * acc


def gather_cap(G, acc=4, aux=False, block=BLOCK, budget=RECORD_BUDGET):
    """plan_gather: samples of a unit parked per trip — the budget over the workgroup's block / G units, less one"""
    return max(1, budget // ((block // G) * record_bytes(acc, aux)) - 1)


def plan_gather(G, S, acc=4, aux=False):
    """-> (sc, trips) of the 256-thread forward and sample-gradient kernels"""
    sc = min(S, gather_cap(G, acc, aux))
    return sc, ceil_div(S, sc)


def lds_plan(G, S, acc=4, aux=False):
    """lds_levels_plan_rt: the 1024-thread kernels' (sc, trips) — a multi-trip sc above G rounded DOWN to a multiple of G
    (whole exchange batches of the sample-gradient kernel per trip)"""
    sc = min(S, gather_cap(G, acc, aux, BLOCK_LDS, LDS_RECORD_BUDGET_AUX if aux else LDS_RECORD_BUDGET))
    if sc < S and sc > G:
        sc = sc // G * G
    return sc, ceil_div(S, sc)


def fused_limit(D, elem_size=4):
    """msda_fused_lp_limit: plan_gather's cap with the fused backward's records, for the narrower of the lane groups the
    16-byte path and the scalar path would take"""
    acc = 8 if elem_size == 8 else 4
    return min(gather_cap(hd.pick_group(ceil_div(D, vec)), acc, aux=True) for vec in (16 // elem_size, 1))


def unit_trips(S, U=1):
    """msda_fwd_unit_kernel: a unit's 64 / U lanes take one sample each per trip"""
    return ceil_div(S, WAVE // U)


def place_variant(P, q_slice=1):
    """run_value_sorted_on, option place_path = 0: 2 = level-major with 256 threads (P <= 256 and a slice's queries covered
    by six rounds of workgroups), 1 = level-major with 1024 threads, 0 = the plane-major pass (P > 1024; strict = 0 only)"""
    if P > PLACE_BLOCK:
        return 0
    return 2 if P <= PLACE_BLOCK_SMALL and q_slice <= 6 * (PLACE_BLOCK_SMALL // P) else 1


def expect(storage, D, S, *, unit_fwd=1, unit_waves=1, lds_levels=1, masked=False, discrete=False, units=1):
    """The launch-info keys of a forward + backward of the plain families (launch_gather / launch_discrete).  lds_levels = 1
    counts as 0: the plan takes the variant only where its workgroups fill the chip, hundreds of times these cases' units."""
    vec, g, _ = hd.instantiation(storage, D)
    acc, arith = ACC_BYTES[storage], hd.ARITH_BYTES[storage]
    if discrete:
        return dict(fwd_variant=3, sample_variant=2, fwd_group=g, sample_group=g, fwd_trips=1, sample_trips=1)
    gl = D // vec
    unit = (unit_fwd != 0 and not masked and vec * arith == 16 and acc == 4 and gl <= WAVE and gl & (gl - 1) == 0 and
            S <= UNIT_FWD_MAX_SAMPLES and (unit_fwd == 2 or units <= UNIT_FWD_MAX_UNITS))
    lds_f = lds_levels == 2 and vec == 4 and acc == 4 and g <= 16          # (16-bit operators: VEC = 8 — no variant)
    lds_s = lds_levels == 2 and vec == 4 and acc == 4 and arith == 4 and g in (4, 8)
    e = {}
    if unit:
        U = 2 if unit_waves == 2 and gl <= WAVE // 2 else 1
        e.update(fwd_variant=2, fwd_group=gl, fwd_trips=unit_trips(S, U))
    elif lds_f:
        e.update(fwd_variant=1, fwd_group=g, fwd_trips=lds_plan(g, S, acc)[1])
    else:
        e.update(fwd_variant=0, fwd_group=g, fwd_trips=plan_gather(g, S, acc)[1])
    e.update(sample_variant=int(lds_s), sample_group=g, sample_trips=(lds_plan if lds_s else plan_gather)(g, S, acc)[1])
    return e


def assert_info(info, want, what):
    got = {k: info[k] for k in want}
    assert got == want, (what, got, want)


# ----------------------------------------------------------------------------------------- pyramids of tiny unequal levels
# 1 x 1 and one-pixel axes among them, no two neighbours alike, so that a wrong `start` / `cstart` lands on another level's
# pixels.  Every axis is at most 7 pixels: with sampling points on odd multiples of 2^-4 no sample then sits on an integer
# pixel coordinate (that would take an axis of 8 k pixels, or of 16 k + 1 under align_corners), which the precondition asks.
_POOL = [(3, 2), (1, 1), (2, 5), (1, 4), (4, 1), (2, 2), (5, 3), (1, 1), (3, 3), (6, 1), (1, 7), (2, 3), (4, 4), (1, 2), (7, 2),
         (3, 1), (2, 6), (1, 1), (5, 2), (1, 3), (3, 4), (2, 1), (6, 2), (1, 5), (4, 3), (2, 2), (1, 6), (5, 1), (3, 5), (1, 1),
         (2, 4), (7, 3)]
assert len(_POOL) == MAX_LEVELS
LEVEL_COUNTS = (1, 2, 3, 5, 8, 9, 16, 17, 32)
_COUNT_PATTERN = (3, 2, 4, 2, 5, 3, 2, 4)


def pyramid(L):
    return list(_POOL[:L])


def level_point_counts(L):
    """A per-level count list whose SMALLEST counts — one point, the least the C ABI admits: a count of 0 is
    MSDA_ERR_BAD_ARG — stand at the front, in the middle and at the end, with the last level's single sample the unit's last
    (fewer than five levels: at the front only)"""
    ones = (0, L // 2, L - 1) if L >= 5 else (0,) if L >= 2 else ()
    return [1 if i in ones else _COUNT_PATTERN[i % len(_COUNT_PATTERN)] for i in range(L)]


_KW = dict(loc_bits=4, attn_bits=2, vmax=1, gmax=1)
_KW_LONG = dict(loc_bits=4, attn_bits=1, vmax=1, gmax=1)     # S in the hundreds: fewer weight bits (chosen on the CPU, below)
_KW_DISC = dict(attn_bits=5, value_bits=3, grad_bits=3)
_ALL16 = (ec.F16, ec.BF16)

LEVEL_CASES = []
for _L in LEVEL_COUNTS:
    _lv = pyramid(_L)
    ec.CASES[f"lv{_L}_p2"] = ("bilinear", (2, 13, 2, 32, _lv, 2), _KW, _ALL16)
    ec.CASES[f"lv{_L}_d5"] = ("bilinear", (2, 13, 2, 5, _lv, 2), _KW, _ALL16)
    ec.CASES[f"lv{_L}_c"] = ("bilinear", (2, 13, 2, 32, _lv, level_point_counts(_L)), _KW, _ALL16)
    ec.CASES[f"lv{_L}_disc"] = ("discrete", (2, 13, 2, 32, _lv, level_point_counts(_L)), _KW_DISC, (ec.BF16,))
    LEVEL_CASES += [f"lv{_L}_p2", f"lv{_L}_d5", f"lv{_L}_c", f"lv{_L}_disc"]
# L = 32 in the sorted pipeline in rounds of queries and two passes over the batch
LEVEL_ROUNDS_CASE, LEVEL_ROUNDS_OPTIONS = "lv32_p2", dict(value_path=2, q_round=5, ws_passes=2)

# ----------------------------------------------------------------------------------------- sample-count classes
SAMPLE_CLASSES = ("cap", "cap+1", "2cap", "3trips+")
# the float32 D of each lane group on the 16-byte path, and one scalar-path D (5 lanes: G = 8)
SAMPLE_DIMS = {"g4": 8, "g8": 32, "g16": 64, "g32": 128, "g64": 256, "scalar": 5}
LDS_DIMS = {"g4": 8, "g8": 32, "g16": 64}  # (the variant exists up to G = 16; its sample gradients for G = 4 and 8)
_TWO_LEVELS = [(5, 4), (3, 2)]


def one_trip_cap(plan):
    """the largest S a kernel with `plan(S) -> (sc, trips)` serves in one trip"""
    S = 1
    while plan(S + 1)[1] == 1:
        S += 1
    return S


def class_samples(plan, cls):
    """The S of a class: the largest one-trip S; one more; two FULL trips of what the plan then parks per trip (the LDS
    plan's rounded sc, not its cap); and two full trips plus a third of one — three trips, the last one partial."""
    cap = one_trip_cap(plan)
    sc = plan(cap + 1)[0]
    return {"cap": cap, "cap+1": cap + 1, "2cap": 2 * sc, "3trips+": 2 * sc + max(1, sc // 3)}[cls]


def sample_class(S, plan):
    """Which of SAMPLE_CLASSES S is for a kernel with that plan; None: none of them."""
    sc, trips = plan(S)
    if trips == 1:
        return "cap" if plan(S + 1)[1] == 2 else None
    if trips == 2 and plan(S - 1)[1] == 1:
        return "cap+1"
    if trips == 2 and S == 2 * sc:
        return "2cap"
    if trips >= 3 and S % sc:
        return "3trips+"
    return None


def _uniform_split(S):
    """(levels, P) with len(levels) * P = S: two or three levels where S divides, one otherwise (the caps are odd, some prime)"""
    for n in (2, 3):
        if S % n == 0:
            return pyramid(n + 1)[1:] if n == 2 else pyramid(3), S // n
    return [(5, 4)], S


SAMPLE_CASES, LDS_CASES = [], []
for _tag, _D in SAMPLE_DIMS.items():
    _G = hd.instantiation("f32", _D)[1]
    assert _tag in (f"g{_G}", "scalar") and (_tag != "scalar" or hd.instantiation("f32", _D)[0] == 1)
    for _cls in SAMPLE_CLASSES:
        _S = class_samples(lambda s, g=_G: plan_gather(g, s), _cls)
        _kw = _KW_LONG if _S > 100 else _KW
        _lv, _P = _uniform_split(_S)
        _name = f"sc_{_tag}_{_cls}"
        ec.CASES[_name] = ("bilinear", (2, 7, 2, _D, _lv, _P), _kw, _ALL16)
        ec.CASES[_name + "_c"] = ("bilinear", (2, 7, 2, _D, _TWO_LEVELS, [_S - _S // 3, _S // 3]), _kw, _ALL16)
        SAMPLE_CASES += [_name, _name + "_c"]
for _tag, _D in LDS_DIMS.items():
    _G = hd.instantiation("f32", _D)[1]
    # cap: one trip; cap + 1: the first S that does not fit — where the rounding to a multiple of G takes hold (17 -> 16 at
    # G = 8, 35 -> 32 at G = 16); 2 * cap, and three trips and more with a partial last one
    for _cls in SAMPLE_CLASSES:
        _S = class_samples(lambda s, g=_G: lds_plan(g, s), _cls)
        _lv, _P = _uniform_split(_S)
        _name = f"lds_{_tag}_{_cls}"
        ec.CASES[_name] = ("bilinear", (2, 37, 2, _D, _lv, _P), _KW, (ec.BF16,))
        ec.CASES[_name + "_c"] = ("bilinear", (2, 37, 2, _D, _TWO_LEVELS, [_S - _S // 3, _S // 3]), _KW, (ec.BF16,))
        LDS_CASES += [_name, _name + "_c"]

# the one-wave-per-unit forward: one trip | two at 64 | 65 samples with one unit per wave and at 32 | 33 with two; eligible up
# to 1024 samples, declined at 1025.  S: (L, P) — every S has a uniform split over more than one level
UNIT_SAMPLES = {32: (2, 16), 33: (3, 11), 64: (4, 16), 65: (5, 13), 1024: (4, 256), 1025: (5, 205)}
UNIT_D = 32
UNIT_CASES = []
for _S, (_L, _P) in UNIT_SAMPLES.items():
    _kw = _KW_LONG if _S > 100 else _KW
    ec.CASES[f"uf_s{_S}"] = ("bilinear", (2, 9, 2, UNIT_D, pyramid(_L), _P), _kw, (ec.BF16,))
    ec.CASES[f"uf_s{_S}_c"] = ("bilinear", (2, 9, 2, UNIT_D, _TWO_LEVELS, [_S - _S // 3, _S // 3]), _kw, (ec.BF16,))
    UNIT_CASES += [f"uf_s{_S}", f"uf_s{_S}_c"]

# the place pass of the sorted grad_value pipeline, by P alone (two levels: S = 2 P); Q = 5 keeps a query slice within the
# six rounds of 256-thread workgroups that P = 256 allows
PLACE_POINTS = (256, 257, 1024, 1025)
PLACE_CASES = []
for _P in PLACE_POINTS:
    ec.CASES[f"pl_p{_P}"] = ("bilinear", (1, 5, 2, 8, _TWO_LEVELS, _P), _KW_LONG, (ec.BF16,))
    PLACE_CASES.append(f"pl_p{_P}")

ALL_CASES = LEVEL_CASES + SAMPLE_CASES + LDS_CASES + UNIT_CASES + PLACE_CASES


def case_dims(name):
    """(B, Q, H, D, L, S, P or None, counts or None) of a registered case"""
    B, Q, H, D, levels, P = ec.CASES[name][1]
    if isinstance(P, int):
        return B, Q, H, D, len(levels), len(levels) * P, P, None
    return B, Q, H, D, len(levels), sum(P), None, list(P)


def case_modes(name):
    """all four padding / align modes on the level-count classes, two on the sample-count classes; discrete sampling knows none"""
    if ec.CASES[name][0] == "discrete":
        return [("border", False)]
    return MODES if name.startswith("lv") else SAMPLE_MODES


# ----------------------------------------------------------------------------------------- the fused families
# The softmax rules equality out: these are generic inputs in the shape of tests/error_bound_cases.py (registered in its
# FUSED_MORE / FUSED_SHAPES tables), held to ITS derived bound against its fp64 composition — no tolerance of this module's.
#   "<base>_<g>_limit"  S = msda_fused_lp_limit(D, 4) exactly, one D per lane group: the fused kernels' one LDS pass, full
#   "<base>_<g>_over"   S = limit + 1: the backward declines and the package composes it around the plain operator (the
#                       forward's records are smaller: it may still be the fused kernel); the same bound
#   "<base>_l8" / "_l9" per-level counts at the fused level scan's bound (in the kernels) and one beyond (composed)
FUSED_BASES = ("module2", "module4_c", "levelref4", "hfbox")      # uniform, per-level counts, per-level reference, box rule
FUSED_LEVEL_BASES = ("module4_c", "hfbox", "hfbox_discrete")      # the families whose level scan is bounded
FUSED_LIMIT_DIMS = {"g4": 8, "g8": 32, "g16": 64, "g32": 128, "g64": 256}
FUSED_SHAPE = dict(B=1, Q=5, H=2)
FUSED_MODES = [("zeros", False), ("border", True)]
FUSED_CASES = {}  # name: (base, fused kernels expected, D, S, L)


def _register_fused():
    import error_bound_cases as eb
    for tag, D in FUSED_LIMIT_DIMS.items():
        limit = fused_limit(D)
        for kind, S in (("limit", limit), ("over", limit + 1)):
            for base in FUSED_BASES:
                rule, ref_dim, p0 = eb.FUSED[base]
                if isinstance(p0, int):
                    L = next(n for n in (3, 2, 1) if S % n == 0)
                    P = S // L
                else:
                    L, P = 3, [S - 2 * (S // 3) + 1, S // 3 - 1, S // 3]  # (unequal: equal counts are the uniform call)
                name = f"{base}_{tag}_{kind}"
                eb.FUSED_MORE[name] = (rule, ref_dim, P)
                eb.FUSED_SHAPES[name] = (dict(FUSED_SHAPE, D=D), eb.LEVELS[:L])
                FUSED_CASES[name] = (base, kind == "limit", D, S, L)
    for base in FUSED_LEVEL_BASES:
        rule, ref_dim, _ = eb.FUSED[base]
        for L in (FUSED_RAGGED_MAX_LEVELS, FUSED_RAGGED_MAX_LEVELS + 1):
            name = f"{base}_l{L}"
            counts = level_point_counts(L)
            eb.FUSED_MORE[name] = (rule, ref_dim, counts)
            eb.FUSED_SHAPES[name] = (dict(FUSED_SHAPE, Q=13, D=32), pyramid(L))
            FUSED_CASES[name] = (base, L <= FUSED_RAGGED_MAX_LEVELS, 32, sum(counts), L)
            if base in eb.FUSED_DISCRETE:
                eb.FUSED_DISCRETE.add(name)


_register_fused()


def fused_modes(name):
    import error_bound_cases as eb
    return [("border", False)] if name in eb.FUSED_DISCRETE else FUSED_MODES


# ----------------------------------------------------------------------------------------- what the case list must reach
def required():
    """(variant, group or tag, class) — every class the sweep is written for"""
    need = {("block256", t, c) for t in SAMPLE_DIMS for c in SAMPLE_CLASSES}
    need |= {("lds_fwd", t, c) for t in LDS_DIMS for c in SAMPLE_CLASSES}
    need |= {("lds_sample", t, c) for t in ("g4", "g8") for c in SAMPLE_CLASSES}
    need |= {("lds_rounded", t, "sc") for t in ("g8", "g16")}
    need |= {("unit", f"u{u}", b) for u, bs in ((1, ("64|65", "1024|1025")), (2, ("32|33", "1024|1025"))) for b in bs}
    need |= {("place", "p", v) for v in ("256|257", "1024|1025")}
    need |= {("levels", fam, L) for fam in ("uniform", "scalar", "counts", "discrete") for L in LEVEL_COUNTS}
    return need


def reached():
    got = set()
    for name in SAMPLE_CASES:
        _, _, _, D, _, S, _, _ = case_dims(name)
        tag = name.split("_")[1]
        G = hd.instantiation("f32", D)[1]
        cls = sample_class(S, lambda s: plan_gather(G, s))
        if cls:
            got.add(("block256", tag, cls))
    for name in LDS_CASES:
        _, _, _, D, _, S, _, _ = case_dims(name)
        tag = name.split("_")[1]
        G = hd.instantiation("f32", D)[1]
        e = expect("f32", D, S, unit_fwd=0, lds_levels=2)
        cls = sample_class(S, lambda s: lds_plan(G, s))
        if cls and e["fwd_variant"] == 1:
            got.add(("lds_fwd", tag, cls))
        if cls and e["sample_variant"] == 1:
            got.add(("lds_sample", tag, cls))
        sc = lds_plan(G, S)[0]
        if sc < S and sc != gather_cap(G, 4, False, BLOCK_LDS, LDS_RECORD_BUDGET):
            got.add(("lds_rounded", tag, "sc"))
    samples = {case_dims(n)[5] for n in UNIT_CASES}
    for U, lanes in ((1, 64), (2, 32)):
        if {lanes, lanes + 1} <= samples and unit_trips(lanes, U) == 1 and unit_trips(lanes + 1, U) == 2:
            got.add(("unit", f"u{U}", f"{lanes}|{lanes + 1}"))
        e0, e1 = (expect("f32", UNIT_D, s, unit_fwd=2, unit_waves=U, lds_levels=0) for s in (1024, 1025))
        if {1024, 1025} <= samples and e0["fwd_variant"] == 2 and e1["fwd_variant"] == 0:
            got.add(("unit", f"u{U}", "1024|1025"))
    pts = {case_dims(n)[6] for n in PLACE_CASES}
    for a, b in ((256, 257), (1024, 1025)):
        if {a, b} <= pts and place_variant(a) != place_variant(b):
            got.add(("place", "p", f"{a}|{b}"))
    for name in LEVEL_CASES:
        _, _, _, D, L, _, _, counts = case_dims(name)
        fam = ("discrete" if ec.CASES[name][0] == "discrete" else "counts" if counts else
               "scalar" if hd.instantiation("f32", D)[0] == 1 else "uniform")
        got.add(("levels", fam, L))
    return got


# ----------------------------------------------------------------------------------------- a query mask on an exact case
def query_mask(name):
    """[B, Q] bool on the host, True = real: the first seeded Bernoulli draw of the case's own sequence that
    query_mask_cases admits (its cap on the share of real queries is a condition on the fixture, and Q is small here)"""
    import query_mask_cases as qmc
    B, Q = ec.CASES[name][1][:2]
    for k in range(64):
        try:
            m = qmc.make_query_mask("bernoulli", B, Q, qmc.zlib_seed("sample_level", name, k))
        except AssertionError:
            continue
        if 0 < int(m.sum()):
            return m
    raise AssertionError(f"no admissible query mask for {name}")


# ----------------------------------------------------------------------------------------- emulated wrong kernels (CPU, fp64)
def level_starts(shapes):
    n = shapes[:, 0] * shapes[:, 1]
    return np.cumsum(n) - n


def scan_without_shift(shapes, shift):
    """The level starts of a 16-lane inclusive row scan (steps 1, 2, 4, 8) that OMITS the step `shift`, less the own size."""
    n = (shapes[:, 0] * shapes[:, 1]).astype(np.int64)
    x = n.copy()
    for step in (1, 2, 4, 8):
        if step == shift:
            continue
        y = x.copy()
        y[step:] += x[:-step] if step < len(x) else 0
        x = y
    return x - n


def _dense(c):
    """exact_cases.dense, and no longer a per-level-count case (what `taps` is then handed is the padded layout itself)"""
    return {k: v for k, v in ec.dense(c).items() if k != "counts"}


def gather_out(c, pm, ac, row=None, start=None, keep=None):
    """`out` of the (dense) case in numpy fp64 by the gather formulation, [B, Q, H, D].  row [L]: the level-table row each
    level's samples READ (a truncated or wrapped table); start [L]: the table's pixel starts (a wrong scan); keep
    [B, Q, H, L, P] bool: the samples that are summed (a dropped trip)."""
    d = _dense(c)
    shapes = d["shapes"]
    L = len(shapes)
    row = np.arange(L) if row is None else np.asarray(row)
    start = level_starts(shapes) if start is None else np.asarray(start)
    used = dict(d, shapes=shapes[row])
    idx, mask, wgt = ec.taps(used, pm, ac)
    true0 = level_starts(used["shapes"]).reshape(1, 1, 1, -1, 1)
    moved = start[row].reshape(1, 1, 1, -1, 1)
    B, I, H, D = d["value"].shape
    bi, hi = np.arange(B).reshape(B, 1, 1, 1, 1), np.arange(H).reshape(1, 1, H, 1, 1)
    total = 0.0
    for k in range(4):
        px = np.clip(idx[k] - true0 + moved, 0, I - 1)  # (a kernel's descriptor keeps a wrong offset inside the plane, or reads 0)
        total = total + np.where(mask[k], wgt[k], 0.0)[..., None] * d["value"][bi, px, hi]
    con = d["attn"][..., None] * total
    if keep is not None:
        con = np.where(keep[..., None], con, 0.0)
    return con.sum((3, 4))


def gather_grad_value(c, pm, ac, cell_level=None):
    """grad_value of the (dense) case in numpy fp64 by scatter, [B, I, H, D]; cell_level [L]: the level a cell word of level l
    is READ as (a level field of too few bits) — its pixels land at that level's start."""
    d = _dense(c)
    shapes = d["shapes"]
    idx, mask, wgt = ec.taps(d, pm, ac)
    st = level_starts(shapes)
    lv = np.arange(len(shapes)) if cell_level is None else np.asarray(cell_level)
    shift = (st[lv] - st).reshape(1, 1, 1, -1, 1)
    B, I, H, D = d["value"].shape
    gv = np.zeros((B, I, H, D))
    bi = np.broadcast_to(np.arange(B).reshape(B, 1, 1, 1, 1), idx[0].shape)
    hi = np.broadcast_to(np.arange(H).reshape(1, 1, H, 1, 1), idx[0].shape)
    g = np.broadcast_to(d["grad_out"][:, :, :, None, None, :], idx[0].shape + (D,))
    for k in range(4):
        w = np.where(mask[k], wgt[k], 0.0) * d["attn"]
        np.add.at(gv, (bi, np.clip(idx[k] + shift, 0, I - 1), hi), w[..., None] * g)
    return gv


def sample_index(c):
    """[L, P] of the dense layout: a sample's index inside its unit (level-major), -1 for `dense`'s padding"""
    d = ec.dense(c)
    L, P = d["loc"].shape[3:5]
    counts = c.get("counts", [P] * L)
    out, s0 = np.full((L, P), -1), 0
    for l, n in enumerate(counts):
        out[l, :n] = np.arange(s0, s0 + n)
        s0 += n
    return out


def keep_without_last_trip(c, sc):
    """the samples a kernel sums that DROPS a unit's last, partial trip of `sc` samples per trip"""
    si = sample_index(c)
    S = int(si.max()) + 1
    assert S % sc, "the last trip is full"
    return np.broadcast_to((si >= 0) & (si < S // sc * sc), ec.dense(c)["attn"].shape)


def keep_without_last_sample(c):
    """... whose pst[L] is one short: the last level's last sample is lost"""
    si = sample_index(c)
    return np.broadcast_to((si >= 0) & (si < int(si.max())), ec.dense(c)["attn"].shape)


def skipping_zero_counts(c):
    """The case as a kernel sees it whose level lookup SKIPS levels without samples: the k-th non-empty run of samples is
    read as level k's.  (CPU only: the C ABI refuses a count of 0, so no kernel is ever handed such a list.)"""
    counts = [n for n in c["counts"] if n > 0]
    return dict(c, counts=counts + [0] * (len(c["counts"]) - len(counts)))


ZERO_COUNTS = [0, 3, 0, 0, 2, 4, 0, 1, 0]  # zero-count levels at the front, in the middle and at the end


def zero_count_case():
    rng = np.random.default_rng(7)
    return ec.exact_case(rng, 2, 5, 2, 8, pyramid(len(ZERO_COUNTS)), ZERO_COUNTS, **_KW)
