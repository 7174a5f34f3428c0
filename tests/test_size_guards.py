"""Every size inequality that makes the 32-bit plane offsets safe ("Size limits"), held at its limit.

The kernels address a (batch, head) plane with a 64-bit base and 32-bit offsets inside it; the launcher's guards are what
make that safe.  This file calls the library through ctypes with dummy, aligned HOST addresses as pointers: the limits
are applied before a pointer is looked at and nothing is launched (a call that got past its guard would fail to launch,
not pass).  One table row per inequality; the limits are written from DESIGN.md §2 / include/msda_hip.h, in Python
integers, never from the code under test.

Per row: the smallest dimensions that land on the limit, every OTHER term of the same check strictly inside its own
limit (asserted: the row exercises its own guard), status MSDA_ERR_TOO_LARGE (-3) with a message, for every entry-point
family the guard applies to and every element size.  Which size a limit uses: every term of the common check takes the
size of the ARITHMETIC / sampling type (4 for every f32_* suffix, whatever the 16-bit storage of value or projection);
the row stride is a byte count and its lower bound H * D * sizeof takes the VALUE type.

Three terms cannot be isolated, and the table says so (`implied`): B >= 2^31 implies B * H >= 2^28 whenever H >= 1
(the backward checks before its empty-problem shortcut, so H = 0 isolates it there), Q >= 2^31 implies Q >= 2^24, and
Q * H * S * 3 >= 2^31 cannot be met with equality (2^31 is no multiple of 3), so `>=` and `>` are the same guard there."""
import ctypes

import pytest

from msda_triton_amd import _lib

TOO_LARGE = -3
L31, L28, L24, L22 = 1 << 31, 1 << 28, 1 << 24, 1 << 22

# suffix -> (size of the arithmetic / sampling type, size of the value type)
SIZES = {"f32": (4, 4), "f16": (2, 2), "bf16": (2, 2), "f64": (8, 8), "f32_vbf16": (4, 2), "f32_vf16": (4, 2),
         "f32_sbf16": (4, 2), "f32_sf16": (4, 2)}
PLAIN = _lib.DTYPE_SUFFIXES
FUSED = _lib.DTYPE_SUFFIXES + _lib.FUSED_STORAGE_SUFFIXES
# family -> (entry-point name pattern, suffixes, is a backward, is fused)
FAMILIES = {
    "fwd": ("msda_fwd_{}", PLAIN, False, False),
    "bwd": ("msda_bwd_{}", PLAIN, True, False),
    "fwd_ragged": ("msda_fwd_ragged_{}", PLAIN, False, False),
    "bwd_ragged": ("msda_bwd_ragged_{}", PLAIN, True, False),
    "fwd_discrete": ("msda_fwd_discrete_{}", PLAIN, False, False),
    "bwd_discrete": ("msda_bwd_discrete_{}", PLAIN, True, False),
    "fwd_fused": ("msda_fwd_fused_{}", FUSED, False, True),
    "bwd_fused": ("msda_bwd_fused_{}", FUSED, True, True),
    "fwd_fused_ragged": ("msda_fwd_fused_ragged_{}", FUSED, False, True),
    "bwd_fused_ragged": ("msda_bwd_fused_ragged_{}", FUSED, True, True),
}


def common_terms(d, es):
    """The common check's terms: name -> (left-hand side, limit).  `es`: the arithmetic type's size."""
    B, I, H, D, Q, S = (d[k] for k in "BIHDQS")  # noqa: E741
    return {
        "I*H*D*sizeof": (I * H * D * es, L31), "B": (B, L31), "Q": (Q, L31), "S": (S, L22), "B*H": (B * H, L28),
        "Q*H*S*2": (Q * H * S * 2, L31), "Q*H*D*sizeof": (Q * H * D * es, L31), "I>=2^24": (I, L24), "Q>=2^24": (Q, L24),
        "H*S": (H * S, L24), "H*D*sizeof": (H * D * es, L24),
    }


def later_terms(d, es, ves):
    """The checks behind the common one, in the order the entry points apply them: the fused projection (fused families
    only), then the row stride (0 = dense: H * D * sizeof(value type))."""
    row = d["stride"] if d["stride"] else d["H"] * d["D"] * ves
    return {"Q*H*S*3": (d["Q"] * d["H"] * d["S"] * 3, L31), "I*stride": (d["I"] * row, L31), "stride>=2^24": (row, L24)}


def _dims(B=1, I=1, H=1, D=1, Q=1, S=1, stride=0):  # noqa: E741
    return dict(B=B, I=I, H=H, D=D, Q=Q, S=S, stride=stride)


def _fused_qs():
    """The smallest Q * S with Q * S * 3 >= 2^31 under Q < 2^24, S < 2^22 (H = 1): (Q, S)."""
    need = -(-L31 // 3)
    best = min(((-(-need // s)) * s, -(-need // s), s) for s in range(64, 4096))
    assert best[1] < L24
    return best[1], best[2]


FQ, FS = _fused_qs()

# name -> (stage, own term, dims as a function of (es, ves), terms the own one necessarily implies, families or None = all)
ROWS = {
    "value_plane_bytes": ("common", "I*H*D*sizeof", lambda es, ves: _dims(I=1 << 23, D=256 // es), (), None),
    "batch": ("common", "B", lambda es, ves: _dims(B=L31), ("B*H",), None),
    "batch_alone": ("common", "B", lambda es, ves: _dims(B=L31, H=0), (), "backward"),
    "queries_31": ("common", "Q", lambda es, ves: _dims(Q=L31, H=0), ("Q>=2^24",), "backward"),
    "queries_31_fwd": ("common", "Q", lambda es, ves: _dims(Q=L31), ("Q>=2^24", "Q*H*S*2", "Q*H*D*sizeof"), None),
    "samples_per_unit": ("common", "S", lambda es, ves: _dims(S=L22), (), None),
    "planes": ("common", "B*H", lambda es, ves: _dims(B=L28), (), None),
    "sample_offsets": ("common", "Q*H*S*2", lambda es, ves: _dims(Q=1 << 10, S=1 << 20), (), None),
    "row_offsets": ("common", "Q*H*D*sizeof", lambda es, ves: _dims(Q=1 << 23, D=256 // es), (), None),
    "pixels_24": ("common", "I>=2^24", lambda es, ves: _dims(I=L24), (), None),
    "queries_24": ("common", "Q>=2^24", lambda es, ves: _dims(Q=L24), (), None),
    "head_samples": ("common", "H*S", lambda es, ves: _dims(H=8, S=1 << 21), (), None),
    "pixel_bytes": ("common", "H*D*sizeof", lambda es, ves: _dims(D=L24 // es), (), None),
    "fused_projection": ("fused", "Q*H*S*3", lambda es, ves: _dims(Q=FQ, S=FS), (), "fused"),
    "plane_stride": ("stride", "I*stride", lambda es, ves: _dims(I=1 << 23, stride=256), (), None),
    "row_stride_24": ("stride", "stride>=2^24", lambda es, ves: _dims(stride=L24), (), None),
}
STAGES = ("common", "fused", "stride")


def _applies(row, family):
    _, _, backward, fused = FAMILIES[family]
    where = ROWS[row][4]
    return where is None or (where == "backward" and backward) or (where == "fused" and fused)


def _isolates(row, family, es, ves):
    """Asserts that the row's dimensions violate its own term (and what that implies) and nothing else that the entry
    point checks at or before the row's stage; returns the dimensions."""
    stage, own, make, implied, _ = ROWS[row]
    d = make(es, ves)
    terms = dict(common_terms(d, es))
    later = later_terms(d, es, ves)
    fused = FAMILIES[family][3]
    if stage in ("fused", "stride") and fused:
        terms["Q*H*S*3"] = later["Q*H*S*3"]
    if stage == "stride":
        terms["I*stride"], terms["stride>=2^24"] = later["I*stride"], later["stride>=2^24"]
    hit = {k for k, (lhs, lim) in terms.items() if lhs >= lim}
    assert own in hit, (row, family, es, "the row does not reach its own limit")
    assert hit - {own} == set(implied), (row, family, es, hit)
    lhs, lim = terms[own]
    if own != "Q*H*S*3":
        assert lhs == lim, (row, "the dimensions do not land exactly on the limit", lhs, lim)
    else:  # (2^31 is no multiple of 3: one query fewer is inside)
        assert (d["Q"] - 1) * d["H"] * d["S"] * 3 < lim <= lhs
    if d["stride"]:
        assert d["stride"] % ves == 0 and d["stride"] >= d["H"] * d["D"] * ves  # a stride the call would otherwise take
    return d


class _Host:
    """A dummy pointer: host memory, 256-byte aligned.  No guard looks behind it."""

    def __init__(self):
        self.buf = ctypes.create_string_buffer(4096 + 256)
        self.p = (ctypes.addressof(self.buf) + 255) // 256 * 256
        self.counts = None


def _call(lib, host, family, suffix, d, want_value=True):
    pattern, _, backward, fused = FAMILIES[family]
    fn = getattr(lib, pattern.format(suffix))
    p = host.p
    B, I, H, D, Q, S, stride = (d[k] for k in ("B", "I", "H", "D", "Q", "S", "stride"))  # noqa: E741
    ragged = family.endswith(("ragged", "discrete"))
    if ragged:
        host.counts = (ctypes.c_int32 * 1)(S)
        pts = (1, ctypes.cast(host.counts, ctypes.c_void_p))  # L = 1, points_per_level = [S]
    else:
        pts = (1, S)                                            # L = 1, P = S
    sizes = (B, I, H, D, Q) + pts
    gv = p if want_value and not fused else None  # (the fused backward asks for its workspace before it reads the stride)
    if family == "fwd_discrete":
        return fn(p, p, p, p, p, *sizes, stride, None)
    if family == "bwd_discrete":
        return fn(p, p, p, p, p, gv, p, *sizes, 0, stride, None, 0, None)
    if not backward:
        return fn(p, p, p, p, p, *sizes, 2, 0, 0, stride, None) if fused else fn(p, p, p, p, p, *sizes, 0, 0, stride, None)
    if fused:
        return fn(p, p, p, p, p, gv, p, p, *sizes, 2, 0, 0, 0, stride, None, 0, None)
    return fn(p, p, p, p, p, gv, p, p, *sizes, 0, 0, 0, stride, None, 0, None)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_the_table_covers_every_term():
    own = {r[1] for r in ROWS.values()}
    assert own == set(common_terms(_dims(), 4)) | set(later_terms(_dims(), 4, 4))
    for family in FAMILIES:
        assert any(_applies(row, family) for row in ROWS)
    assert {s for s in SIZES if SIZES[s][0] == 2} and {s for s in SIZES if SIZES[s][0] == 8}  # sizes 2, 4 and 8 are there
    assert set(SIZES) == set(FUSED)


@pytest.mark.parametrize("row,family,suffix", [(r, f, s) for r in ROWS for f in FAMILIES if _applies(r, f)
                                               for s in FAMILIES[f][1]])
def test_guard_at_its_limit_is_refused(lib, row, family, suffix):
    host = _Host()
    es, ves = SIZES[suffix]
    d = _isolates(row, family, es, ves)
    assert lib.msda_get_option(b"no such option") == -1  # (leaves its own text behind: the next one is this call's)
    stale = lib.msda_last_error()
    rc = _call(lib, host, family, suffix, d)
    msg = lib.msda_last_error()
    assert rc == TOO_LARGE, (row, family, suffix, d, rc, msg)
    assert msg and msg != stale, (row, family, suffix, msg)


# ------------------------------------------------------------------------------------------------- workspace queries
def _queries(lib, d, es, ves, flags=0):
    """Every workspace query at these dimensions (L = 1): name -> bytes."""
    B, I, H, D, Q, S = (d[k] for k in "BIHDQS")  # noqa: E741
    counts = (ctypes.c_int32 * 1)(S)
    cp = ctypes.cast(counts, ctypes.c_void_p)
    return {
        "msda_bwd_workspace_bytes": lib.msda_bwd_workspace_bytes(B, I, H, D, Q, 1, S, es, ves, 0, flags),
        "msda_bwd_fused_workspace_bytes": lib.msda_bwd_fused_workspace_bytes(B, I, H, D, Q, 1, S, es, ves, 0, flags),
        "msda_bwd_ragged_workspace_bytes": lib.msda_bwd_ragged_workspace_bytes(B, I, H, D, Q, 1, cp, es, ves, 0, flags),
        "msda_bwd_discrete_workspace_bytes": lib.msda_bwd_discrete_workspace_bytes(B, I, H, D, Q, 1, cp, es, ves, 0, flags),
        "msda_bwd_fused_ragged_workspace_bytes": lib.msda_bwd_fused_ragged_workspace_bytes(B, I, H, D, Q, 1, cp, es, ves,
                                                                                           0, flags),
    }


def _fused_points(d, es):
    """The fused queries' own part (include/msda_hip.h): the derived sampling points and attention weights, 3 elements
    per sample, rounded up to 256 bytes — float32 elements for a 2-byte call: the 16-bit operators park them in float."""
    return -(-(d["B"] * d["Q"] * d["H"] * d["S"] * 3 * max(es, 4)) // 256) * 256


def _sorted_part(name, got, d, es):
    """A query's answer without the fused part: what the grad_value pipeline gets."""
    if "fused" not in name:
        return got
    assert got >= _fused_points(d, es), (name, got, d)
    return got - _fused_points(d, es)


def _partial_rows(d, es):
    """What every sorted-pipeline workspace holds whatever its rounds and slices (`scratch[pixel][corner]`):
    four partial rows of the accumulate type per pixel and plane."""
    return d["B"] * d["H"] * d["I"] * 4 * d["D"] * (8 if es == 8 else 4)


@pytest.mark.parametrize("row", [r for r in ROWS if ROWS[r][0] != "stride"])  # (the queries take no stride)
def test_workspace_queries_answer_0_where_the_call_is_refused(lib, row):
    """Dimensions a call refuses with MSDA_ERR_TOO_LARGE have no workspace to size: every query says 0 (include/msda_hip.h),
    never a product that wrapped.  The fused projection's own limit binds the two fused queries only."""
    for es, ves in ((4, 4), (2, 2), (8, 8), (4, 2)):
        d = ROWS[row][2](es, ves)
        for name, got in _queries(lib, d, es, ves).items():
            if ROWS[row][0] == "fused" and "fused" not in name:
                continue
            assert got == 0, (row, name, es, d, got)


def test_workspace_queries_answer_0_where_grad_value_is_unsupported(lib):
    """A plane of 2^22 pixels: the forward and the sample gradients run, grad_value does not (msda_bwd_supported says 0,
    the call MSDA_ERR_UNSUPPORTED), so there is no workspace to size either."""
    for es, ves in ((4, 4), (2, 2), (8, 8), (4, 2)):
        d = _dims(B=2, I=L22, H=2, D=8, Q=8192, S=4)
        assert lib.msda_bwd_supported(2, L22, 2, 8, 8192, 1, 4, es) == 0
        for name, got in _queries(lib, d, es, ves).items():
            assert _sorted_part(name, got, d, es) == 0, (name, es, got)


def test_workspace_query_at_the_largest_supported_plane(lib):
    """I = 2^22 - 1 pixels: the last plane the sorted records' pixel field can name."""
    for es, ves, D in ((4, 4, 16), (2, 2, 16), (8, 8, 8), (4, 2, 16)):
        acc = 8 if es == 8 else 4
        d = _dims(B=2, I=L22 - 1, H=2, D=D, Q=8192, S=4)
        assert d["I"] * 4 * D * acc < L31  # (its partial rows stay inside the 32-bit slot offsets)
        assert lib.msda_bwd_supported(2, d["I"], 2, D, 8192, 1, 4, es) == 1
        records = d["B"] * d["H"] * d["Q"] * d["S"] * (32 if es == 8 else 16)  # one round: far below its 1 GiB budget
        for name, got in _queries(lib, d, es, ves).items():
            rest = _sorted_part(name, got, d, es)
            assert rest == 0 or rest >= records + _partial_rows(d, es), (name, es, got)
            assert rest > 0, (name, es)  # 8192 queries are beyond the single-launch kernel


def test_workspace_grows_with_the_batch_in_one_pass(lib):
    keep = lib.msda_get_option(b"ws_passes")
    try:
        assert lib.msda_set_option(b"ws_passes", 1) == 0
        for es, ves in ((4, 4), (2, 2), (8, 8), (4, 2)):
            last = None
            for B in (1, 2, 3, 4, 5, 8, 9):
                got = _queries(lib, _dims(B=B, I=1344, H=4, D=32, Q=6000, S=8), es, ves, flags=_lib.ws_passes(1))
                assert all(v > 0 for v in got.values()), (B, es, got)
                if last is not None:
                    assert all(got[k] > last[k] for k in got), (B, es, got, last)
                last = got
    finally:
        lib.msda_set_option(b"ws_passes", keep)
