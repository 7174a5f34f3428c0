"""The argument-error contract of every entry-point family (include/msda_hip.h), one table row per rule.

Every family in ``_lib.EXPORTED_SYMBOLS`` — plain, ``_ragged``, ``_discrete``, ``_masked``, ``_fused``, ``_fused_ragged``,
``_fused_levelref``, ``_fused_hfbox``, ``_fused_levelref_masked`` — in both directions and with every suffix it has, is
called through ctypes at B=1, I=4, H=1, D=4, Q=1, L=1, P=1 with dummy, 256-byte aligned HOST addresses as buffers, as
tests/test_size_guards.py does.  Every row must be refused with the status the header gives it, or return 0, BEFORE anything
is launched: a row's safety rests on that refusal, so the module skips itself where a GPU is present (a call that slipped
through would launch on host addresses).  The GPU side of the contract is held by test_gpu_buffer_contract.py and
test_gpu_parity.py.

The expectations are written from include/msda_hip.h and the rule list, not from the launcher.  A refused call leaves a
non-empty, fresh message; keywords are asserted only where the contract names them.  Two readings are written down here:
"every pointer null" (B = 0, Q = 0) means every device BUFFER — the host arrays ``points_per_level`` / ``level_scale`` are
arguments of the call like L, and a null ``value_mask`` is by the header an error "before any other argument is looked
at"; and where two faults with different codes meet, the order is the one the header's status list implies (dimensions and
levels, size limits, null buffers, alignment, then the per-argument rules), with the one direction-dependent case —
``ref_dim`` against a too-large tensor — recorded per direction."""
import ctypes
import re

import pytest
import torch

from msda_triton_amd import _lib

if torch.cuda.is_available():
    pytest.skip("the rows pass host addresses as buffers: safe only where a call that slipped past its guard cannot launch "
                "(the GPU side of the contract: test_gpu_buffer_contract.py, test_gpu_parity.py)", allow_module_level=True)

BAD_ARG, TOO_MANY_LEVELS, TOO_LARGE, MISALIGNED = -1, -2, -3, -4  # include/msda_hip.h
MAX_LEVELS = 32

# suffix -> bytes of (the arithmetic type: points, weights, reference points; the value rows; the module storage: the fused
# families' projection, out and their gradients)
SIZES = {"f32": (4, 4, 4), "f16": (2, 2, 2), "bf16": (2, 2, 2), "f64": (8, 8, 8), "f32_vbf16": (4, 2, 4),
         "f32_vf16": (4, 2, 4), "f32_sbf16": (4, 2, 2), "f32_sf16": (4, 2, 2)}
KINDS = ("plain", "ragged", "discrete", "masked", "fused", "fused_ragged", "fused_levelref", "fused_hfbox",
         "fused_levelref_masked")
FAMILIES = [(d, k) for k in KINDS for d in ("fwd", "bwd")]
DIMS = dict(B=1, I=4, H=1, D=4, Q=1, L=1, P=1)


def _fused(kind):
    return kind.startswith("fused")


def _counts(kind):
    return kind in ("ragged", "discrete", "fused_ragged", "fused_hfbox")


def _suffixes(kind):
    return _lib.DTYPE_SUFFIXES + (_lib.FUSED_STORAGE_SUFFIXES if _fused(kind) else ())


def _symbol(direction, kind, suffix):
    return f"msda_{direction}_{suffix}" if kind == "plain" else f"msda_{direction}_{kind}_{suffix}"


def _spec(direction, kind):
    """The family's C argument list (include/msda_hip.h), as names."""
    pts, aux = ("proj", "ref") if _fused(kind) else ("loc", "attn")
    names = (["grad_out"] if direction == "bwd" else []) + ["value"]
    names += (["value_mask"] if kind.endswith("masked") else []) + ["shapes", pts, aux]
    if direction == "fwd":
        names.append("out")
    else:
        names.append("grad_value")
        if kind != "discrete":
            names.append("grad_proj" if _fused(kind) else "grad_loc")
        names.append("grad_ref" if _fused(kind) else "grad_attn")
    names += list("BIHDQL") + (["ppl"] if _counts(kind) else ["P"])
    names += ["level_scale", "offset_scale"] if kind == "fused_hfbox" else []
    names += ["ref_dim"] if _fused(kind) else []
    names += ["padding", "align"] if kind != "discrete" else []
    names += ["mlc"] if direction == "bwd" else []
    names.append("stride")
    names += ["ws", "wsb"] if direction == "bwd" else []
    return names + ["stream"]


BUFFERS = ("grad_out", "value", "value_mask", "shapes", "loc", "attn", "proj", "ref", "out", "grad_value", "grad_loc",
           "grad_attn", "grad_proj", "grad_ref")


def _inputs(direction, kind):
    return [n for n in _spec(direction, kind) if n in ("grad_out", "value", "shapes", "loc", "attn", "proj", "ref")]


def _outputs(direction, kind):
    return [n for n in _spec(direction, kind) if n in ("out", "grad_value", "grad_loc", "grad_attn", "grad_proj", "grad_ref")]


def _mandatory_outputs(direction, kind):
    """What the header lets no call leave out: the forward's out, the fused backward's grad_proj and partials."""
    return [n for n in _outputs(direction, kind) if n in ("out", "grad_proj", "grad_ref")]


def _elem(name, kind, suffix):
    """Bytes of one element of buffer `name`."""
    es, ves, ss = SIZES[suffix]
    if name in ("value", "grad_value"):
        return ves
    if name == "shapes":
        return 8
    if name in ("proj", "grad_proj") or (name in ("out", "grad_out") and _fused(kind)):
        return ss
    return es


class _Host:
    """Dummy buffers: host memory, 256-byte aligned, and the host arrays a call reads."""

    def __init__(self):
        self.buf = ctypes.create_string_buffer(4096 + 256)
        self.p = (ctypes.addressof(self.buf) + 255) // 256 * 256
        self.keep = []

    def array(self, ctype, values):
        a = (ctype * len(values))(*values)
        self.keep.append(a)
        return ctypes.cast(a, ctypes.c_void_p)


def _call(lib, direction, kind, suffix, **over):
    """One call of the family's entry point: valid tiny arguments except what `over` says.  `ppl` / `level_scale` take a
    list (made a host array) or None; a buffer takes an address or None."""
    host = _Host()
    vals = dict(DIMS, offset_scale=0.5, ref_dim=4 if kind == "fused_hfbox" else 2, padding=0, align=0, mlc=0, stride=0,
                ws=None, wsb=0, stream=None)
    vals.update({n: host.p for n in BUFFERS})
    vals.update(over)
    levels = max(int(vals["L"]), 1)
    ppl = over.get("ppl", [1] * levels)
    vals["ppl"] = None if ppl is None else host.array(ctypes.c_int32, ppl)
    scale = over.get("level_scale", [1.0] * levels)
    vals["level_scale"] = None if scale is None else host.array(ctypes.c_float, scale)
    fn = getattr(lib, _symbol(direction, kind, suffix))
    names = _spec(direction, kind)
    assert len(names) == len(fn.argtypes), (direction, kind, suffix)
    return fn(*[vals[n] for n in names])


def _null_buffers(direction, kind):
    """Every device buffer null (the mask stays: without it the call is an error by definition)."""
    return {n: None for n in _spec(direction, kind) if n in BUFFERS and n != "value_mask"}


# ---------------------------------------------------------------------------------------------------------------- rows
# Each row: (direction, kind, suffix) -> list of (label, overrides, status, message keyword or None); [] = not this family.
def row_negative_dimension(direction, kind, suffix):
    dims = "BIHDQL" + ("" if _counts(kind) else "P")
    return [(f"{n}=-1", {n: -1}, BAD_ARG, None) for n in dims]


def row_padding_mode(direction, kind, suffix):
    return [] if kind == "discrete" else [("padding_mode=2", {"padding": 2}, BAD_ARG, None)]


def row_too_many_levels(direction, kind, suffix):
    return [("L=33", {"L": MAX_LEVELS + 1}, TOO_MANY_LEVELS, None)]  # (count families: a 33-entry points_per_level)


def row_null_buffer(direction, kind, suffix):
    word = r"null buffer \(argument \d+\)" if kind == "plain" else None
    return [(f"{n}=NULL", {n: None}, BAD_ARG, word if n in _inputs(direction, kind) or n == "out" else None)
            for n in _inputs(direction, kind) + _mandatory_outputs(direction, kind)]


def row_misaligned(direction, kind, suffix):
    return [(f"{n}+half", {n: ("shift", _elem(n, kind, suffix) // 2)}, MISALIGNED, "misaligned")
            for n in _inputs(direction, kind) + _outputs(direction, kind)]


def row_one_sample_gradient(direction, kind, suffix):
    if direction != "bwd" or _fused(kind) or kind == "discrete":
        return []
    return [("grad_loc only", {"grad_attn": None}, BAD_ARG, None), ("grad_attn only", {"grad_loc": None}, BAD_ARG, None)]


def row_ref_dim(direction, kind, suffix):
    return [("ref_dim=3", {"ref_dim": 3}, BAD_ARG, "ref_dim")] if _fused(kind) else []


def row_fused_workspace(direction, kind, suffix):
    if direction != "bwd" or not _fused(kind):
        return []
    return [("ws=NULL", {"ws": None, "wsb": 1 << 20}, BAD_ARG, None),
            ("ws misaligned", {"ws": ("shift", 128), "wsb": 1 << 20}, BAD_ARG, None),
            ("ws too small", {"ws": ("shift", 0), "wsb": 8}, BAD_ARG, None)]  # (3 elements per sample alone are 12 bytes)


def row_point_counts(direction, kind, suffix):
    if not _counts(kind):
        return []
    return [("points_per_level=NULL", {"ppl": None}, BAD_ARG, None), ("a count of 0", {"ppl": [0]}, BAD_ARG, None)]


def row_box_rule(direction, kind, suffix):
    if kind != "fused_hfbox":
        return []
    return [("ref_dim=2", {"ref_dim": 2}, BAD_ARG, None), ("level_scale=NULL", {"level_scale": None}, BAD_ARG, None)]


def row_null_mask(direction, kind, suffix):
    if not kind.endswith("masked"):
        return []
    others = [{}, {"B": -1}, {"L": MAX_LEVELS + 1}, {"value": ("shift", 1)}, {"shapes": None}, {"I": 1 << 24}]
    return [(f"value_mask=NULL with {o}", dict(o, value_mask=None), BAD_ARG, "value_mask") for o in others]


def row_value_row_stride(direction, kind, suffix):
    ves = SIZES[suffix][1]
    dense = DIMS["H"] * DIMS["D"] * ves
    # (the fused backward asks for its workspace before it reads the stride: without grad_value it needs none)
    base = {"grad_value": None} if direction == "bwd" and _fused(kind) else {}
    return [("negative", dict(base, stride=-dense), BAD_ARG, None),
            ("below the dense row", dict(base, stride=dense - ves), BAD_ARG, None),
            ("no multiple of the element", dict(base, stride=2 * dense + 1), BAD_ARG, None)]


def row_empty_batch(direction, kind, suffix):
    rows = [("B=0, buffers NULL", dict(_null_buffers(direction, kind), B=0), 0, None)]
    if direction == "fwd":
        rows.append(("Q=0, buffers NULL", dict(_null_buffers(direction, kind), Q=0), 0, None))
    return rows


def row_precedence(direction, kind, suffix):
    inp = "value"
    out = {"fwd": "out", "bwd": "grad_ref" if _fused(kind) else "grad_attn"}[direction]
    rows = [("L=33 with I=2^24", {"L": MAX_LEVELS + 1, "I": 1 << 24}, TOO_MANY_LEVELS, None),
            ("too large with a null input", {"I": 1 << 24, inp: None}, TOO_LARGE, None),
            ("null input with a misaligned output", {inp: None, out: ("shift", _elem(out, kind, suffix) // 2)}, BAD_ARG, None),
            ("misaligned with a bad stride", {inp: ("shift", _elem(inp, kind, suffix) // 2), "stride": -16}, MISALIGNED,
             "misaligned")]
    if _fused(kind):
        # As the parent answers: the fused forwards test ref_dim before the common check, the fused backwards run the common
        # check first; the box rule's own ref_dim test (ref_dim must be 4) stands in front of both directions.
        first = BAD_ARG if direction == "fwd" or kind == "fused_hfbox" else TOO_LARGE
        rows.append(("ref_dim=3 with I=2^24", {"ref_dim": 3, "I": 1 << 24}, first, "ref_dim" if first == BAD_ARG else None))
    return rows


ROWS = {f.__name__[4:]: f for f in (row_negative_dimension, row_padding_mode, row_too_many_levels, row_null_buffer,
                                    row_misaligned, row_one_sample_gradient, row_ref_dim, row_fused_workspace,
                                    row_point_counts, row_box_rule, row_null_mask, row_value_row_stride, row_empty_batch,
                                    row_precedence)}


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_the_families_are_the_exported_entry_points():
    mine = {_symbol(d, k, s) for d, k in FAMILIES for s in _suffixes(k)}
    entry = {s for s in _lib.EXPORTED_SYMBOLS if re.match(r"msda_(fwd|bwd)_", s) and not s.endswith(("_bytes", "_supported"))}
    assert mine == entry
    assert set(SIZES) == set(_lib.DTYPE_SUFFIXES + _lib.FUSED_STORAGE_SUFFIXES)


@pytest.mark.parametrize("row,direction,kind", [(r, d, k) for r in ROWS for d, k in FAMILIES if ROWS[r](d, k, "f32")])
def test_row_is_answered_before_anything_is_launched(lib, row, direction, kind):
    for suffix in _suffixes(kind):
        cases = ROWS[row](direction, kind, suffix)
        assert cases
        for label, over, want, word in cases:
            assert lib.msda_get_option(b"no such option") == -1  # (leaves its own text behind: the next one is this call's)
            stale = lib.msda_last_error()
            rc = _call_resolved(lib, direction, kind, suffix, over)
            msg = lib.msda_last_error()
            where = (row, label, direction, kind, suffix, rc, msg)
            assert rc == want, where
            if want != 0:
                assert msg and msg != stale, where
                if word is not None:
                    assert re.search(word, msg.decode()), where


def _call_resolved(lib, direction, kind, suffix, over):
    """`("shift", n)` in a row stands for "the call's aligned dummy address plus n bytes"."""
    probe = _Host()  # (backs the shifted pointers for the length of the call; nothing reads it)
    fixed = {k: (probe.p + v[1] if isinstance(v, tuple) and v[0] == "shift" else v) for k, v in over.items()}
    return _call(lib, direction, kind, suffix, **fixed)


# ------------------------------------------------------------------------------------------------- workspace queries
def _queries(lib, B, I, H, D, Q, L, P, es, ves, flags=0):  # noqa: E741
    """Every workspace query (uniform P, or P points on each of L levels): name -> bytes."""
    host = _Host()
    cp = host.array(ctypes.c_int32, [P] * max(L, 1))
    return {
        "msda_bwd_workspace_bytes": lib.msda_bwd_workspace_bytes(B, I, H, D, Q, L, P, es, ves, 0, flags),
        "msda_bwd_fused_workspace_bytes": lib.msda_bwd_fused_workspace_bytes(B, I, H, D, Q, L, P, es, ves, 0, flags),
        "msda_bwd_ragged_workspace_bytes": lib.msda_bwd_ragged_workspace_bytes(B, I, H, D, Q, L, cp, es, ves, 0, flags),
        "msda_bwd_discrete_workspace_bytes": lib.msda_bwd_discrete_workspace_bytes(B, I, H, D, Q, L, cp, es, ves, 0, flags),
        "msda_bwd_fused_ragged_workspace_bytes": lib.msda_bwd_fused_ragged_workspace_bytes(B, I, H, D, Q, L, cp, es, ves,
                                                                                           0, flags),
    }


WS_SHAPE = dict(B=4, I=1344, H=4, D=32, Q=6000, L=1, P=8)  # beyond the single-launch kernel: every query is positive
WS_SIZES = ((4, 4), (2, 2), (8, 8), (4, 2))


def test_workspace_queries_answer_0_for_a_negative_dimension(lib):
    for es, ves in WS_SIZES:
        assert all(v > 0 for v in _queries(lib, **WS_SHAPE, es=es, ves=ves).values())
        for n in "BIHDQLP":
            got = _queries(lib, **dict(WS_SHAPE, **{n: -1}), es=es, ves=ves)
            assert all(v == 0 for v in got.values()), (n, es, got)  # (P = -1: a count below 1 in the per-level queries)


def test_workspace_queries_answer_0_for_elem_size_0(lib):
    got = _queries(lib, **WS_SHAPE, es=0, ves=0)
    assert all(v == 0 for v in got.values()), got


def test_two_passes_need_no_more_than_one_and_no_less_than_half_the_batch(lib):
    keep = lib.msda_get_option(b"ws_passes")
    try:
        assert lib.msda_set_option(b"ws_passes", 1) == 0
        for es, ves in WS_SIZES:
            one = _queries(lib, **WS_SHAPE, es=es, ves=ves, flags=_lib.ws_passes(1))
            half = _queries(lib, **dict(WS_SHAPE, B=2), es=es, ves=ves, flags=_lib.ws_passes(1))
            two = _queries(lib, **WS_SHAPE, es=es, ves=ves, flags=_lib.ws_passes(2))
            for name in one:
                assert 0 < half[name] <= two[name] <= one[name], (name, es, half[name], two[name], one[name])
    finally:
        lib.msda_set_option(b"ws_passes", keep)
