"""CPU: both padding masks inside the nn.Module's fused kernels — the C ABI of the two new families
(msda_{fwd,bwd}_fused_masked_<suffix>, msda_{fwd,bwd}_fused_ragged_masked_<suffix>) and the host-tensor definition.

The symbol table, the header and the ctypes signatures are compared with the unmasked twins; the argument-error table is
written in the style of tests/test_entry_point_contract.py (dummy 256-byte aligned HOST addresses at B=1, I=4, H=1, D=4, Q=1,
L=1, P=1: every row must be answered before anything is launched, so those tests skip themselves where a GPU is present); on
host tensors the cores and the module compose the masks, and the definition is held against the unmasked route."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from msda_triton_amd import _lib, functional, module as msda_module, ragged
from msda_triton_amd.functional import apply_query_mask, fused_module_core
from msda_triton_amd.module import MultiscaleDeformableAttention

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUFFIXES = _lib.DTYPE_SUFFIXES + _lib.FUSED_STORAGE_SUFFIXES
KINDS = ("fused_masked", "fused_ragged_masked")
TWIN = {"fused_masked": "fused", "fused_ragged_masked": "fused_ragged"}
BAD_ARG, TOO_MANY_LEVELS, TOO_LARGE, MISALIGNED, UNSUPPORTED = -1, -2, -3, -4, -5
SIZES = {"f32": (4, 4, 4), "f16": (2, 2, 2), "bf16": (2, 2, 2), "f64": (8, 8, 8), "f32_vbf16": (4, 2, 4),
         "f32_vf16": (4, 2, 4), "f32_sbf16": (4, 2, 2), "f32_sf16": (4, 2, 2)}


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ------------------------------------------------------------------------------------------------ symbols and lists
def test_the_symbol_table():
    want = {f"msda_{d}_{k}_{s}" for d in ("fwd", "bwd") for k in KINDS for s in SUFFIXES}
    assert len(_lib.MODULE_MASK_SYMBOLS) == 32 and set(_lib.MODULE_MASK_SYMBOLS) == want
    assert not set(_lib.MODULE_MASK_SYMBOLS) & set(_lib.EXPORTED_SYMBOLS)
    assert not set(_lib.MODULE_MASK_SYMBOLS) & set(_lib.QUERY_MASK_SYMBOLS + _lib.HFBOX_DISCRETE_SYMBOLS)


def test_every_symbol_is_exported_by_the_built_library(lib):
    assert _lib.has_module_masks()
    for s in _lib.MODULE_MASK_SYMBOLS:
        assert hasattr(lib, s), s
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    defined = set(re.findall(r" T (msda_\w+)", nm))
    assert set(_lib.MODULE_MASK_SYMBOLS) <= defined


def _header():
    with open(os.path.join(ROOT, "include", "msda_hip.h")) as f:
        return f.read().replace("\\\n", " ")


def _macro_decls(text, macro):
    """{family: [parameter names]} of the declarations inside `#define <macro>(SUF) ...`."""
    body = re.search(r"#define " + macro + r"\(SUF\)(.*)", text).group(1)
    out = {}
    for name, params in re.findall(r"int msda_(\w+)_##SUF\(([^)]*)\)", body):
        out[name] = [re.sub(r"\s+", " ", p).strip() for p in params.split(",")]
    return out


def test_the_header_declares_them_through_a_macro_of_its_own():
    text = _header()
    decl = _macro_decls(text, "MSDA_MODULE_MASK")
    assert set(decl) == {f"{d}_{k}" for d in ("fwd", "bwd") for k in KINDS}
    used = re.findall(r"MSDA_MODULE_MASK\((\w+)\)", text)
    assert sorted(s for s in used if s != "SUF") == sorted(SUFFIXES)
    for name, body in re.findall(r"#define (MSDA_DECLARE\w*)\(SUF\)(.*)", text):  # (those macros are EXPORTED_SYMBOLS')
        assert "fused_masked_##SUF" not in body and "fused_ragged_masked_##SUF" not in body, name
    # each list is the twin's with `value_mask`, `query_mask` directly behind `value`
    twins = _macro_decls(text, "MSDA_DECLARE_FUSED_STORAGE")
    for d in ("fwd", "bwd"):
        for k in KINDS:
            mine, twin = decl[f"{d}_{k}"], twins[f"{d}_{TWIN[k]}"]
            at = twin.index("const void *value") + 1
            assert mine == twin[:at] + ["const uint8_t *value_mask", "const uint8_t *query_mask"] + twin[at:], (d, k)


def test_each_ctypes_list_is_the_twins_plus_two_pointers(lib):
    for d in ("fwd", "bwd"):
        for k in KINDS:
            for s in SUFFIXES:
                mine = getattr(lib, f"msda_{d}_{k}_{s}").argtypes
                twin = getattr(lib, f"msda_{d}_{TWIN[k]}_{s}").argtypes
                at = 1 if d == "fwd" else 2
                assert list(mine) == list(twin[:at]) + [ctypes.c_void_p] * 2 + list(twin[at:]), (d, k, s)


# ---------------------------------------------------------------------------------------------- argument-error table
no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="the rows pass host addresses as buffers: safe only where a "
                            "call that slipped past its guard cannot launch (the GPU side: test_gpu_module_masks.py)")
DIMS = dict(B=1, I=4, H=1, D=4, Q=1, L=1, P=1)
BUFFERS = ("grad_out", "value", "value_mask", "query_mask", "shapes", "proj", "ref", "out", "grad_value", "grad_proj", "grad_ref")


def _spec(direction, kind):
    names = (["grad_out"] if direction == "bwd" else []) + ["value", "value_mask", "query_mask", "shapes", "proj", "ref"]
    names += ["out"] if direction == "fwd" else ["grad_value", "grad_proj", "grad_ref"]
    names += list("BIHDQL") + (["ppl"] if kind == "fused_ragged_masked" else ["P"]) + ["ref_dim", "padding", "align"]
    names += ["mlc"] if direction == "bwd" else []
    names.append("stride")
    names += ["ws", "wsb"] if direction == "bwd" else []
    return names + ["stream"]


def _elem(name, suffix):
    es, ves, ss = SIZES[suffix]
    if name in ("value", "grad_value"):
        return ves
    if name == "shapes":
        return 8
    return ss if name in ("proj", "grad_proj", "out", "grad_out") else es


def _call(lib, direction, kind, suffix, **over):
    buf = ctypes.create_string_buffer(4096 + 512)
    p = (ctypes.addressof(buf) + 255) // 256 * 256
    vals = dict(DIMS, ref_dim=2, padding=0, align=0, mlc=0, stride=0, ws=None, wsb=0, stream=None)
    vals.update({n: p for n in BUFFERS})
    vals.update({k: (p + v[1] if isinstance(v, tuple) else v) for k, v in over.items()})
    ppl = over.get("ppl", [1] * max(int(vals["L"]), 1))
    arr = None if ppl is None else (ctypes.c_int32 * len(ppl))(*ppl)
    vals["ppl"] = None if arr is None else ctypes.cast(arr, ctypes.c_void_p)
    fn = getattr(lib, f"msda_{direction}_{kind}_{suffix}")
    names = _spec(direction, kind)
    assert len(names) == len(fn.argtypes)
    rc = fn(*[vals[n] for n in names])
    del buf, arr
    return rc


def _inputs(direction):
    return (["grad_out"] if direction == "bwd" else []) + ["value", "shapes", "proj", "ref"]


def _outputs(direction):
    return ["out"] if direction == "fwd" else ["grad_value", "grad_proj", "grad_ref"]


def _rows(direction, kind, suffix):
    """(label, overrides, status, message keyword or None)"""
    counts = kind == "fused_ragged_masked"
    rows = []
    # a NULL value_mask wins over every other fault; a NULL query_mask is accepted (here: an empty call returns 0)
    for o in ({}, {"B": -1}, {"L": 33}, {"value": ("shift", 1)}, {"shapes": None}, {"I": 1 << 24}, {"ref_dim": 3},
              {"query_mask": None}) + (({"ppl": [0]}, {"ppl": None}, {"L": 9, "ppl": [1] * 9}) if counts else ()):
        rows.append((f"value_mask=NULL with {o}", dict(o, value_mask=None), BAD_ARG, "value_mask"))
    nulls = {n: None for n in _spec(direction, kind) if n in BUFFERS and n != "value_mask"}
    rows.append(("B=0, buffers NULL", dict(nulls, B=0), 0, None))
    if direction == "fwd":
        rows.append(("Q=0, buffers NULL", dict(nulls, Q=0), 0, None))
    rows.append(("B=0, query_mask NULL", {"B": 0, "query_mask": None}, 0, None))
    for n in "BIHDQL" + ("" if counts else "P"):
        rows.append((f"{n}=-1", {n: -1}, BAD_ARG, None))
    rows.append(("padding_mode=2", {"padding": 2}, BAD_ARG, None))
    rows.append(("L=33", {"L": 33}, TOO_MANY_LEVELS, None))
    rows.append(("ref_dim=3", {"ref_dim": 3}, BAD_ARG, "ref_dim"))
    rows.append(("I too large", {"I": 1 << 24}, TOO_LARGE, None))
    rows.append(("L=33 with I=2^24", {"L": 33, "I": 1 << 24}, TOO_MANY_LEVELS, None))
    rows.append(("too large with a null input", {"I": 1 << 24, "value": None}, TOO_LARGE, None))
    first = BAD_ARG if direction == "fwd" else TOO_LARGE  # (as the twins answer: test_entry_point_contract.row_precedence)
    rows.append(("ref_dim=3 with I=2^24", {"ref_dim": 3, "I": 1 << 24}, first, "ref_dim" if first == BAD_ARG else None))
    for n in _inputs(direction) + [o for o in _outputs(direction) if o != "grad_value"]:
        rows.append((f"{n}=NULL", {n: None}, BAD_ARG, None))
    for n in _inputs(direction) + _outputs(direction):
        rows.append((f"{n}+half", {n: ("shift", _elem(n, suffix) // 2)}, MISALIGNED, "misaligned"))
    rows.append(("null input with a misaligned output", {"value": None, _outputs(direction)[-1]: ("shift", _elem(_outputs(direction)[-1], suffix) // 2)},
                 BAD_ARG, None))
    rows.append(("misaligned with a bad stride", {"value": ("shift", _elem("value", suffix) // 2), "stride": -16}, MISALIGNED, "misaligned"))
    if direction == "bwd":
        rows += [("ws=NULL", {"ws": None, "wsb": 1 << 20}, BAD_ARG, None),
                 ("ws misaligned", {"ws": ("shift", 128), "wsb": 1 << 20}, BAD_ARG, None),
                 ("ws too small", {"ws": ("shift", 0), "wsb": 8}, BAD_ARG, None)]
    dense = DIMS["H"] * DIMS["D"] * SIZES[suffix][1]
    base = {"grad_value": None} if direction == "bwd" else {}
    rows += [("stride negative", dict(base, stride=-dense), BAD_ARG, None),
             ("stride below the dense row", dict(base, stride=dense - SIZES[suffix][1]), BAD_ARG, None),
             ("stride no multiple of the element", dict(base, stride=2 * dense + 1), BAD_ARG, None)]
    if counts:
        rows += [("points_per_level=NULL", {"ppl": None}, BAD_ARG, None), ("a count of 0", {"ppl": [0]}, BAD_ARG, None),
                 ("L=9", dict(base, L=9, ppl=[1] * 9), UNSUPPORTED, None)]
    return rows


@no_gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("direction", ["fwd", "bwd"])
def test_argument_errors_are_answered_before_anything_is_launched(lib, direction, kind):
    for suffix in SUFFIXES:
        for label, over, want, word in _rows(direction, kind, suffix):
            assert lib.msda_get_option(b"no such option") == -1  # (leaves its own text behind: the next one is this call's)
            stale = lib.msda_last_error()
            rc = _call(lib, direction, kind, suffix, **over)
            msg = lib.msda_last_error()
            where = (label, direction, kind, suffix, rc, msg)
            assert rc == want, where
            if want != 0:
                assert msg and msg != stale, where
                if word is not None:
                    assert re.search(word, msg.decode()), where


# ------------------------------------------------------------------------------------------ host tensors: the definition
LEVELS = [(6, 5), (3, 3), (2, 2)]


def _host_inputs(counts, ref_dim, seed, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    B, Q, H, D = 2, 7, 2, 4
    I = sum(h * w for h, w in LEVELS)  # noqa: E741
    value = torch.randn(B, I, H, D, generator=g, dtype=dtype)
    if isinstance(counts, int):
        proj = torch.randn(B, Q, H, len(LEVELS), counts, 3, generator=g, dtype=dtype)
    else:
        proj = torch.randn(B, Q, H, sum(counts), 3, generator=g, dtype=dtype)
    ref = torch.rand(B, Q, ref_dim, generator=g, dtype=dtype)
    vm = torch.rand(B, I, generator=g) < 0.6
    qm = torch.rand(B, Q, generator=g) < 0.7
    qm[0, 0], qm[1, -1] = True, False
    return value, torch.tensor(LEVELS), proj, ref, vm, qm


@pytest.mark.parametrize("in_kernels", [True, False])
@pytest.mark.parametrize("ref_dim", [2, 4])
@pytest.mark.parametrize("counts", [4, (3, 6, 3), (2, 2, 2)], ids=["uniform", "ragged", "equal_counts"])
def test_host_cores_compose_the_masks(counts, ref_dim, in_kernels):
    value, shapes, proj, ref, vm, qm = _host_inputs(counts, ref_dim, 3)
    ppl = None if isinstance(counts, int) else counts
    poisoned = torch.where(vm[:, :, None, None], value, torch.full_like(value, float("nan")))
    nan_rows = ~qm
    proj_p, ref_p = proj.clone(), ref.clone()
    proj_p[nan_rows], ref_p[nan_rows] = float("nan"), float("inf")
    leaves = [t.clone().requires_grad_(True) for t in (poisoned, proj_p, ref_p)]
    got = fused_module_core(leaves[0], shapes, leaves[1], leaves[2], "zeros", False, None, ppl, vm, qm, mask_in_kernels=in_kernels)
    got.sum().backward()
    want_l = [torch.where(vm[:, :, None, None], value, torch.zeros_like(value)).requires_grad_(True),
              apply_query_mask(proj, qm, 0.0).requires_grad_(True), apply_query_mask(ref, qm, 0.5).requires_grad_(True)]
    want = fused_module_core(want_l[0], shapes, want_l[1], want_l[2], "zeros", False, None, ppl)
    want = apply_query_mask(want, qm, 0.0)
    want.sum().backward()
    assert torch.equal(got, want) and not got[nan_rows].any()
    assert torch.equal(leaves[0].grad, torch.where(vm[:, :, None, None], want_l[0].grad, torch.zeros_like(value)))
    for g, w in zip(leaves[1:], want_l[1:]):
        assert torch.equal(g.grad, apply_query_mask(w.grad, qm, 0.0))
    if ppl is not None:  # the ragged function is the same route
        again = ragged.fused_ragged_module_core(poisoned, shapes, proj_p, ref_p, "zeros", False, ppl, None, vm, qm)
        assert torch.equal(again, got.detach())


@pytest.mark.parametrize("num_points", [2, [3, 6, 3]], ids=["int", "per_level"])
def test_host_module_a_masked_query_gets_the_bias(num_points):
    torch.manual_seed(5)
    mod = MultiscaleDeformableAttention(8, 8, len(LEVELS), 2, num_points, "zeros", False).double()
    B, Q = 2, 7
    I = sum(h * w for h, w in LEVELS)  # noqa: E741
    img, queries, ref = torch.randn(B, I, 8).double(), torch.randn(B, Q, 8).double(), torch.rand(B, Q, 4).double()
    shapes = torch.tensor(LEVELS)
    vm, qm = torch.rand(B, I) < 0.6, torch.rand(B, Q) < 0.7
    qm[0, 0], qm[1, -1] = True, False
    img_p, queries_p = img.clone(), queries.clone()
    img_p[~vm], queries_p[~qm] = float("nan"), float("nan")
    keep = msda_module.MASK_IN_KERNELS
    try:
        outs = []
        for switch in (True, False):
            msda_module.MASK_IN_KERNELS = switch
            assert msda_module.mask_in_kernels(img) is False  # host tensors compose either way
            outs.append(mod(img_p, shapes, queries_p, ref, value_mask=vm, query_mask=qm))
    finally:
        msda_module.MASK_IN_KERNELS = keep
    assert torch.equal(outs[0], outs[1]) and torch.isfinite(outs[0]).all()
    bias = mod.query_output_proj.bias.detach()
    assert torch.equal(outs[0][~qm], bias.expand_as(outs[0][~qm]))
    # the unmasked route on where(mask, value, 0): the projected pyramid is what the mask acts on
    B_, I_, _ = img.shape
    value = mod.img_input_proj(img).reshape(B_, I_, 2, 4)
    pts_in = mod.query_input_proj(queries)
    proj = pts_in.reshape(B, Q, 2, len(LEVELS), 2, 3) if isinstance(num_points, int) else pts_in.reshape(B, Q, 2, 12, 3)
    core = fused_module_core(functional.apply_value_mask(value, vm), shapes, proj, ref, "zeros", False, None,
                             None if isinstance(num_points, int) else tuple(num_points))
    want = mod.query_output_proj(core.reshape(B, Q, 8))
    assert torch.equal(outs[0][qm], want[qm])
