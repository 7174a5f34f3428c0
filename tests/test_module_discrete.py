"""CPU: discrete sampling in the nn.Module — `MultiscaleDeformableAttention(sampling_mode="discrete")`,
`fused_module_core(..., sampling_mode="discrete")` and the C ABI of msda_{fwd,bwd}_fused_discrete_<suffix>.

Host tensors take the composition (`module_sampling_inputs` / `ragged_module_sampling_inputs` + the discrete operator), which
is held against a hand-written one; the symbol table, the header and the ctypes lists are compared with the hfbox-discrete
pair's; the argument-error table is tests/test_module_masks.py's (dummy HOST addresses: skipped where a GPU is present);
and the kernels' per-sample rule is restated in numpy fp32 with its mutants.

Mutants on the boundary fixture (tests/test_gpu_hf_box_discrete.boundary_coords on the first three levels of SHAPES["d32"],
with zero offsets for 2-d reference points and zero-size boxes for 4-d ones — there the point IS the reference point).  NONE
of the four changes a pixel on it; each is recorded as such (asserted: no pixel changes), with where it does show:
  * (w, h) instead of (h, w) for ref_dim 2                the offsets are zero, 0 / h == 0 / w.  Changes pixels on the GPU
                                                          tests' random-input fixture.
  * 1 / (2 max P) instead of the level's own count        the box size is zero.  Changes pixels on the random fixture.
  * reciprocal-multiply instead of the division at P = 3  0 * (1 / 6) == 0 / 6.  On the random fixture it changes bits of the
                                                          POINT — which tests/test_gpu_module_discrete.py's parked-point test
                                                          compares bit for bit — but, at one ulp, no pixel in that many samples.
  * a fused multiply-add in `x * w + 0.5`                 separate and fused rounding can part only at the boundary 0.5 | 1 of
                                                          the first pixel (k + 0.5 and k + 1 share a binade for k >= 1) and
                                                          only for a product in (0.5 - 1.5 * 2^-25, 0.5 - 2^-25); the axis
                                                          sizes here (16, 12, 8, 9, 4, 4) put no coordinate there.  The same
                                                          construction on an axis of 19 pixels does (shown below): the mutant
                                                          is real, this fixture does not see it.  `discrete_pixel` itself is
                                                          not touched by these kernels' rule and is held by
                                                          tests/test_discrete_sampling.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from msda_triton_amd import _lib, discrete
from msda_triton_amd.functional import (apply_query_mask, apply_value_mask, fused_module_core, module_sampling_inputs,
                                        multiscale_deformable_attention)
from msda_triton_amd.module import MultiscaleDeformableAttention
from msda_triton_amd.ragged import ragged_module_sampling_inputs
from test_gpu_fused_ragged import SHAPES
from test_gpu_hf_box_discrete import boundary_coords

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUFFIXES = _lib.DTYPE_SUFFIXES + _lib.FUSED_STORAGE_SUFFIXES
BAD_ARG, TOO_MANY_LEVELS, TOO_LARGE, MISALIGNED, UNSUPPORTED = -1, -2, -3, -4, -5
SIZES = {"f32": (4, 4, 4), "f16": (2, 2, 2), "bf16": (2, 2, 2), "f64": (8, 8, 8), "f32_vbf16": (4, 2, 4),
         "f32_vf16": (4, 2, 4), "f32_sbf16": (4, 2, 2), "f32_sf16": (4, 2, 2)}
LEVELS = SHAPES["d5"][4][:3]  # non-square: (6, 4), (3, 2), (2, 5)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ------------------------------------------------------------------------------------------ the module on host tensors
def _module_inputs(ref_dim, seed=0):
    g = torch.Generator().manual_seed(seed)
    B, Q, E = 2, 13, 12
    I = sum(h * w for h, w in LEVELS)  # noqa: E741
    img = torch.randn(B, I, E, generator=g, dtype=torch.float64)
    queries = torch.randn(B, Q, E, generator=g, dtype=torch.float64)
    ref = torch.rand(B, Q, ref_dim, generator=g, dtype=torch.float64)
    vm = torch.rand(B, I, generator=g) < 0.6
    qm = torch.rand(B, Q, generator=g) < 0.7
    qm[0, 0], qm[1, -1] = True, False
    return img, torch.tensor(LEVELS), queries, ref, vm, qm


def _by_hand(m, img, shapes, queries, ref, vm=None, qm=None):
    """the composition, written out: projections, the module's prologue, the discrete operator, the masks around them"""
    B, I, _ = img.shape  # noqa: E741
    N, H = queries.shape[1], m.num_heads
    counts = m.points_per_level
    value = apply_value_mask(m.img_input_proj(img).reshape(B, I, H, m.hidden_dim // H), vm)
    proj = m.query_input_proj(queries)
    ref = apply_query_mask(ref, qm, 0.5)
    if counts is None:
        proj = apply_query_mask(proj.reshape(B, N, H, m.num_levels, m.num_points, 3), qm, 0.0)
        pts, att = module_sampling_inputs(proj, shapes, ref)
    else:
        proj = apply_query_mask(proj.reshape(B, N, H, sum(counts), 3), qm, 0.0)
        pts, att = ragged_module_sampling_inputs(proj, shapes, ref, counts)
    out = multiscale_deformable_attention(value, shapes, pts, att, "border", False, points_per_level=counts,
                                          sampling_mode="discrete")
    return m.query_output_proj(apply_query_mask(out, qm, 0.0).reshape(B, N, m.hidden_dim))


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masks"])
@pytest.mark.parametrize("ref_dim", [2, 4])
@pytest.mark.parametrize("num_points", [4, 3, [3, 6, 3]], ids=["p4", "p3", "3_6_3"])
def test_host_module_is_the_composition(num_points, ref_dim, masked):
    torch.manual_seed(7)
    m = MultiscaleDeformableAttention(12, 15, 3, 3, num_points, "border", False, sampling_mode="discrete").double()
    img, shapes, queries, ref, vm, qm = _module_inputs(ref_dim)
    masks = dict(value_mask=vm, query_mask=qm) if masked else {}
    r1 = ref.clone().requires_grad_(True)
    got = m(img, shapes, queries, r1, **masks)
    gout = torch.randn(got.shape, generator=torch.Generator().manual_seed(1), dtype=got.dtype)
    got.backward(gout)
    grads = {n: p.grad.clone() for n, p in m.named_parameters()}
    assert r1.grad is None or not bool(r1.grad.any())  # (the pixel index is an integer: nothing reaches the reference points)
    m.zero_grad(set_to_none=True)
    want = _by_hand(m, img, shapes, queries, ref, *(vm, qm) if masked else ())
    want.backward(gout)
    torch.testing.assert_close(got, want, atol=1e-12, rtol=1e-12)
    assert set(grads) == {n for n, p in m.named_parameters() if p.grad is not None}
    for n, p in m.named_parameters():
        torch.testing.assert_close(grads[n], p.grad, atol=1e-12, rtol=1e-12, msg=lambda s: f"{n}: {s}")
    # the offset rows of the query projection have exactly zero gradients, the logit rows do not
    S = m.query_input_proj.out_features // (3 * m.num_heads)
    gw = grads["query_input_proj.weight"].reshape(m.num_heads, S, 3, -1)
    gb = grads["query_input_proj.bias"].reshape(m.num_heads, S, 3)
    assert not bool(gw[:, :, :2].any()) and not bool(gb[:, :, :2].any())
    assert bool(gw[:, :, 2].any()) and bool(gb[:, :, 2].any())
    if masked:  # a masked query's row is the output projection's bias
        assert torch.equal(got[~qm], m.query_output_proj.bias.detach().expand_as(got[~qm]))


def test_construction_errors_and_state_dict():
    with pytest.raises(ValueError, match="border"):
        MultiscaleDeformableAttention(12, 15, 3, 3, 4, "zeros", False, sampling_mode="discrete")
    with pytest.raises(ValueError, match="border"):
        MultiscaleDeformableAttention(12, 15, 3, 3, 4, "border", True, sampling_mode="discrete")
    with pytest.raises(ValueError, match="sampling_mode"):
        MultiscaleDeformableAttention(12, 15, 3, 3, 4, "border", False, sampling_mode="nearest")
    for npts in (4, [3, 6, 3]):
        a = MultiscaleDeformableAttention(12, 15, 3, 3, npts, "border", False)
        b = MultiscaleDeformableAttention(12, 15, 3, 3, npts, "border", False, sampling_mode="discrete")
        assert a.sampling_mode == "bilinear" and b.sampling_mode == "discrete"
        assert list(a.state_dict()) == list(b.state_dict())
        assert [tuple(v.shape) for v in a.state_dict().values()] == [tuple(v.shape) for v in b.state_dict().values()]
        b.load_state_dict(a.state_dict())
        # sampling_inputs() does not depend on the mode
        img, shapes, queries, ref, _, _ = _module_inputs(4)
        args = (shapes, queries.float(), ref.float())
        for x, y in zip(a.sampling_inputs(*args), b.sampling_inputs(*args)):
            assert torch.equal(x, y)
    import msda_triton
    shim = msda_triton.MultiscaleDeformableAttention(12, 15, 3, 3, 4, "border", False, sampling_mode="discrete")
    assert shim.sampling_mode == "discrete"


@pytest.mark.parametrize("fuse", [None, True, False])
def test_host_core_modes_and_errors(fuse):
    g = torch.Generator().manual_seed(3)
    counts = [3, 6, 3]
    value = torch.randn(2, sum(h * w for h, w in LEVELS), 3, 5, generator=g)
    shapes = torch.tensor(LEVELS)
    proj = torch.randn(2, 13, 3, sum(counts), 3, generator=g)
    ref = torch.rand(2, 13, 4, generator=g)
    got = fused_module_core(value, shapes, proj, ref, "border", False, points_per_level=counts, sampling_mode="discrete",
                            fuse_discrete=fuse)
    pts, att = ragged_module_sampling_inputs(proj, shapes, ref, counts)
    want = discrete.discrete_multiscale_deformable_attention(value, shapes, pts, att, "border", False, counts)
    assert torch.equal(got, want)
    # the uniform 6-D layout is the same call with equal counts
    p6 = torch.randn(2, 13, 3, 3, 4, 3, generator=g)
    a = fused_module_core(value, shapes, p6, ref, "border", False, sampling_mode="discrete", fuse_discrete=fuse)
    b = fused_module_core(value, shapes, p6.reshape(2, 13, 3, 12, 3), ref, "border", False, points_per_level=[4, 4, 4],
                          sampling_mode="discrete", fuse_discrete=fuse)
    pts, att = module_sampling_inputs(p6, shapes, ref)
    assert torch.equal(a, b)
    assert torch.equal(a, multiscale_deformable_attention(value, shapes, pts, att, "border", False, sampling_mode="discrete"))
    with pytest.raises(ValueError, match="border"):
        fused_module_core(value, shapes, proj, ref, "zeros", False, points_per_level=counts, sampling_mode="discrete")
    with pytest.raises(ValueError, match="border"):
        fused_module_core(value, shapes, proj, ref, "border", True, points_per_level=counts, sampling_mode="discrete")
    with pytest.raises(ValueError, match="sampling_mode"):
        fused_module_core(value, shapes, proj, ref, "border", False, points_per_level=counts, sampling_mode="nearest")
    # "bilinear" given explicitly is the call as it always was
    assert torch.equal(fused_module_core(value, shapes, proj, ref, "zeros", False, points_per_level=counts, sampling_mode="bilinear"),
                       fused_module_core(value, shapes, proj, ref, "zeros", False, points_per_level=counts))


def test_the_default_follows_the_measured_dtypes():
    from msda_triton_amd import module
    assert module.DISCRETE_IN_KERNELS_DTYPES == (torch.float32, torch.bfloat16)  # (the two that were measured)
    for dt in (torch.float32, torch.bfloat16, torch.float16, torch.float64):
        assert discrete.fuse_discrete_default(torch.empty(1, dtype=dt)) == (dt in module.DISCRETE_IN_KERNELS_DTYPES)
    assert MultiscaleDeformableAttention(12, 15, 3, 3, 4, "border", False, sampling_mode="discrete").fuse_discrete is None


# ------------------------------------------------------------------------------------------------ symbols and lists
def test_the_symbol_table(lib):
    assert _lib.has_module_discrete()
    want = {f"msda_{d}_fused_discrete_{s}" for d in ("fwd", "bwd") for s in SUFFIXES} | {"msda_bwd_fused_discrete_workspace_bytes"}
    assert len(_lib.MODULE_DISCRETE_SYMBOLS) == 17 and set(_lib.MODULE_DISCRETE_SYMBOLS) == want
    for other in (_lib.EXPORTED_SYMBOLS, _lib.QUERY_MASK_SYMBOLS, _lib.HFBOX_DISCRETE_SYMBOLS, _lib.MODULE_MASK_SYMBOLS):
        assert not set(_lib.MODULE_DISCRETE_SYMBOLS) & set(other)
    for s in _lib.MODULE_DISCRETE_SYMBOLS:
        assert hasattr(lib, s), s
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(_lib.MODULE_DISCRETE_SYMBOLS) <= set(re.findall(r" T (msda_\w+)", nm))
    assert lib.msda_abi_version() == 12


def _macro_decls(text, macro):
    body = re.search(r"#define " + macro + r"\(SUF\)(.*)", text).group(1)
    return {name: [re.sub(r"\s+", " ", p).strip() for p in params.split(",")]
            for name, params in re.findall(r"int msda_(\w+)_##SUF\(([^)]*)\)", body)}


def test_the_header_declares_them_through_macros_of_their_own():
    with open(os.path.join(ROOT, "include", "msda_hip.h")) as f:
        text = f.read().replace("\\\n", " ")
    decl = _macro_decls(text, "MSDA_MODULE_DISCRETE")
    assert set(decl) == {"fwd_fused_discrete", "bwd_fused_discrete"}
    used = re.findall(r"MSDA_MODULE_DISCRETE\((\w+)\)", text)
    assert sorted(s for s in used if s != "SUF") == sorted(SUFFIXES)
    assert "MSDA_MODULE_DISCRETE_QUERY(workspace_bytes)" in text
    assert "#undef MSDA_MODULE_DISCRETE\n" in text and "#undef MSDA_MODULE_DISCRETE_QUERY\n" in text
    for name, body in re.findall(r"#define (MSDA_DECLARE\w*)\(SUF\)(.*)", text):  # (those macros are EXPORTED_SYMBOLS')
        assert "fused_discrete_##SUF" not in body, name
    twins = _macro_decls(text, "MSDA_HFBOX_DISCRETE")
    for d in ("fwd", "bwd"):
        twin = twins[f"{d}_fused_hfbox_discrete"]
        at = twin.index("const float *level_scale")
        assert twin[at + 1] == "double offset_scale"
        assert decl[f"{d}_fused_discrete"] == twin[:at] + ["int ref_dim"] + twin[at + 2:], d


def test_each_ctypes_list_is_the_box_pairs_with_one_int_for_the_two_scales(lib):
    for d in ("fwd", "bwd"):
        for s in SUFFIXES:
            mine = list(getattr(lib, f"msda_{d}_fused_discrete_{s}").argtypes)
            twin = list(getattr(lib, f"msda_{d}_fused_hfbox_discrete_{s}").argtypes)
            at = twin.index(ctypes.c_double) - 1  # (level_scale, offset_scale)
            assert twin[at] is ctypes.c_void_p
            assert mine == twin[:at] + [ctypes.c_int] + twin[at + 2:], (d, s)
            assert getattr(lib, f"msda_{d}_fused_discrete_{s}").restype is ctypes.c_int
    q, t = lib.msda_bwd_fused_discrete_workspace_bytes, lib.msda_bwd_fused_hfbox_discrete_workspace_bytes
    assert list(q.argtypes) == list(t.argtypes) and q.restype is ctypes.c_int64


def test_the_workspace_query(lib):
    counts3 = (ctypes.c_int32 * 3)(3, 6, 3)
    args = (8, 8400, 8, 32, 300, 3, counts3, 4, 4, 0, 0)
    got = lib.msda_bwd_fused_discrete_workspace_bytes(*args)
    assert got == lib.msda_bwd_fused_hfbox_discrete_workspace_bytes(*args) and got >= 8 * 300 * 8 * 12 * 3 * 4
    counts9 = (ctypes.c_int32 * 9)(*([1] * 9))
    assert lib.msda_bwd_fused_discrete_workspace_bytes(2, 100, 2, 8, 5, 9, counts9, 4, 4, 0, 0) == 0  # (refused: L > 8)
    assert lib.msda_bwd_fused_discrete_workspace_bytes(2, 1 << 24, 2, 8, 5, 3, counts3, 4, 4, 0, 0) == 0  # (too large)
    bad = (ctypes.c_int32 * 3)(3, 0, 3)
    assert lib.msda_bwd_fused_discrete_workspace_bytes(2, 100, 2, 8, 5, 3, bad, 4, 4, 0, 0) == 0
    assert lib.msda_bwd_fused_discrete_workspace_bytes(2, 100, 2, 8, 5, 3, None, 4, 4, 0, 0) == 0


# ---------------------------------------------------------------------------------------------- argument-error table
no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="the rows pass host addresses as buffers: safe only where a "
                            "call that slipped past its guard cannot launch (the GPU side: test_gpu_module_discrete.py)")
DIMS = dict(B=1, I=4, H=1, D=4, Q=1, L=1)
BUFFERS = ("grad_out", "value", "shapes", "proj", "ref", "out", "grad_value", "grad_proj")


def _spec(direction):
    names = (["grad_out"] if direction == "bwd" else []) + ["value", "shapes", "proj", "ref"]
    names += ["out"] if direction == "fwd" else ["grad_value", "grad_proj"]
    names += list("BIHDQL") + ["ppl", "ref_dim"] + (["mlc"] if direction == "bwd" else []) + ["stride"]
    names += ["ws", "wsb"] if direction == "bwd" else []
    return names + ["stream"]


def _elem(name, suffix):
    es, ves, ss = SIZES[suffix]
    if name in ("value", "grad_value"):
        return ves
    if name == "shapes":
        return 8
    return ss if name in ("proj", "grad_proj", "out", "grad_out") else es


def _call(lib, direction, suffix, **over):
    buf = ctypes.create_string_buffer(4096 + 512)
    p = (ctypes.addressof(buf) + 255) // 256 * 256
    vals = dict(DIMS, ref_dim=2, mlc=0, stride=0, ws=None, wsb=0, stream=None)
    vals.update({n: p for n in BUFFERS})
    vals.update({k: (p + v[1] if isinstance(v, tuple) else v) for k, v in over.items()})
    ppl = over.get("ppl", [1] * max(int(vals["L"]), 1))
    arr = None if ppl is None else (ctypes.c_int32 * len(ppl))(*ppl)
    vals["ppl"] = None if arr is None else ctypes.cast(arr, ctypes.c_void_p)
    fn = getattr(lib, f"msda_{direction}_fused_discrete_{suffix}")
    names = _spec(direction)
    assert len(names) == len(fn.argtypes)
    rc = fn(*[vals[n] for n in names])
    ws = lib.msda_bwd_fused_discrete_workspace_bytes(*[vals[n] for n in "BIHDQL"], vals["ppl"], SIZES[suffix][0],
                                                     SIZES[suffix][1], 0, 0)
    del buf, arr
    return rc, ws


def _rows(direction, suffix):
    """(label, overrides, status, message keyword or None, does the workspace query see the fault too?)"""
    inputs = (["grad_out"] if direction == "bwd" else []) + ["value", "shapes", "proj", "ref"]
    outputs = ["out"] if direction == "fwd" else ["grad_value", "grad_proj"]
    rows = []
    for n in "BIHDQL":
        rows.append((f"{n}=-1", {n: -1}, BAD_ARG, None, True))
    for n in inputs + [o for o in outputs if o != "grad_value"]:
        rows.append((f"{n}=NULL", {n: None}, BAD_ARG, None, False))
    rows += [("points_per_level=NULL", {"ppl": None}, BAD_ARG, None, True), ("a count of 0", {"ppl": [0]}, BAD_ARG, None, True),
             ("a count of -3", {"ppl": [-3]}, BAD_ARG, None, True)]
    for rd in (0, 1, 3, 5, -2):
        rows.append((f"ref_dim={rd}", {"ref_dim": rd}, BAD_ARG, "ref_dim", False))
    rows.append(("ref_dim=3 with I=2^24", {"ref_dim": 3, "I": 1 << 24}, BAD_ARG, "ref_dim", True))
    rows.append(("L=33", {"L": 33, "ppl": [1] * 33}, TOO_MANY_LEVELS, None, True))
    rows.append(("L=33 with I=2^24", {"L": 33, "ppl": [1] * 33, "I": 1 << 24}, TOO_MANY_LEVELS, None, True))
    base = {"grad_value": None} if direction == "bwd" else {}
    for L in (9, 32):
        rows.append((f"L={L}", dict(base, L=L, ppl=[1] * L), UNSUPPORTED, "levels", True))
    rows.append(("I too large", {"I": 1 << 24}, TOO_LARGE, None, True))
    rows.append(("too large with a null input", {"I": 1 << 24, "value": None}, TOO_LARGE, None, True))
    for n in inputs + outputs:
        rows.append((f"{n}+half", {n: ("shift", _elem(n, suffix) // 2)}, MISALIGNED, "misaligned", False))
    rows.append(("misaligned with a bad stride", {"value": ("shift", _elem("value", suffix) // 2), "stride": -16}, MISALIGNED,
                 "misaligned", False))
    if direction == "bwd":
        rows += [("ws=NULL", {"ws": None, "wsb": 1 << 20}, BAD_ARG, None, False),
                 ("ws misaligned", {"ws": ("shift", 128), "wsb": 1 << 20}, BAD_ARG, None, False),
                 ("ws too small", {"ws": ("shift", 0), "wsb": 8}, BAD_ARG, None, False)]
    dense = DIMS["H"] * DIMS["D"] * SIZES[suffix][1]
    rows += [("stride negative", dict(base, stride=-dense), BAD_ARG, None, False),
             ("stride below the dense row", dict(base, stride=dense - SIZES[suffix][1]), BAD_ARG, None, False),
             ("stride no multiple of the element", dict(base, stride=2 * dense + 1), BAD_ARG, None, False)]
    # nothing to produce: an empty call returns 0 without looking at its buffers
    nulls = {n: None for n in BUFFERS}
    rows.append(("B=0, buffers NULL", dict(nulls, B=0), 0, None, False))
    if direction == "fwd":
        rows.append(("Q=0, buffers NULL", dict(nulls, Q=0), 0, None, False))
    return rows


@no_gpu
@pytest.mark.parametrize("direction", ["fwd", "bwd"])
def test_argument_errors_are_answered_before_anything_is_launched(lib, direction):
    for suffix in SUFFIXES:
        for label, over, want, word, query_sees in _rows(direction, suffix):
            assert lib.msda_get_option(b"no such option") == -1  # (leaves its own text behind: the next one is this call's)
            stale = lib.msda_last_error()
            rc, ws = _call(lib, direction, suffix, **over)
            msg = lib.msda_last_error()
            where = (label, direction, suffix, rc, msg)
            assert rc == want, where
            if want != 0:
                assert msg and msg != stale, where
                if word is not None:
                    assert re.search(word, msg.decode()), where
                if query_sees:  # the sizes themselves are refused: there is no call to size a workspace for
                    assert ws == 0, where


# --------------------------------------------------------------------------------- the rule in numpy fp32, and its mutants
def np_rule(xy, ref, levels, counts, mutant=None):
    """The kernels' per-sample rule, operation by operation in fp32: xy [N, S, 2] offsets, ref [N, 2 | 4] ->
    (points [N, S, 2] fp32, pixel [N, S] int64)."""
    f32 = np.float32
    xy, ref = xy.astype(f32), ref.astype(f32)
    N, S, _ = xy.shape
    pts, pix = np.empty((N, S, 2), f32), np.empty((N, S), np.int64)
    s0 = start = 0
    for (h, w), P in zip(levels, counts):
        o = xy[:, s0:s0 + P]
        if ref.shape[-1] == 2:
            dx, dy = (f32(w), f32(h)) if mutant == "wh_order" else (f32(h), f32(w))
            x, y = ref[:, None, 0] + o[..., 0] / dx, ref[:, None, 1] + o[..., 1] / dy
        else:
            den = f32(2 * (max(counts) if mutant == "max_p" else P))
            tx, ty = o[..., 0] * ref[:, None, 2], o[..., 1] * ref[:, None, 3]
            if mutant == "reciprocal":
                qx, qy = tx * (f32(1) / den), ty * (f32(1) / den)
            else:
                qx, qy = tx / den, ty / den
            x, y = ref[:, None, 0] + qx, ref[:, None, 1] + qy
        assert x.dtype == f32 and y.dtype == f32
        if mutant == "fma":  # one rounding: the exact product and sum in fp64, rounded to fp32 once
            tx, ty = (x.astype(np.float64) * w + 0.5).astype(f32), (y.astype(np.float64) * h + 0.5).astype(f32)
        else:
            tx, ty = x * f32(w) + f32(0.5), y * f32(h) + f32(0.5)
        with np.errstate(invalid="ignore"):
            ix = np.clip(np.trunc(tx), 0, w - 1).astype(np.int64)
            iy = np.clip(np.trunc(ty), 0, h - 1).astype(np.int64)
        pts[:, s0:s0 + P, 0], pts[:, s0:s0 + P, 1] = x, y
        pix[:, s0:s0 + P] = start + iy * w + ix
        s0, start = s0 + P, start + h * w
    return pts, pix


def torch_pixels(pts, levels, counts):
    """the discrete operator's host formulation of the pixel (discrete.native_discrete), on fp32 points [N, S, 2]"""
    out, s0, start = [], 0, 0
    for (h, w), P in zip(levels, counts):
        xy = pts[:, s0:s0 + P]
        ix = torch.clamp(torch.trunc(xy[..., 0] * w + 0.5), 0, w - 1).to(torch.int64)
        iy = torch.clamp(torch.trunc(xy[..., 1] * h + 0.5), 0, h - 1).to(torch.int64)
        out.append(start + iy * w + ix)
        s0, start = s0 + P, start + h * w
    return torch.cat(out, -1)


def boundary_fixture(ref_dim, levels, counts):
    """every rounding boundary of every level's axes as the reference point of a query; zero offsets (2-d), zero-size
    boxes and random offsets (4-d): the point is the reference point"""
    xs = np.concatenate([boundary_coords(w, np.float32) for _, w in levels])
    ys = np.concatenate([boundary_coords(h, np.float32) for h, _ in levels])
    n = max(len(xs), len(ys))
    x = np.concatenate([np.resize(xs, n), np.resize(xs, n), np.resize(xs[::-1], n)])
    y = np.concatenate([np.resize(ys, n), np.resize(ys[::-1], n), np.resize(ys, n)])
    S = sum(counts)
    if ref_dim == 2:
        return np.zeros((len(x), S, 2), np.float32), np.stack([x, y], -1)
    xy = np.random.default_rng(5).standard_normal((len(x), S, 2)).astype(np.float32) * 1.5
    return xy, np.stack([x, y, np.zeros_like(x), np.zeros_like(x)], -1)


def random_fixture(ref_dim, counts, n=4000):
    rng = np.random.default_rng(71 + ref_dim)
    return (rng.standard_normal((n, sum(counts), 2)) * 1.5).astype(np.float32), rng.random((n, ref_dim)).astype(np.float32)


D32 = SHAPES["d32"][4][:3]


@pytest.mark.parametrize("counts", [[3, 6, 3], [3, 3, 3]], ids=["3_6_3", "p3"])
@pytest.mark.parametrize("ref_dim", [2, 4])
def test_numpy_rule_is_the_host_yardstick(ref_dim, counts):
    """... so the mutants below are mutants of the rule the GPU tests hold the kernels to: the same points bit for bit, the
    same pixels.  (P = 3: torch's CPU division by a Python scalar is the true division.)"""
    for xy, ref in (random_fixture(ref_dim, counts), boundary_fixture(ref_dim, D32, counts)):
        N, S, _ = xy.shape
        proj = torch.cat([torch.from_numpy(xy), torch.zeros(N, S, 1)], -1).reshape(1, N, 1, S, 3)
        pts, _ = ragged_module_sampling_inputs(proj, torch.tensor(D32), torch.from_numpy(ref)[None], counts)
        mine, pix = np_rule(xy, ref, D32, counts)
        assert pts.dtype == torch.float32 and np.array_equal(pts[0, :, 0].numpy(), mine, equal_nan=True)
        assert np.array_equal(torch_pixels(pts[0, :, 0], D32, counts).numpy(), pix)


def test_mutants_on_the_boundary_fixture():
    counts = [3, 6, 3]
    changed = {}
    for ref_dim in (2, 4):
        xy, ref = boundary_fixture(ref_dim, D32, counts)
        _, base = np_rule(xy, ref, D32, counts)
        for mutant in ("fma",) + (("wh_order",) if ref_dim == 2 else ("max_p", "reciprocal")):
            changed[mutant, ref_dim] = int((np_rule(xy, ref, D32, counts, mutant)[1] != base).sum())
    print(changed)
    # recorded as NOT detectable on this fixture (module docstring)
    assert not any(changed.values()), changed
    # the fused multiply-add IS a mutant: the same coordinates on an axis of 19 pixels part from the two-rounding rule
    c = boundary_coords(19, np.float32)
    sep = np.trunc(c * np.float32(19) + np.float32(0.5))
    fma = np.trunc((c.astype(np.float64) * 19 + 0.5).astype(np.float32))
    assert int((np.clip(sep, 0, 18) != np.clip(fma, 0, 18)).sum()) > 0


def test_mutants_the_boundary_fixture_cannot_see_show_on_the_random_one():
    counts = [3, 6, 3]
    xy, ref = random_fixture(2, counts)
    assert (np_rule(xy, ref, D32, counts, "wh_order")[1] != np_rule(xy, ref, D32, counts)[1]).sum() > 0
    xy, ref = random_fixture(4, counts)
    pts, pix = np_rule(xy, ref, D32, counts)
    assert (np_rule(xy, ref, D32, counts, "max_p")[1] != pix).sum() > 0
    # the reciprocal: a different POINT (the parked-point test's bit-for-bit comparison), on levels with P = 3 only
    rpts, rpix = np_rule(xy, ref, D32, counts, "reciprocal")
    differ = (rpts != pts).any(-1)
    print("reciprocal-multiply: points that differ", int(differ.sum()), "pixels that differ", int((rpix != pix).sum()))
    assert differ[:, :3].sum() + differ[:, 9:].sum() > 0  # (the samples of the two levels with P = 3)
