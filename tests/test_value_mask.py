"""The value padding mask (``value_mask=``) without a GPU: the contract on host tensors through every public route, the
composition routes, the new C-ABI symbols with their guards, the Hugging Face adapter's hand-over, and the argument checks.

The contract (include/msda_hip.h, "VALUE PADDING MASK"): with ``m`` the mask broadcast over heads and channels,

    out, grad_loc, grad_attn (grad_proj, grad_ref)  ==  those of the unmasked operator on  where(m, value, 0)
    grad_value                                      ==  where(m, grad_value of the unmasked operator, +0)

whatever bits the masked pixels hold."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import MODES, kink_mask, mode_key
from msda_triton_amd import MultiscaleDeformableAttention, _lib, functional
from msda_triton_amd.functional import (fused_hf_box_core, fused_hf_module_core, fused_module_core,
                                        multiscale_deformable_attention)

LEVELS = [(5, 7), (3, 2), (2, 6)]
I = sum(h * w for h, w in LEVELS)  # noqa: E741
# the tolerances of tests/test_reference_suite.py
TOL = {torch.float32: {"fwd": (1e-4, 1e-3), "bwd": (1e-3, 1e-2)}, torch.float64: {"fwd": (1e-8, 1e-8), "bwd": (1e-8, 1e-8)}}


def _mask(B, seed=0):
    g = torch.Generator().manual_seed(100 + seed)
    m = torch.rand(B, I, generator=g) < 0.6
    m[0, 0] = False  # (the first and the last pixel of the pyramid are always among the masked / the real ones)
    m[-1, -1] = True
    return m


def _case(dtype, B=2, Q=9, H=3, D=4, P=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    L = len(LEVELS)
    value = torch.randn(B, I, H, D, generator=g, dtype=dtype)
    loc = (torch.rand(B, Q, H, L, P, 2, generator=g, dtype=dtype) * 1.4 - 0.2)
    attn = torch.rand(B, Q, H, L, P, generator=g, dtype=dtype)
    go = torch.randn(B, Q, H, D, generator=g, dtype=dtype)
    return value, torch.tensor(LEVELS), loc, attn, go


def _grads(fn, tensors, go):
    """fn over fresh leaves of `tensors` -> (out, grads...)"""
    leaves = [t.detach().clone().requires_grad_(True) for t in tensors]
    out = fn(*leaves)
    out.backward(go)
    return (out.detach(),) + tuple(t.grad for t in leaves)


def _poisoned(value, m, poison=float("nan")):
    return torch.where(m[:, :, None, None], value, torch.full_like(value, poison))


def _premasked(value, m):
    return torch.where(m[:, :, None, None], value, torch.zeros_like(value))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("pm,ac", MODES, ids=[mode_key(*m) for m in MODES])
def test_host_operator_holds_the_contract(oracle, pm, ac, dtype):
    value, shapes, loc, attn, go = _case(dtype)
    m = _mask(value.shape[0])
    pre = _premasked(value, m)
    want = _grads(lambda v, l, a: multiscale_deformable_attention(v, shapes, l, a, pm, ac), (pre, loc, attn), go)
    for mask in (m, m.to(torch.uint8)):
        for v in (value, _poisoned(value, m), _poisoned(value, m, float("inf"))):  # NaN / Inf in padding change nothing
            got = _grads(lambda v_, l, a: multiscale_deformable_attention(v_, shapes, l, a, pm, ac, value_mask=mask),
                         (v, loc, attn), go)
            assert torch.equal(got[0], want[0])
            assert torch.equal(got[2], want[2]) and torch.equal(got[3], want[3])
            assert torch.equal(got[1], torch.where(m[:, :, None, None], want[1], torch.zeros_like(want[1])))
            assert (got[1][~m] == 0).all() and not torch.signbit(got[1][~m]).any()  # exactly +0 in the padding
    # ... and the CPU oracle on the pre-masked value agrees
    host = [t.numpy() for t in (pre, shapes, loc, attn)]
    (fa, fr), (ba, br) = TOL[dtype]["fwd"], TOL[dtype]["bwd"]
    np.testing.assert_allclose(want[0].numpy(), oracle.forward(*host, pm, ac), atol=fa, rtol=fr)
    r_gv, r_gl, r_ga = oracle.backward(go.numpy(), *host, pm, ac)
    got = _grads(lambda v_, l, a: multiscale_deformable_attention(v_, shapes, l, a, pm, ac, value_mask=m),
                 (_poisoned(value, m), loc, attn), go)
    np.testing.assert_allclose(got[1].numpy(), np.where(m[:, :, None, None].numpy(), r_gv, 0), atol=ba, rtol=br)
    np.testing.assert_allclose(got[3].numpy(), r_ga, atol=ba, rtol=br)
    keep = ~kink_mask(loc.numpy(), shapes.numpy(), ac)
    np.testing.assert_allclose(np.where(keep, got[2].numpy(), 0), np.where(keep, r_gl, 0), atol=ba, rtol=br)


def _check_route(fn_masked, fn_plain, tensors, go, m):
    """A composition route: value_mask=m on the poisoned value == the route on where(m, value, 0), bit for bit; tensors[0]
    is the value pyramid."""
    value = tensors[0]
    want = _grads(fn_plain, (_premasked(value, m),) + tuple(tensors[1:]), go)
    got = _grads(fn_masked, (_poisoned(value, m),) + tuple(tensors[1:]), go)
    assert torch.equal(got[0], want[0])
    assert torch.equal(got[1], torch.where(m[:, :, None, None], want[1], torch.zeros_like(want[1])))
    assert (got[1][~m] == 0).all()
    for g, w in zip(got[2:], want[2:]):
        assert (g is None and w is None) or torch.equal(g, w)


def test_points_per_level_route_composes():
    counts = (3, 1, 2)
    value, shapes, _, _, go = _case(torch.float32, seed=1)
    g = torch.Generator().manual_seed(5)
    B, Q, H = value.shape[0], go.shape[1], value.shape[2]
    loc = torch.rand(B, Q, H, sum(counts), 2, generator=g) * 1.4 - 0.2
    attn = torch.rand(B, Q, H, sum(counts), generator=g)
    m = _mask(B, 1)
    _check_route(lambda v, l, a: multiscale_deformable_attention(v, shapes, l, a, "zeros", False, points_per_level=counts, value_mask=m),
                 lambda v, l, a: multiscale_deformable_attention(v, shapes, l, a, "zeros", False, points_per_level=counts),
                 (value, loc, attn), go, m)


def test_discrete_route_composes():
    value, shapes, loc, attn, go = _case(torch.float32, seed=2)
    m = _mask(value.shape[0], 2)

    def run(v, a, **kw):
        return multiscale_deformable_attention(v, shapes, loc, a, "border", False, sampling_mode="discrete", **kw)

    _check_route(lambda v, a: run(v, a, value_mask=m), run, (value, attn), go, m)


def _hf_inputs(ref_dim, dtype=torch.float32, seed=3, B=2, Q=7, H=3, D=4, P=3):
    g = torch.Generator().manual_seed(seed)
    L = len(LEVELS)
    value = torch.randn(B, I, H, D, generator=g, dtype=dtype)
    proj = torch.randn(B, Q, H, L, P, 3, generator=g, dtype=dtype)
    ref = torch.rand(B, Q, L, ref_dim, generator=g, dtype=dtype)
    go = torch.randn(B, Q, H, D, generator=g, dtype=dtype)
    return value, torch.tensor(LEVELS), proj, ref, go


@pytest.mark.parametrize("ref_dim", [2, 4])
def test_fused_hf_module_core_composes_on_the_host(ref_dim):
    value, shapes, proj, ref, go = _hf_inputs(ref_dim)
    m = _mask(value.shape[0], 3)
    for kw in ({}, {"mask_in_kernels": False}):
        _check_route(lambda v, p, r: fused_hf_module_core(v, shapes, p, r, "zeros", False, value_mask=m, **kw),
                     lambda v, p, r: fused_hf_module_core(v, shapes, p, r, "zeros", False), (value, proj, ref), go, m)


@pytest.mark.parametrize("ref_dim", [2, 4])
def test_fused_module_core_composes(ref_dim):
    value, shapes, proj, ref, go = _hf_inputs(ref_dim, seed=4)
    ref = ref[:, :, 0].contiguous()
    m = _mask(value.shape[0], 4)
    _check_route(lambda v, p, r: fused_module_core(v, shapes, p, r, "border", True, value_mask=m),
                 lambda v, p, r: fused_module_core(v, shapes, p, r, "border", True), (value, proj, ref), go, m)


def test_fused_hf_box_core_composes():
    counts = (3, 1, 2)
    value, shapes, _, _, go = _hf_inputs(4, seed=5)
    g = torch.Generator().manual_seed(6)
    B, Q, H = value.shape[0], go.shape[1], value.shape[2]
    proj = torch.randn(B, Q, H, sum(counts), 3, generator=g)
    box = torch.rand(B, Q, 4, generator=g)
    m = _mask(B, 5)
    _check_route(lambda v, p, r: fused_hf_box_core(v, shapes, p, r, counts, value_mask=m),
                 lambda v, p, r: fused_hf_box_core(v, shapes, p, r, counts), (value, proj, box), go, m)


def test_nn_module_applies_the_mask_behind_its_value_projection():
    torch.manual_seed(0)
    mod = MultiscaleDeformableAttention(16, 12, len(LEVELS), 3, 2, "zeros", False)
    g = torch.Generator().manual_seed(7)
    img, queries, ref = torch.randn(2, I, 16, generator=g), torch.randn(2, 5, 16, generator=g), torch.rand(2, 5, 2, generator=g)
    shapes = torch.tensor(LEVELS)
    m = _mask(2, 6)
    out = mod(img, shapes, queries, ref, value_mask=m)
    # the pixels' inputs do not matter where the mask is 0 — the projection's bias included
    other = torch.where(m[:, :, None], img, torch.randn(2, I, 16, generator=g))
    assert torch.equal(out, mod(other, shapes, queries, ref, value_mask=m))
    # ... and it is the module's own core on the masked projection
    value = torch.nn.functional.linear(img, mod.img_input_proj.weight, mod.img_input_proj.bias).reshape(2, I, 3, 4)
    proj = mod.query_input_proj(queries).reshape(2, 5, 3, len(LEVELS), 2, 3)
    want = mod.query_output_proj(fused_module_core(_premasked(value, m), shapes, proj, ref, "zeros", False).reshape(2, 5, 12))
    torch.testing.assert_close(out, want, atol=1e-6, rtol=1e-5)
    assert not torch.equal(out, mod(img, shapes, queries, ref))  # the mask has an effect


@pytest.mark.parametrize("ref_dim", [2, 4])
def test_gradcheck_fp64_with_a_mask(ref_dim):
    """value and points, at the sizes of test_hf_fused.test_host_core_gradcheck_fp64"""
    levels = [(3, 2), (2, 3)]
    g = torch.Generator().manual_seed(2)
    value = torch.randn(1, 12, 2, 4, generator=g, dtype=torch.float64)
    proj = torch.randn(1, 3, 2, 2, 2, 3, generator=g, dtype=torch.float64) * 0.45
    ref = 0.25 + 0.5 * torch.rand(1, 3, 2, ref_dim, generator=g, dtype=torch.float64)
    shapes = torch.tensor(levels)
    m = torch.tensor([[1, 0, 1, 1, 0, 1, 1, 1, 0, 1, 1, 0]], dtype=torch.bool)
    value.requires_grad_(True), proj.requires_grad_(True), ref.requires_grad_(True)
    assert torch.autograd.gradcheck(lambda v, p, r: fused_hf_module_core(v, shapes, p, r, "zeros", False, value_mask=m),
                                    (value, proj, ref), eps=1e-6, atol=1e-6, rtol=1e-4)
    pts, att = functional.hf_module_sampling_inputs(proj.detach(), shapes, ref.detach())
    pts.requires_grad_(True), att.requires_grad_(True)
    assert torch.autograd.gradcheck(lambda v, l, a: multiscale_deformable_attention(v, shapes, l, a, "zeros", False, value_mask=m),
                                    (value, pts, att), eps=1e-6, atol=1e-6, rtol=1e-4)


# ------------------------------------------------------------------------------------------ the C ABI
def test_masked_symbols_exist_for_every_suffix_with_the_twins_lists_plus_one_pointer():
    lib = _lib.load()
    assert _lib.has_value_mask()
    vp = ctypes.c_void_p
    for stem, twin, suffixes in (("msda_{}_masked_{}", "msda_{}_{}", _lib.DTYPE_SUFFIXES),
                                 ("msda_{}_fused_levelref_masked_{}", "msda_{}_fused_levelref_{}",
                                  _lib.DTYPE_SUFFIXES + _lib.FUSED_STORAGE_SUFFIXES)):
        for suf in suffixes:
            for d in ("fwd", "bwd"):
                name = stem.format(d, suf)
                assert name in _lib.EXPORTED_SYMBOLS
                got, want = getattr(lib, name).argtypes, getattr(lib, twin.format(d, suf)).argtypes
                k = 1 if d == "fwd" else 2  # `value_mask` sits behind `value`
                assert list(got) == list(want[:k]) + [vp] + list(want[k:]), name


def _masked_call(sg, lib, host, family, suffix, d, mask):
    """tests/test_size_guards._call for the masked twin of `family` ("fwd", "bwd", "fwd_fused", "bwd_fused")."""
    backward, fused = family.startswith("bwd"), family.endswith("fused")
    fn = getattr(lib, ("msda_{}_fused_levelref_masked_{}" if fused else "msda_{}_masked_{}").format(family[:3], suffix))
    p = host.p
    B, I_, H, D, Q, S, stride = (d[k] for k in ("B", "I", "H", "D", "Q", "S", "stride"))
    sizes = (B, I_, H, D, Q, 1, S)
    gv = p if not fused else None
    if not backward:
        return fn(p, mask, p, p, p, p, *sizes, 2, 0, 0, stride, None) if fused else fn(p, mask, p, p, p, p, *sizes, 0, 0, stride, None)
    if fused:
        return fn(p, p, mask, p, p, p, gv, p, p, *sizes, 2, 0, 0, 0, stride, None, 0, None)
    return fn(p, p, mask, p, p, p, gv, p, p, *sizes, 0, 0, 0, stride, None, 0, None)


def _guard_rows():
    import test_size_guards as sg
    return list(sg.ROWS)


@pytest.mark.parametrize("row", _guard_rows())
def test_guards_answer_what_the_twins_answer(row):
    import test_size_guards as sg
    lib = _lib.load()
    for family, suffix in (("fwd", "f32"), ("bwd", "f32"), ("fwd", "bf16"), ("bwd", "f64"), ("fwd", "f32_vbf16"),
                           ("fwd_fused", "f32"), ("bwd_fused", "f32"), ("fwd_fused", "f32_sbf16"), ("bwd_fused", "f64")):
        if not sg._applies(row, family):
            continue
        es, ves = sg.SIZES[suffix]
        d = sg._isolates(row, family, es, ves)
        host = sg._Host()
        want = sg._call(lib, host, family, suffix, d)
        got = _masked_call(sg, lib, host, family, suffix, d, host.p)
        assert got == want == sg.TOO_LARGE, (row, family, suffix, got, want, lib.msda_last_error())


def test_a_null_mask_is_a_bad_argument_before_any_pointer_is_read():
    import test_size_guards as sg
    lib = _lib.load()
    host = sg._Host()
    for family, suffixes in (("fwd", _lib.DTYPE_SUFFIXES), ("bwd", _lib.DTYPE_SUFFIXES),
                             ("fwd_fused", _lib.DTYPE_SUFFIXES + _lib.FUSED_STORAGE_SUFFIXES),
                             ("bwd_fused", _lib.DTYPE_SUFFIXES + _lib.FUSED_STORAGE_SUFFIXES)):
        for suf in suffixes:
            # (valid small sizes and dummy host addresses: a call that got past the check would try to launch on them)
            rc = _masked_call(sg, lib, host, family, suf, sg._dims(I=4, D=4, Q=2, S=2), None)
            assert rc == -1, (family, suf, rc)
            assert b"value_mask" in lib.msda_last_error()
            # ... also where the sizes alone would be refused: the mask is looked at first
            assert _masked_call(sg, lib, host, family, suf, sg._dims(I=1 << 24), None) == -1


# ------------------------------------------------------------------------------------------ argument checks
def test_bad_masks_raise_value_error():
    value, shapes, loc, attn, _ = _case(torch.float32)
    B = value.shape[0]
    calls = (lambda mk: multiscale_deformable_attention(value, shapes, loc, attn, "zeros", False, value_mask=mk),
             lambda mk: fused_hf_module_core(*_hf_inputs(2)[:4], "zeros", False, value_mask=mk),
             lambda mk: functional.apply_value_mask(value, mk))
    for call in calls:
        with pytest.raises(ValueError, match="bool or uint8"):
            call(torch.ones(B, I))
        with pytest.raises(ValueError, match="value_mask"):
            call(torch.ones(B, I, 1, dtype=torch.bool))
        with pytest.raises(ValueError, match="value_mask"):
            call(torch.ones(B, I + 1, dtype=torch.bool))
        with pytest.raises(ValueError, match="device"):
            call(torch.ones(B, I, dtype=torch.bool, device="meta"))
    with pytest.raises(ValueError):
        functional.hip_multiscale_deformable_attention(value, shapes, loc, attn, "zeros", False,
                                                       value_mask=torch.ones(B, I, dtype=torch.bool))  # host tensors


def test_a_bool_mask_travels_as_its_uint8_view_without_a_copy():
    m = _mask(2)
    u8 = functional.check_value_mask(m, torch.empty(2, I, 1, 1))
    assert u8.dtype == torch.uint8 and u8.data_ptr() == m.data_ptr()


def test_sharded_operators_refuse_a_mask():
    from msda_triton_amd import distributed
    value, shapes, loc, attn, _ = _case(torch.float32)
    m = _mask(value.shape[0])
    with pytest.raises(ValueError, match="value_mask"):
        distributed.sharded_multiscale_deformable_attention(value, shapes, loc, attn, "zeros", False, value_mask=m)
    with pytest.raises(ValueError, match="value_mask"):
        distributed.row_sharded_multiscale_deformable_attention(value, shapes, loc, attn, "zeros", False, value_mask=m,
                                                                compute_only_as=(2, 0))


# ------------------------------------------------------------------------------------------ the HF adapter
def _spy_core(monkeypatch):
    """Patches the adapter's fused_hf_module_core: records every call's mask, runs the real function."""
    from msda_triton_amd import hf_adapter
    seen = []
    real = hf_adapter.fused_hf_module_core

    def spy(value, *args, **kw):
        seen.append((value, kw.get("value_mask")))
        return real(value, *args, **kw)

    monkeypatch.setattr(hf_adapter, "fused_hf_module_core", spy)
    return seen


def _assert_mask_reached_the_core(seen, pixel_mask_pads):
    assert len(seen) == 4 and all(mk is not None for _, mk in seen)
    for value, mk in seen:
        assert tuple(mk.shape) == tuple(value.shape[:2]) and mk.dtype == torch.bool
        assert pixel_mask_pads and not mk.all() and mk[0].all()  # element 1 is really padded, element 0 is not
        # no masked_fill of the adapter's own: the padding pixels still hold the value projection's output (its bias at least)
        assert (value[~mk] != 0).any()


def test_wrapped_deformable_detr_hands_the_padding_mask_to_the_core(monkeypatch):
    pytest.importorskip("transformers")
    from test_hf_model import WATCHED, _inputs, run_model, tiny_deformable_detr
    from msda_triton_amd.hf_adapter import replace_hf_msda
    model = tiny_deformable_detr()
    x, mask = _inputs("cpu")
    assert not mask[1].all() and mask[0].all()  # the pixel_mask really pads one image
    hs0, enc0, g0 = run_model(model, x, mask)
    assert replace_hf_msda(model, fused=True) == 8
    seen = _spy_core(monkeypatch)
    hs1, enc1, g1 = run_model(model, x, mask)
    _assert_mask_reached_the_core(seen, True)
    torch.testing.assert_close(enc1, enc0, atol=1e-5, rtol=1e-4)
    torch.testing.assert_close(hs1, hs0, atol=1e-5, rtol=1e-4)
    for k in WATCHED:
        err = float((g1[k] - g0[k]).norm() / g0[k].norm().clamp_min(1e-30))
        assert err < 1e-4, (k, err)


def test_wrapped_grounding_dino_hands_the_padding_mask_to_the_core(monkeypatch):
    pytest.importorskip("transformers")
    from test_hf_model import GDINO_WATCHED, _gdino_inputs, run_gdino, tiny_grounding_dino
    from msda_triton_amd.hf_adapter import replace_hf_msda
    model = tiny_grounding_dino()
    inputs = _gdino_inputs("cpu")
    assert not inputs["pixel_mask"][1].all()
    hs0, enc0, ref0, g0 = run_gdino(model, inputs)
    assert replace_hf_msda(model, fused=True) == 8
    seen = _spy_core(monkeypatch)
    hs1, enc1, ref1, g1 = run_gdino(model, inputs)
    _assert_mask_reached_the_core(seen, True)
    torch.testing.assert_close(ref1, ref0, atol=1e-5, rtol=1e-4)
    torch.testing.assert_close(enc1, enc0, atol=1e-5, rtol=1e-4)
    torch.testing.assert_close(hs1, hs0, atol=1e-5, rtol=1e-4)
    for k in GDINO_WATCHED:
        err = float((g1[k] - g0[k]).norm() / g0[k].norm().clamp_min(1e-30))
        assert err < 1e-4, (k, err)
