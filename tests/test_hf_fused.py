"""The fused prologue for Hugging Face attention modules, without a GPU: transformers' prologue stated once
(`functional.hf_module_sampling_inputs`), `fused_hf_module_core` on host tensors, the `replace_hf_msda(model, fused=True)`
wrapper on the tiny Deformable-DETR / Grounding-DINO of tests/test_hf_model.py, and the new C-ABI symbols with their size
guards (msda_{fwd,bwd}_fused_levelref_<suffix>)."""
import pytest
import torch

from msda_triton_amd import _lib, functional
from msda_triton_amd.functional import (fused_hf_module_core, hf_module_sampling_inputs, module_sampling_inputs,
                                        multiscale_deformable_attention)

LEVELS = [(5, 7), (3, 2), (2, 6)]  # every level non-square


def hf_expression(sampling_offsets, logits, reference_points, spatial_shapes, n_points):
    """DeformableDetrMultiscaleDeformableAttention.forward between its projections and its core
    (transformers/models/deformable_detr/modeling_deformable_detr.py), on the tensors that module's two Linear layers give."""
    import torch.nn.functional as F
    batch_size, num_queries, n_heads, n_levels = sampling_offsets.shape[:4]
    attention_weights = F.softmax(logits, -1).view(batch_size, num_queries, n_heads, n_levels, n_points)
    num_coordinates = reference_points.shape[-1]
    if num_coordinates == 2:
        offset_normalizer = torch.stack([spatial_shapes[..., 1], spatial_shapes[..., 0]], -1)
        sampling_locations = (
            reference_points[:, :, None, :, None, :]
            + sampling_offsets / offset_normalizer[None, None, None, :, None, :]
        )
    else:
        sampling_locations = (
            reference_points[:, :, None, :, None, :2]
            + sampling_offsets / n_points * reference_points[:, :, None, :, None, 2:] * 0.5
        )
    return sampling_locations, attention_weights


def make(B, Q, H, D, levels, P, ref_dim, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    L = len(levels)
    value = torch.randn(B, sum(h * w for h, w in levels), H, D, generator=g, dtype=dtype)
    proj = torch.randn(B, Q, H, L, P, 3, generator=g, dtype=dtype) * 1.5
    ref = torch.rand(B, Q, L, ref_dim, generator=g, dtype=dtype)  # a point per level, drawn independently
    return value, torch.tensor(levels), proj, ref


@pytest.mark.parametrize("P", [3, 4])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("ref_dim", [2, 4])
def test_prologue_is_transformers_expression_bit_for_bit(ref_dim, dtype, P):
    _, shapes, proj, ref = make(2, 11, 3, 4, LEVELS, P, ref_dim, dtype, seed=ref_dim + P)
    B, Q, H, L = proj.shape[:4]
    offsets = proj[..., :2].contiguous()                      # what `sampling_offsets(hidden).view(...)` is
    logits = proj[..., 2].reshape(B, Q, H, L * P).contiguous()  # ... and `attention_weights(hidden).view(...)`
    want_pts, want_att = hf_expression(offsets, logits, ref, shapes, P)
    pts, att = hf_module_sampling_inputs(proj, shapes, ref)
    assert pts.dtype == dtype and tuple(pts.shape) == (B, Q, H, L, P, 2)
    assert torch.equal(pts, want_pts)
    assert torch.equal(att, want_att)


def test_prologue_is_not_the_reference_modules_rule():
    """On a non-square level (x, y) / (w, h) and (x, y) / (h, w) differ: the two prologues must not be the same code."""
    _, shapes, proj, ref = make(1, 5, 2, 4, LEVELS, 4, 2, torch.float32, seed=9)
    same_point = ref[:, :, :1].expand(-1, -1, len(LEVELS), -1).contiguous()
    hf, _ = hf_module_sampling_inputs(proj, shapes, same_point)
    reference, att = module_sampling_inputs(proj, shapes, same_point[:, :, 0])
    assert not torch.equal(hf, reference)
    # ... and differ by exactly the swap: the x offset over the width against the x offset over the height
    dx_hf, dx_ref = hf[..., 0] - same_point[:, :, None, :, None, 0], reference[..., 0] - same_point[:, :, None, :, None, 0]
    w_over_h = torch.tensor([w / h for h, w in LEVELS])[None, None, None, :, None]
    torch.testing.assert_close(dx_hf * w_over_h, dx_ref, atol=1e-6, rtol=1e-5)
    assert torch.equal(att, hf_module_sampling_inputs(proj, shapes, same_point)[1])


def test_prologue_rejects_reference_points_without_a_level_axis():
    _, shapes, proj, ref = make(1, 5, 2, 4, LEVELS, 4, 2, torch.float32)
    with pytest.raises(ValueError):
        hf_module_sampling_inputs(proj, shapes, ref[:, :, 0])
    with pytest.raises(ValueError):
        hf_module_sampling_inputs(proj, shapes, torch.rand(1, 5, len(LEVELS), 3))


@pytest.mark.parametrize("ref_dim", [2, 4])
def test_host_core_is_the_composition_bit_for_bit(ref_dim):
    value, shapes, proj, ref = make(2, 9, 3, 8, LEVELS, 3, ref_dim, torch.float32, seed=4)
    out = fused_hf_module_core(value, shapes, proj, ref, "zeros", False, level_shapes=LEVELS)
    want = multiscale_deformable_attention(value, shapes, *hf_module_sampling_inputs(proj, shapes, ref), "zeros", False)
    assert torch.equal(out, want)


@pytest.mark.parametrize("ref_dim", [2, 4])
def test_host_core_gradcheck_fp64(ref_dim):
    levels = [(3, 2), (2, 3)]
    value, shapes, proj, ref = make(1, 3, 2, 4, levels, 2, ref_dim, torch.float64, seed=2)
    proj = proj * 0.3
    ref = 0.25 + 0.5 * ref  # keep the samples off the border kinks of the bilinear footprint
    value.requires_grad_(True), proj.requires_grad_(True), ref.requires_grad_(True)
    assert torch.autograd.gradcheck(lambda v, p, r: fused_hf_module_core(v, shapes, p, r, "zeros", False), (value, proj, ref),
                                    eps=1e-6, atol=1e-6, rtol=1e-4)


# ------------------------------------------------------------------------------------------ the HF adapter
def _fused_modules(model):
    from msda_triton_amd.hf_adapter import FusedHFDeformableAttention
    return [m for m in model.modules() if isinstance(m, FusedHFDeformableAttention)]


def test_wrapped_deformable_detr_matches_hf_on_cpu():
    pytest.importorskip("transformers")
    from test_hf_model import WATCHED, _inputs, run_model, tiny_deformable_detr
    from msda_triton_amd.hf_adapter import replace_hf_msda
    model = tiny_deformable_detr()
    x, mask = _inputs("cpu")
    keys = list(model.state_dict().keys())
    params = [id(p) for p in model.parameters()]
    hs0, enc0, g0 = run_model(model, x, mask)
    assert replace_hf_msda(model, fused=True) == 8  # 4 cores swapped + their 4 attention modules wrapped
    assert len(_fused_modules(model)) == 4
    assert list(model.state_dict().keys()) == keys and [id(p) for p in model.parameters()] == params
    assert replace_hf_msda(model, fused=True) == 0  # idempotent
    hs1, enc1, g1 = run_model(model, x, mask)
    torch.testing.assert_close(enc1, enc0, atol=1e-5, rtol=1e-4)
    torch.testing.assert_close(hs1, hs0, atol=1e-5, rtol=1e-4)
    for k in WATCHED:
        err = float((g1[k] - g0[k]).norm() / g0[k].norm().clamp_min(1e-30))
        assert err < 1e-4, (k, err)


def test_wrapped_grounding_dino_matches_hf_on_cpu():
    pytest.importorskip("transformers")
    from test_hf_model import GDINO_WATCHED, _gdino_inputs, run_gdino, tiny_grounding_dino
    from msda_triton_amd.hf_adapter import replace_hf_msda
    model = tiny_grounding_dino()
    inputs = _gdino_inputs("cpu")
    keys = list(model.state_dict().keys())
    hs0, enc0, ref0, g0 = run_gdino(model, inputs)
    assert replace_hf_msda(model, fused=True) == 8
    assert len(_fused_modules(model)) == 4
    assert list(model.state_dict().keys()) == keys
    hs1, enc1, ref1, g1 = run_gdino(model, inputs)
    torch.testing.assert_close(ref1, ref0, atol=1e-5, rtol=1e-4)
    torch.testing.assert_close(enc1, enc0, atol=1e-5, rtol=1e-4)
    torch.testing.assert_close(hs1, hs0, atol=1e-5, rtol=1e-4)
    for k in GDINO_WATCHED:
        err = float((g1[k] - g0[k]).norm() / g0[k].norm().clamp_min(1e-30))
        assert err < 1e-4, (k, err)


def test_adapter_contract_flag_off_and_attention_weights_on_request():
    pytest.importorskip("transformers")
    from test_hf_model import tiny_deformable_detr
    from msda_triton_amd.hf_adapter import replace_hf_msda
    model = tiny_deformable_detr()
    assert replace_hf_msda(model) == 4 and not _fused_modules(model)  # today's count, nothing wrapped
    hf = tiny_deformable_detr()
    attn_hf = hf.encoder.layers[0].self_attn
    assert replace_hf_msda(model, fused=True) == 4  # (the cores were swapped above: only the wrapping is counted now)
    attn = model.encoder.layers[0].self_attn
    assert attn in _fused_modules(model) and attn.return_attention_weights is False
    g = torch.Generator().manual_seed(1)
    levels = [(6, 8), (3, 4), (2, 2), (1, 1)]
    n = sum(h * w for h, w in levels)
    hidden, pos = torch.randn(2, n, 64, generator=g), torch.randn(2, n, 64, generator=g)
    ref = torch.rand(2, n, 4, 2, generator=g)
    mask = torch.ones(2, n, dtype=torch.bool)
    mask[1, -5:] = False
    kw = dict(attention_mask=mask, encoder_hidden_states=hidden, position_embeddings=pos, reference_points=ref,
              spatial_shapes=torch.tensor(levels), spatial_shapes_list=levels, level_start_index=None)
    want, want_w = attn_hf(hidden, **kw)
    out, w = attn(hidden, **kw)
    assert w is None
    torch.testing.assert_close(out, want, atol=1e-5, rtol=1e-4)
    attn.return_attention_weights = True
    out, w = attn(hidden, **kw)
    torch.testing.assert_close(out, want, atol=1e-5, rtol=1e-4)
    torch.testing.assert_close(w, want_w, atol=1e-6, rtol=1e-5)


# ------------------------------------------------------------------------------------------ the C ABI
def test_new_symbols_exist_for_the_eight_suffixes():
    lib = _lib.load()
    suffixes = _lib.DTYPE_SUFFIXES + _lib.FUSED_STORAGE_SUFFIXES
    assert len(suffixes) == 8 and _lib.has_fused_levelref()
    for suf in suffixes:
        for d in ("fwd", "bwd"):
            name = f"msda_{d}_fused_levelref_{suf}"
            assert name in _lib.EXPORTED_SYMBOLS
            assert getattr(lib, name).argtypes == getattr(lib, f"msda_{d}_fused_{suf}").argtypes


def _fused_rows():
    import test_size_guards as sg
    return [r for r in sg.ROWS if sg._applies(r, "fwd_fused") or sg._applies(r, "bwd_fused")]


@pytest.mark.parametrize("row", _fused_rows())
def test_guards_refuse_at_the_uniform_fused_pairs_limits(row):
    """One row per inequality of tests/test_size_guards.py's table, exactly on its limit: the new entry points answer what
    the uniform fused pair answers (MSDA_ERR_TOO_LARGE, before any pointer is read)."""
    import test_size_guards as sg
    lib = _lib.load()
    for family, suffix in (("fwd_fused", "f32"), ("bwd_fused", "f32"), ("fwd_fused", "f32_sbf16"), ("bwd_fused", "f64")):
        if not sg._applies(row, family):
            continue
        es, ves = sg.SIZES[suffix]
        d = sg._isolates(row, family, es, ves)
        host = sg._Host()
        want = sg._call(lib, host, family, suffix, d)
        saved = sg.FAMILIES[family]
        sg.FAMILIES["levelref"] = (saved[0].replace("fused_", "fused_levelref_"),) + saved[1:]
        try:
            got = sg._call(lib, host, "levelref", suffix, d)
        finally:
            del sg.FAMILIES["levelref"]
        assert got == want == sg.TOO_LARGE, (row, family, suffix, got, want, lib.msda_last_error())
