"""Host: the box prologue of transformers' D-FINE / DEIMv2 / RT-DETRv2 attention modules in front of DISCRETE sampling —
`fused_hf_box_core(..., sampling_mode="discrete")` against transformers' own expressions (the box branch of
`DFineMultiscaleDeformableAttention.forward` plus `multi_scale_deformable_attention_v2(method="discrete")`), and
`replace_hf_msda(model, fused=True, discrete=True, fuse_discrete=True)` on tiny random-init models built from their configs (no download):
wrapping counts, state_dict keys, fp64 parity with the unpatched model, the set of parameters without a gradient."""
import pytest
import torch

from msda_triton_amd.functional import fused_hf_box_core
from msda_triton_amd.hf_adapter import FusedHFBoxDeformableAttention, replace_hf_msda

from test_hf_box_fused import make, transformers_box_rule

LEVELS = [(9, 7), (5, 6), (3, 2), (2, 2)]


@pytest.mark.parametrize("offset_scale", [0.5, 0.3])
@pytest.mark.parametrize("counts", [[3, 6, 3], [1, 2, 5, 1]], ids=["3_6_3", "1_2_5_1"])
def test_host_core_is_transformers_discrete_expression(counts, offset_scale):
    pytest.importorskip("transformers")
    from transformers.models.d_fine.modeling_d_fine import multi_scale_deformable_attention_v2 as hf_core
    B, Q, H, D = 2, 37, 4, 8
    value, shapes, proj, ref = make(B, Q, H, D, LEVELS, counts, 11, torch.float64)
    gout = torch.randn(B, Q, H * D, generator=torch.Generator().manual_seed(12), dtype=torch.float64)

    def leaves():
        return [t.clone().requires_grad_(True) for t in (value, proj, ref)]

    v0, p0, r0 = leaves()
    pts, att = transformers_box_rule(p0[..., :2], p0[..., 2], r0, counts, offset_scale)
    want = hf_core(v0, [tuple(s) for s in shapes.tolist()], pts, att, counts, "discrete")  # [B, Q, H * D]
    want.backward(gout)
    v1, p1, r1 = leaves()
    got = fused_hf_box_core(v1, shapes, p1, r1, counts, offset_scale, sampling_mode="discrete")
    assert got.shape == (B, Q, H, D)
    got.flatten(2).backward(gout)
    torch.testing.assert_close(got.flatten(2), want, atol=1e-12, rtol=1e-12)
    torch.testing.assert_close(v1.grad, v0.grad, atol=1e-12, rtol=1e-12)
    torch.testing.assert_close(p1.grad, p0.grad, atol=1e-12, rtol=1e-12)
    assert r1.grad is None  # (the pixel index is an integer: nothing differentiable reaches the box)
    assert bool((p1.grad[..., :2] == 0).all()) and bool((p1.grad[..., 2] != 0).any())
    # "border" / False given explicitly is the same call; [B, Q, 4] boxes too
    again = fused_hf_box_core(value, shapes, proj, ref[:, :, 0], counts, offset_scale, "border", False, sampling_mode="discrete")
    assert torch.equal(again, got.detach())


def test_bad_modes_are_refused():
    counts = [1, 2, 5, 1]
    value, shapes, proj, ref = make(2, 5, 2, 4, LEVELS, counts, 6, torch.float32)
    with pytest.raises(ValueError, match="border"):
        fused_hf_box_core(value, shapes, proj, ref, counts, 0.5, "zeros", False, sampling_mode="discrete")
    with pytest.raises(ValueError, match="border"):
        fused_hf_box_core(value, shapes, proj, ref, counts, 0.5, "border", True, sampling_mode="discrete")
    with pytest.raises(ValueError, match="sampling_mode"):
        fused_hf_box_core(value, shapes, proj, ref, counts, 0.5, sampling_mode="nearest")


def test_probe_and_symbol_list():
    from msda_triton_amd import _lib
    assert _lib.has_fused_hfbox_discrete()
    lib = _lib.load()
    assert len(_lib.HFBOX_DISCRETE_SYMBOLS) == 17 and not set(_lib.HFBOX_DISCRETE_SYMBOLS) & set(_lib.EXPORTED_SYMBOLS)
    for sym in _lib.HFBOX_DISCRETE_SYMBOLS:
        assert getattr(lib, sym) is not None
    header = open(_lib.os.path.join(_lib._HERE, "..", "include", "msda_hip.h")).read()
    assert "msda_fwd_fused_hfbox_discrete_##SUF" in header and "msda_bwd_fused_hfbox_discrete_##SUF" in header


def test_arguments_are_refused_before_any_launch():
    """No GPU here: whatever the entry points answer, they answer from the host checks in front of the first launch."""
    import ctypes
    from msda_triton_amd import _lib
    lib = _lib.load()
    counts9 = (ctypes.c_int32 * 9)(*([1] * 9))
    scale9 = (ctypes.c_float * 9)(*([1.0] * 9))
    one = ctypes.c_void_p(256)  # (never dereferenced: the calls below are refused on their arguments)
    # more than 8 levels: the workspace query says 0; a null level_scale and a count below 1 are argument errors
    assert lib.msda_bwd_fused_hfbox_discrete_workspace_bytes(2, 100, 2, 8, 5, 9, counts9, 4, 4, 0, 0) == 0
    counts3 = (ctypes.c_int32 * 3)(3, 6, 3)
    assert lib.msda_bwd_fused_hfbox_discrete_workspace_bytes(8, 8400, 8, 32, 300, 3, counts3, 4, 4, 0, 0) >= 8 * 300 * 8 * 12 * 3 * 4
    assert lib.msda_fwd_fused_hfbox_discrete_f32(one, one, one, one, one, 2, 100, 2, 8, 5, 3, counts3, None, 0.5, 0, None) == -1
    bad = (ctypes.c_int32 * 3)(3, 0, 3)
    assert lib.msda_fwd_fused_hfbox_discrete_f32(one, one, one, one, one, 2, 100, 2, 8, 5, 3, bad, scale9, 0.5, 0, None) == -1
    assert lib.msda_bwd_fused_hfbox_discrete_f32(one, one, one, one, one, None, None, 2, 100, 2, 8, 5, 3, counts3, scale9, 0.5, 0,
                                                 0, None, 0, None) == -1  # (grad_proj is always produced)


# ------------------------------------------------------------------------------------------ whole models
def tiny(kind, method="discrete"):
    tf = pytest.importorskip("transformers")
    torch.manual_seed(0)
    if kind == "rt_detr_v2":
        if not hasattr(tf, "RTDetrV2Model"):
            pytest.skip("this transformers has no RT-DETRv2")
        return tf.RTDetrV2Model(tf.RTDetrV2Config(num_queries=30, decoder_layers=2, decoder_method=method)).eval()
    if kind == "deimv2" and not hasattr(tf, "Deimv2Model"):
        pytest.skip("this transformers has no DEIMv2")
    cls, cfg = (tf.DFineModel, tf.DFineConfig) if kind == "d_fine" else (tf.Deimv2Model, tf.Deimv2Config)
    return cls(cfg(decoder_n_points=[3, 6, 3], num_queries=30, decoder_layers=2, decoder_method=method)).eval()


def wrapped(model):
    return [m for m in model.modules() if isinstance(m, FusedHFBoxDeformableAttention)]


@pytest.mark.parametrize("kind", ["d_fine", "deimv2", "rt_detr_v2"])
def test_wrapping_counts_and_state_dict(kind):
    model = tiny(kind)
    keys = list(model.state_dict())
    discrete = [m for m in model.modules() if getattr(m, "decoder_method", getattr(m, "method", None)) == "discrete"
                and hasattr(m, "sampling_offsets")]
    assert len(discrete) == 2
    plain = replace_hf_msda(tiny(kind), discrete=True)  # (without `fused`: what it always returned)
    assert replace_hf_msda(model, fused=True) == 0 and wrapped(model) == []  # `fused` alone leaves discrete modules alone
    # ... and so do `fused` and `discrete` together, as they always did (tests/test_hf_box_fused.py): the cores only
    probe = tiny(kind)
    assert replace_hf_msda(probe, discrete=True, fused=True) == plain and wrapped(probe) == []
    assert replace_hf_msda(model, fused=True, discrete=True, fuse_discrete=True) == plain + 2  # ... a wrapper per decoder layer on top
    assert len(wrapped(model)) == 2 and all(m.__dict__.get("_msda_fused_discrete") for m in wrapped(model))
    assert replace_hf_msda(model, fused=True, discrete=True, fuse_discrete=True) == 0
    assert list(model.state_dict()) == keys


def test_tiny_dfine_fused_discrete_matches_hf_on_cpu():
    """The bounds of test_hf_dfine_discrete.test_tiny_discrete_dfine_matches_hf_on_cpu, on the wrapped model."""
    from test_hf_dfine_discrete import _x, run, tiny_dfine
    model = tiny_dfine().double()
    x = _x("cpu").double()
    hs0, g0, none0 = run(model, x)
    assert replace_hf_msda(model, fused=True, discrete=True, fuse_discrete=True) == 4
    assert len(wrapped(model)) == 2
    hs1, g1, none1 = run(model, x)
    torch.testing.assert_close(hs1, hs0, atol=1e-10, rtol=1e-9)
    assert g0.keys() == g1.keys() and len(g0) > 0
    assert none0 == none1 and any("sampling_offsets" in n for n in none1)
    for k in g0:
        torch.testing.assert_close(g1[k], g0[k], atol=1e-9, rtol=1e-7, msg=lambda m: f"{k}: {m}")
