"""Host: the box prologue of transformers' D-FINE / DEIMv2 / RT-DETRv2 attention modules —
`functional.hf_box_sampling_inputs` against the expression of `modeling_d_fine.py` (torch.equal), `fused_hf_box_core` on
host tensors against the composition, and `replace_hf_msda(model, fused=True)` on tiny random-init models built from
their configs (no download): wrapping counts, state_dict keys, fp64 parity with transformers' own forward, fallbacks."""
import pytest
import torch

from msda_triton_amd import hf_adapter
from msda_triton_amd.functional import (fused_hf_box_core, hf_box_level_scale, hf_box_sampling_inputs,
                                        multiscale_deformable_attention)
from msda_triton_amd.hf_adapter import FusedHFBoxDeformableAttention, replace_hf_msda

from test_gpu_fused_ragged import SHAPES  # (importing it needs no GPU; its tests do)

COUNTS = {"3_6_3": [3, 6, 3], "1_2_5_1": [1, 2, 5, 1], "4_4_4": [4, 4, 4]}
D5 = SHAPES["d5"]


def transformers_box_rule(sampling_offsets, logits, reference_points, num_points_list, offset_scale):
    """DFineMultiscaleDeformableAttention.forward, the lines between the two projections and the core (boxes):
    `sampling_offsets` [B, Q, H, S, 2], `logits` [B, Q, H, S], `reference_points` [B, Q, 1, 4]."""
    num_points_scale = [1 / n for n in num_points_list for _ in range(n)]
    num_points_scale = torch.tensor(num_points_scale, dtype=torch.float32)  # (the module's buffer)
    attention_weights = torch.nn.functional.softmax(logits, dim=-1)
    num_points_scale = num_points_scale.to(dtype=sampling_offsets.dtype).unsqueeze(-1)
    offset = sampling_offsets * num_points_scale * reference_points[:, :, None, :, 2:] * offset_scale
    sampling_locations = reference_points[:, :, None, :, :2] + offset
    return sampling_locations, attention_weights


def make(B, Q, H, D, levels, counts, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    levels = levels[:len(counts)]
    value = torch.randn(B, sum(h * w for h, w in levels), H, D, generator=g, dtype=dtype)
    proj = torch.randn(B, Q, H, sum(counts), 3, generator=g, dtype=dtype) * 1.5
    ref = torch.rand(B, Q, 1, 4, generator=g, dtype=dtype)
    return value, torch.tensor(levels), proj, ref


@pytest.mark.parametrize("offset_scale", [0.5, 0.3])
@pytest.mark.parametrize("cname", list(COUNTS))
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_rule_is_transformers_expression_bit_for_bit(dtype, cname, offset_scale):
    counts = COUNTS[cname]
    _, _, proj, ref = make(2, 257, 4, 8, [(9, 7), (5, 6), (3, 2), (2, 2)], counts, 3, dtype)
    pts, att = hf_box_sampling_inputs(proj, ref, counts, offset_scale)
    want_pts, want_att = transformers_box_rule(proj[..., :2], proj[..., 2], ref, counts, offset_scale)
    assert pts.shape == (2, 257, 4, sum(counts), 2) and att.shape == (2, 257, 4, sum(counts))
    assert torch.equal(pts, want_pts) and torch.equal(att, want_att)
    pts3, att3 = hf_box_sampling_inputs(proj, ref[:, :, 0], counts, offset_scale)  # [B, Q, 4]
    assert torch.equal(pts3, want_pts) and torch.equal(att3, want_att)


def test_scale_is_the_fp32_rounded_one_in_fp64():
    """transformers widens float32(1 / P_l); the same rule written with 1 / P_l in double gives other bits whenever P_l is
    not a power of two — here (3 and 6) at every point."""
    counts = [3, 6, 3]
    _, _, proj, ref = make(2, 257, 4, 8, [(9, 7), (5, 6), (3, 2)], counts, 4, torch.float64)
    pts, _ = hf_box_sampling_inputs(proj, ref, counts, 0.5)
    scale = torch.tensor([1 / n for n in counts for _ in range(n)], dtype=torch.float64).unsqueeze(-1)
    exact = ref[:, :, None, :, :2] + proj[..., :2] * scale * ref[:, :, None, :, 2:] * 0.5
    assert not torch.equal(pts, exact)
    assert bool((pts != exact).any(-1).all())
    assert hf_box_level_scale(counts) == tuple(float(torch.tensor(1 / n, dtype=torch.float32)) for n in counts)
    assert hf_box_level_scale(counts)[0] != 1 / 3


@pytest.mark.parametrize("cname", list(COUNTS))
def test_host_route_is_the_composition_bit_for_bit(cname):
    counts = COUNTS[cname]
    B, Q, H, D, levels = D5
    value, shapes, proj, ref = make(B, Q, H, D, levels, counts, 5, torch.float32)
    for pm, ac, scale in (("zeros", False, 0.5), ("border", True, 0.3)):
        got = fused_hf_box_core(value, shapes, proj, ref, counts, scale, pm, ac)
        pts, att = hf_box_sampling_inputs(proj, ref, counts, scale)
        want = multiscale_deformable_attention(value, shapes, pts, att, pm, ac, points_per_level=counts)
        assert got.shape == (B, Q, H, D) and torch.equal(got, want)
    assert torch.equal(fused_hf_box_core(value, shapes, proj, ref[:, :, 0], counts), fused_hf_box_core(value, shapes, proj, ref, counts))


def test_bad_arguments_are_refused():
    value, shapes, proj, ref = make(*D5[:4], D5[4], [1, 2, 5, 1], 6, torch.float32)
    with pytest.raises(ValueError, match="reference_points"):
        fused_hf_box_core(value, shapes, proj, ref[..., :2], [1, 2, 5, 1])
    with pytest.raises(ValueError, match="reference_points"):
        fused_hf_box_core(value, shapes, proj, ref.expand(-1, -1, 4, -1), [1, 2, 5, 1])
    with pytest.raises(ValueError, match="points_per_level"):
        fused_hf_box_core(value, shapes, proj, ref, [1, 2, 5, 2])
    with pytest.raises(ValueError):
        hf_box_sampling_inputs(proj, ref, [1, 2, 5])


def test_gradcheck_fp64():
    counts = [1, 2, 5, 1]
    B, Q, H, D, levels = D5
    value, shapes, proj, ref = make(B, Q, H, D, levels, counts, 7, torch.float64)
    ref = 0.25 + 0.5 * ref  # (samples spread over the levels, few of them on a pixel boundary's kink)
    proj.requires_grad_(True)
    ref.requires_grad_(True)
    torch.autograd.gradcheck(lambda p, r: fused_hf_box_core(value, shapes, p, r, counts, 0.3, "border", True), (proj, ref),
                             eps=1e-6, atol=1e-5, rtol=1e-4, nondet_tol=0.0)


# ------------------------------------------------------------------------------------------ whole models
transformers = pytest.importorskip("transformers")


def tiny(kind, method="default"):
    import transformers as tf
    torch.manual_seed(0)
    if kind == "rt_detr_v2":
        return tf.RTDetrV2Model(tf.RTDetrV2Config(num_queries=30, decoder_layers=2, decoder_method=method)).eval()
    cls, cfg = (tf.DFineModel, tf.DFineConfig) if kind == "d_fine" else (tf.Deimv2Model, tf.Deimv2Config)
    return cls(cfg(decoder_n_points=[3, 6, 3], num_queries=30, decoder_layers=2, decoder_method=method)).eval()


def wrapped(model):
    return [m for m in model.modules() if isinstance(m, FusedHFBoxDeformableAttention)]


def x128(dev="cpu"):
    g = torch.Generator().manual_seed(1)
    return torch.randn(1, 3, 128, 128, generator=g).to(dev)


def run_model(model, x, autocast_dtype=None):
    """tests/test_hf_dfine.py's `run`: the decoder's last hidden state and its parameter gradients."""
    from test_hf_dfine import run
    return run(model, x, autocast_dtype)


@pytest.mark.parametrize("kind", ["d_fine", "deimv2"])
def test_wrapping_counts_and_state_dict(kind):
    model = tiny(kind)
    keys = list(model.state_dict())
    params = [id(p) for p in model.parameters()]
    assert replace_hf_msda(tiny(kind)) == 2  # (without `fused`: what it always returned)
    assert replace_hf_msda(model, fused=True) == 2 + 2  # a core and a wrapper per decoder layer
    assert len(wrapped(model)) == 2
    assert replace_hf_msda(model, fused=True) == 0
    assert list(model.state_dict()) == keys and [id(p) for p in model.parameters()] == params
    assert all(type(m).__name__.startswith("Fused") and type(m).__mro__[3].__name__.endswith("MultiscaleDeformableAttention")
               for m in wrapped(model))


def test_rt_detr_v2_decoder_modules_are_wrapped():
    model = tiny("rt_detr_v2")
    keys = list(model.state_dict())
    assert replace_hf_msda(tiny("rt_detr_v2")) == 0
    assert replace_hf_msda(model, fused=True) == 2 and len(wrapped(model)) == 2
    assert all(hasattr(m, "value_proj") and hasattr(m, "output_proj") for m in wrapped(model))
    assert replace_hf_msda(model, fused=True) == 0 and list(model.state_dict()) == keys


def test_discrete_and_foreign_scale_modules_are_not_wrapped():
    model = tiny("d_fine", "discrete")
    assert replace_hf_msda(model, fused=True) == 0 and not wrapped(model)
    assert replace_hf_msda(model, discrete=True, fused=True) == 2 and not wrapped(model)  # (the discrete cores only)
    model = tiny("d_fine")
    mods = [m for m in model.modules() if hasattr(m, "num_points_scale")]
    with torch.no_grad():
        mods[0].num_points_scale[4] = 0.2  # (what a loaded checkpoint could carry)
    assert replace_hf_msda(model, fused=True) == 2 + 1
    assert wrapped(model) == [mods[1]]
    model = tiny("rt_detr_v2")
    mods = [m for m in model.modules() if hasattr(m, "n_points_scale")]
    with torch.no_grad():
        mods[1].n_points_scale.mul_(2.0)
    assert replace_hf_msda(model, fused=True) == 1 and wrapped(model) == [mods[0]]


@pytest.mark.parametrize("kind", ["d_fine", "deimv2", "rt_detr_v2"])
def test_wrapped_model_matches_transformers_in_fp64(kind, monkeypatch):
    model = tiny(kind).double()
    x = x128().double()
    hs0, g0 = run_model(model, x)
    assert replace_hf_msda(model, fused=True) == (2 if kind == "rt_detr_v2" else 4)
    calls = []
    real = hf_adapter.fused_hf_box_core
    monkeypatch.setattr(hf_adapter, "fused_hf_box_core", lambda *a, **k: calls.append(a[4]) or real(*a, **k))
    hs1, g1 = run_model(model, x)
    assert calls == [[4, 4, 4]] * 2 if kind == "rt_detr_v2" else calls == [[3, 6, 3]] * 2, calls
    torch.testing.assert_close(hs1, hs0, atol=1e-10, rtol=1e-9)
    assert g0.keys() == g1.keys() and len(g0) > 0
    for k in g0:
        torch.testing.assert_close(g1[k], g0[k], atol=1e-9, rtol=1e-7, msg=lambda m: f"{k}: {m}")


def _module_inputs(mod, B=2, Q=7, levels=((4, 5), (3, 2), (2, 2)), ref_dim=4, ref_len=1):
    g = torch.Generator().manual_seed(11)
    d = mod.sampling_offsets.in_features
    hidden = torch.randn(B, Q, d, generator=g)
    enc = torch.randn(B, sum(h * w for h, w in levels), d, generator=g)
    ref = torch.rand(B, Q, ref_len, ref_dim, generator=g)
    return dict(hidden_states=hidden, encoder_hidden_states=enc, reference_points=ref,
                spatial_shapes=torch.tensor(levels), spatial_shapes_list=[tuple(s) for s in levels])


@pytest.mark.parametrize("kind", ["d_fine", "rt_detr_v2"])
def test_fallbacks_run_the_original_forward_and_return_attention_weights(kind, monkeypatch):
    import copy
    model = tiny(kind)
    plain = copy.deepcopy(model)
    replace_hf_msda(model, fused=True)
    mod = wrapped(model)[0]
    orig = [m for m in plain.modules() if type(m).__name__.endswith("MultiscaleDeformableAttention")][0]
    calls = []
    real = hf_adapter.fused_hf_box_core
    monkeypatch.setattr(hf_adapter, "fused_hf_box_core", lambda *a, **k: calls.append(1) or real(*a, **k))
    kw = _module_inputs(mod)
    S = mod.sampling_offsets.out_features // (2 * mod.n_heads)
    out, att = mod(**kw)
    want, want_att = orig(**kw)
    assert att is None and calls == [1]
    torch.testing.assert_close(out, want, atol=1e-5, rtol=1e-4)
    # attention weights asked for: the original forward, bit for bit the unwrapped module over the same core
    replace_hf_msda(plain)
    want, want_att = orig(**kw)
    for how in ("kwarg", "flag"):
        if how == "flag":
            mod.return_attention_weights = True
        out, att = mod(**kw, **({"output_attentions": True} if how == "kwarg" else {}))
        assert calls == [1] and att is not None and att.shape == (2, 7, mod.n_heads, S)
        assert torch.equal(out, want) and torch.equal(att, want_att)
    mod.return_attention_weights = False
    # a reference-point axis longer than 1
    kw4 = _module_inputs(mod, ref_len=S)
    out, att = mod(**kw4)
    want, want_att = orig(**kw4)
    assert calls == [1] and torch.equal(out, want) and torch.equal(att, want_att)
    # 2-d reference points: transformers' own 2-d branches do not broadcast for these modules' sample axis (D-FINE's with
    # unequal counts, RT-DETRv2's [B, Q, H, L * P, 2] offsets against a per-level normaliser), so only the route is checked
    seen = []
    monkeypatch.setattr(type(orig), "forward", lambda self, *a, **k: seen.append(k["reference_points"].shape[-1]) or (None, "w"))
    assert mod(**_module_inputs(mod, ref_dim=2)) == (None, "w") and seen == [2] and calls == [1]


def test_positional_arguments_follow_the_wrapped_class():
    model = tiny("d_fine")
    replace_hf_msda(model, fused=True)
    mod = wrapped(model)[0]
    kw = _module_inputs(mod)
    out, att = mod(**kw)
    pos, att2 = mod(kw["hidden_states"], None, kw["reference_points"], kw["encoder_hidden_states"], kw["spatial_shapes"],
                    kw["spatial_shapes_list"])  # D-FINE's order: reference_points before encoder_hidden_states
    assert att is None and att2 is None and torch.equal(out, pos)
