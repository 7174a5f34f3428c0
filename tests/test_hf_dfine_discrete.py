"""D-FINE with ``decoder_method="discrete"`` through ``replace_hf_msda(model, discrete=True)``: a tiny random-init
DFineModel from its config (no download), the adapter's discrete core against transformers' own
``multi_scale_deformable_attention_v2(method="discrete")`` — on the host in fp64 and on the GPU (the discrete kernels) in
fp32 and under bf16 autocast, at the tolerances of tests/test_hf_dfine.py."""
import pytest
import torch

transformers = pytest.importorskip("transformers")
try:
    from transformers import DFineConfig, DFineModel
except ImportError:  # pragma: no cover - older transformers
    pytest.skip("this transformers has no D-FINE", allow_module_level=True)


def tiny_dfine():
    torch.manual_seed(0)
    return DFineModel(DFineConfig(decoder_n_points=[3, 6, 3], num_queries=30, decoder_layers=2,
                                  decoder_method="discrete")).eval()


def run(model, x, autocast_dtype=None):
    model.zero_grad(set_to_none=True)
    ctx = torch.autocast(x.device.type, dtype=autocast_dtype) if autocast_dtype is not None else \
        torch.autocast(x.device.type, enabled=False)
    with ctx:
        out = model(pixel_values=x)
    hs = out.last_hidden_state.float()
    hs.pow(2).mean().backward()
    grads = {n: p.grad.detach().float().clone() for n, p in model.named_parameters()
             if p.grad is not None and n.startswith("decoder.")}
    no_grad = {n for n, p in model.named_parameters() if p.grad is None}
    return hs.detach(), grads, no_grad


def _x(dev):
    g = torch.Generator().manual_seed(1)
    return torch.randn(1, 3, 128, 128, generator=g).to(dev)


def rel(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-12))


def test_discrete_patching_is_opt_in():
    from msda_triton_amd.hf_adapter import ms_deformable_attn_core_v2, replace_hf_msda
    model = tiny_dfine()
    assert replace_hf_msda(model) == 0            # today's behaviour: discrete modules are left alone
    assert replace_hf_msda(model, discrete=True) == 2
    cores = [m.ms_deformable_attn_core for m in model.modules() if hasattr(m, "ms_deformable_attn_core")]
    assert len(cores) == 2 and all(c is ms_deformable_attn_core_v2 for c in cores)
    assert replace_hf_msda(model, discrete=True) == 0  # (already patched)


def test_tiny_discrete_dfine_matches_hf_on_cpu():
    from msda_triton_amd.hf_adapter import replace_hf_msda
    model = tiny_dfine().double()
    x = _x("cpu").double()
    hs0, g0, none0 = run(model, x)
    assert replace_hf_msda(model) == 0
    assert replace_hf_msda(model, discrete=True) == 2
    hs1, g1, none1 = run(model, x)
    torch.testing.assert_close(hs1, hs0, atol=1e-10, rtol=1e-9)
    assert g0.keys() == g1.keys() and len(g0) > 0
    assert none0 == none1  # (the sampling offsets of the last layer ... keep grad None exactly as unpatched)
    for k in g0:
        torch.testing.assert_close(g1[k], g0[k], atol=1e-9, rtol=1e-7, msg=lambda m: f"{k}: {m}")


def test_core_v2_serves_both_methods():
    from msda_triton_amd import hf_adapter
    from transformers.models.d_fine.modeling_d_fine import multi_scale_deformable_attention_v2 as hf_core
    g = torch.Generator().manual_seed(3)
    v = torch.randn(2, 16 + 4, 2, 4, generator=g, dtype=torch.float64)
    loc = torch.rand(2, 3, 2, 5, 2, generator=g, dtype=torch.float64) * 1.6 - 0.3
    att = torch.rand(2, 3, 2, 5, generator=g, dtype=torch.float64)
    shapes = [(4, 4), (2, 2)]
    for method in ("default", "discrete"):
        got = hf_adapter.ms_deformable_attn_core_v2(v, shapes, loc, att, [2, 3], method)
        ref = hf_core(v, shapes, loc, att, [2, 3], method)
        torch.testing.assert_close(got, ref, atol=1e-12, rtol=1e-12)
    with pytest.raises(ValueError, match="discrete"):
        hf_adapter.ms_deformable_attn_core_v2(v, shapes, loc, att, [2, 3], "nearest")


@pytest.mark.gpu
def test_tiny_discrete_dfine_matches_hf_on_gpu_fp32():
    from msda_triton_amd import _lib
    from msda_triton_amd.hf_adapter import replace_hf_msda
    dev = "cuda:0"
    model = tiny_dfine().to(dev)
    x = _x(dev)
    hs0, g0, none0 = run(model, x)
    assert replace_hf_msda(model, discrete=True) == 2
    hs1, g1, none1 = run(model, x)
    assert _lib.last_launch_info()["fwd_variant"] == 3  # the discrete kernel served the decoder
    torch.testing.assert_close(hs1, hs0, atol=1e-4, rtol=1e-3)
    assert g0.keys() == g1.keys() and len(g0) > 0 and none0 == none1
    for k in g0:  # (fp32 round-off is amplified by the decoder: tests/test_hf_dfine.py)
        assert rel(g1[k], g0[k]) < 5e-2 or float(g0[k].norm()) < 1e-6, (k, rel(g1[k], g0[k]))


@pytest.mark.gpu
def test_tiny_discrete_dfine_matches_hf_on_gpu_bf16_autocast():
    from msda_triton_amd.hf_adapter import replace_hf_msda
    dev = "cuda:0"
    model = tiny_dfine().to(dev)
    x = _x(dev)
    hs0, g0, _ = run(model, x, torch.bfloat16)
    hs_fp32, _, _ = run(model, x)  # the yardstick: how far bf16 autocast itself is from fp32
    assert replace_hf_msda(model, discrete=True) == 2
    hs1, g1, _ = run(model, x, torch.bfloat16)
    noise = rel(hs0, hs_fp32)
    assert rel(hs1, hs0) < max(3 * noise, 3e-2), (rel(hs1, hs0), noise)
    for k in g0:
        assert torch.isfinite(g1[k]).all(), k
        assert rel(g1[k], g0[k]) < 0.15 or float(g0[k].norm()) < 1e-6, (k, rel(g1[k], g0[k]))
