"""D-FINE (per-level point counts, decoder_n_points = [3, 6, 3]) through ``replace_hf_msda``: a tiny random-init
DFineModel from its config (no download), with the adapter against transformers' own ``multi_scale_deformable_attention_v2``
core — on the host (per-level grid_sample) and on the GPU (the ragged kernels), fp32 and under bf16 autocast."""
import pytest
import torch

transformers = pytest.importorskip("transformers")
try:
    from transformers import DFineConfig, DFineModel
except ImportError:  # pragma: no cover - older transformers
    pytest.skip("this transformers has no D-FINE", allow_module_level=True)


def tiny_dfine(method="default"):
    torch.manual_seed(0)
    return DFineModel(DFineConfig(decoder_n_points=[3, 6, 3], num_queries=30, decoder_layers=2,
                                  decoder_method=method)).eval()


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
    return hs.detach(), grads


def _x(dev):
    g = torch.Generator().manual_seed(1)
    return torch.randn(1, 3, 128, 128, generator=g).to(dev)


def test_replace_counts_default_decoders_and_leaves_discrete_alone():
    from msda_triton_amd.hf_adapter import ms_deformable_attn_core, replace_hf_msda
    model = tiny_dfine()
    assert replace_hf_msda(model) == 2  # one core per decoder layer
    cores = [m.ms_deformable_attn_core for m in model.modules() if hasattr(m, "ms_deformable_attn_core")]
    assert len(cores) == 2 and all(c is ms_deformable_attn_core for c in cores)
    assert replace_hf_msda(model) == 0  # (already patched)
    discrete = tiny_dfine("discrete")
    before = [m.ms_deformable_attn_core for m in discrete.modules() if hasattr(m, "ms_deformable_attn_core")]
    assert replace_hf_msda(discrete) == 0
    after = [m.ms_deformable_attn_core for m in discrete.modules() if hasattr(m, "ms_deformable_attn_core")]
    assert after == before


def rel(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-12))


def test_tiny_dfine_matches_hf_on_cpu():
    """In fp64: D-FINE's decoder amplifies fp32 round-off in its parameter gradients (the host adapter against
    transformers' own core: up to 1.3 % relative in fp32, nothing at fp64), so the host comparison is made where the two
    formulations must agree to the last digits."""
    from msda_triton_amd.hf_adapter import replace_hf_msda
    model = tiny_dfine().double()
    x = _x("cpu").double()
    hs0, g0 = run(model, x)
    assert replace_hf_msda(model) == 2
    hs1, g1 = run(model, x)
    torch.testing.assert_close(hs1, hs0, atol=1e-10, rtol=1e-9)
    assert g0.keys() == g1.keys() and len(g0) > 0
    for k in g0:
        torch.testing.assert_close(g1[k], g0[k], atol=1e-9, rtol=1e-7, msg=lambda m: f"{k}: {m}")


def test_core_caches_the_shapes_tensor():
    from msda_triton_amd import hf_adapter
    v = torch.randn(1, 16 + 4, 2, 4)
    loc, att = torch.rand(1, 3, 2, 5, 2), torch.rand(1, 3, 2, 5)
    a = hf_adapter.ms_deformable_attn_core(v, [(4, 4), (2, 2)], loc, att, [2, 3])
    t = hf_adapter._shapes_tensor([(4, 4), (2, 2)], v.device)
    assert hf_adapter._shapes_tensor([[4, 4], [2, 2]], v.device) is t
    assert a.shape == (1, 3, 8)
    with pytest.raises(ValueError, match="default"):
        hf_adapter.ms_deformable_attn_core(v, [(4, 4), (2, 2)], loc, att, [2, 3], "discrete")


@pytest.mark.gpu
def test_tiny_dfine_matches_hf_on_gpu_fp32():
    from msda_triton_amd.hf_adapter import replace_hf_msda
    dev = "cuda:0"
    model = tiny_dfine().to(dev)
    x = _x(dev)
    hs0, g0 = run(model, x)
    assert replace_hf_msda(model) == 2
    hs1, g1 = run(model, x)
    torch.testing.assert_close(hs1, hs0, atol=1e-4, rtol=1e-3)
    assert g0.keys() == g1.keys() and len(g0) > 0
    for k in g0:  # (fp32 round-off is amplified by the decoder: see test_tiny_dfine_matches_hf_on_cpu)
        assert rel(g1[k], g0[k]) < 5e-2 or float(g0[k].norm()) < 1e-6, (k, rel(g1[k], g0[k]))


@pytest.mark.gpu
def test_tiny_dfine_matches_hf_on_gpu_bf16_autocast():
    from msda_triton_amd.hf_adapter import replace_hf_msda
    dev = "cuda:0"
    model = tiny_dfine().to(dev)
    x = _x(dev)
    hs0, g0 = run(model, x, torch.bfloat16)
    hs_fp32, _ = run(model, x)  # the yardstick: how far bf16 autocast itself is from fp32
    assert replace_hf_msda(model) == 2
    hs1, g1 = run(model, x, torch.bfloat16)
    noise = rel(hs0, hs_fp32)
    assert rel(hs1, hs0) < max(3 * noise, 3e-2), (rel(hs1, hs0), noise)
    for k in g0:
        assert torch.isfinite(g1[k]).all(), k
        assert rel(g1[k], g0[k]) < 0.15 or float(g0[k].norm()) < 1e-6, (k, rel(g1[k], g0[k]))
