"""Key-aware deformable attention on the host: the PyTorch formulation and the module against the float64 reference
(key_aware_cases.py), forward and all four gradients, at the seeds and tolerances the GPU tests use."""
import pytest
import torch

import key_aware_cases as kc
from msda_triton_amd import KeyAwareDeformableAttention, key_aware_deformable_attention
from test_gpu_parity import BWD_TOL, FWD_TOL

F32, F64 = torch.float32, torch.float64


@pytest.mark.parametrize("pm,ac", kc.MODES)
@pytest.mark.parametrize("dtype", [F32, F64])
def test_host_path_meets_the_reference(pm, ac, dtype):
    inputs, want = kc.case(dtype=dtype, pm=pm, ac=ac)
    got = kc.run(key_aware_deformable_attention, inputs, kc.BASE_LEVELS, pm, ac, dtype, "cpu")
    kc.assert_close(got, want, FWD_TOL[dtype], BWD_TOL[dtype])


def test_gradcheck_float64():
    inputs, _ = kc.case(B=1, H=2, Q=3, D=4, levels=((3, 2), (2, 2)), P=2, dtype=F64, seed=3, pm="zeros")
    leaves = [inputs[n].clone().requires_grad_(True) for n in ("query", "key", "value", "points")]
    shapes = torch.tensor(((3, 2), (2, 2)))
    fn = lambda q, k, v, p: key_aware_deformable_attention(q, k, v, shapes, p, "zeros", False)  # noqa: E731
    assert torch.autograd.gradcheck(fn, leaves, eps=1e-6, atol=1e-6)


def test_attention_rows_sum_to_one_and_one_sample_is_the_sampled_value():
    levels = ((4, 4),)
    inputs, want = kc.case(levels=levels, P=1, dtype=F64, seed=1)
    got = kc.run(key_aware_deformable_attention, inputs, levels, "border", False, F64, "cpu")
    kc.assert_close(got, want, FWD_TOL[F64], BWD_TOL[F64])
    assert torch.equal(got["attn"], torch.ones_like(got["attn"]))
    assert got["grad_query"].abs().max() <= 1e-12 and got["grad_key"].abs().max() <= 1e-12
    _, attn = key_aware_deformable_attention(*[kc.case()[0][n].float() for n in ("query", "key", "value")],
                                             torch.tensor(kc.BASE_LEVELS), kc.case()[0]["points"].float(), return_attention=True)
    torch.testing.assert_close(attn.sum((-1, -2)), torch.ones(attn.shape[:3]), atol=1e-6, rtol=0)


def test_module_meets_the_reference():
    torch.manual_seed(0)
    E, H, L, P = 12, 3, len(kc.BASE_LEVELS), 2
    mod = KeyAwareDeformableAttention(E, H, L, P, "zeros", False).double()
    assert not hasattr(mod, "attention_weights") and mod.sampling_offsets.bias.abs().max() == P
    torch.nn.init.normal_(mod.sampling_offsets.weight, std=0.3)
    I = sum(h * w for h, w in kc.BASE_LEVELS)  # noqa: E741
    img, queries, ref = torch.randn(2, I, E, dtype=F64), torch.randn(2, 5, E, dtype=F64), torch.rand(2, 5, 2, dtype=F64)
    shapes = torch.tensor(kc.BASE_LEVELS)
    leaves = [img.requires_grad_(True), queries.requires_grad_(True)]
    out = mod(img, shapes, queries, ref)
    q, k, v = (lin(x).reshape(2, -1, H, E // H) for lin, x in ((mod.query_proj, queries), (mod.key_proj, img), (mod.value_proj, img)))
    points = ref[:, :, None, None, None, :] + mod.sampling_offsets(queries).reshape(2, 5, H, L, P, 2) / shapes[:, None, :]
    want = mod.output_proj(kc.reference(q, k, v, kc.BASE_LEVELS, points, "zeros", False, (E // H) ** -0.5)[0].reshape(2, 5, E))
    torch.testing.assert_close(out, want, **FWD_TOL[F64])
    wrt = leaves + list(mod.parameters())
    for got, ref_g in zip(torch.autograd.grad(out.sum(), wrt), torch.autograd.grad(want.sum(), wrt)):
        torch.testing.assert_close(got, ref_g, **BWD_TOL[F64])


@pytest.mark.parametrize("change", ["padding", "key_shape", "points_shape", "shapes", "scale", "ref_dim", "heads"])
def test_rejected_arguments_raise_value_error(change):
    inputs, _ = kc.case()
    q, k, v, p = (inputs[n].float() for n in ("query", "key", "value", "points"))
    shapes, kw = torch.tensor(kc.BASE_LEVELS), {}
    if change == "padding":
        kw["padding_mode"] = "reflection"
    elif change == "key_shape":
        k = k[:, :-1]
    elif change == "points_shape":
        p = p[..., :1]
    elif change == "shapes":
        shapes = shapes[:-1]
    elif change == "scale":
        kw["scale"] = float("nan")
    with pytest.raises(ValueError):
        if change == "heads":
            KeyAwareDeformableAttention(10, 3, 2, 2)
        elif change == "ref_dim":
            KeyAwareDeformableAttention(12, 3, 3, 2)(torch.randn(2, 42, 12), shapes, torch.randn(2, 5, 12), torch.rand(2, 5, 4))
        else:
            key_aware_deformable_attention(q, k, v, shapes, p, **kw)
