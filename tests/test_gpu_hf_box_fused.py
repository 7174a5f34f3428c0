"""GPU: the fused module kernels for Hugging Face's box rule with per-level point counts
(msda_fwd_fused_hfbox_ / msda_bwd_fused_hfbox_<suffix>) against `hf_box_sampling_inputs` + the ragged operator on the same
GPU, through `fused_hf_box_core` and `replace_hf_msda(model, fused=True)` on D-FINE, DEIMv2 and RT-DETRv2.  Shapes, counts
and bounds are tests/test_gpu_fused_ragged.py's.  A box per query with w, h in (0, 1): a wrong level's scale or a dropped
offset_scale moves samples by whole pixels.  Nothing is masked."""
import zlib

import pytest
import torch

from msda_triton_amd import _ext, functional, ragged
from msda_triton_amd.functional import (KernelTimer, fused_hf_box_core, hf_box_sampling_inputs,
                                        multiscale_deformable_attention)
from test_gpu_fused_ragged import COUNTS, SHAPES, assert_fp32_close, close16, names

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def make(B, Q, H, D, levels, counts, seed, dtype=torch.float32):
    g = torch.Generator(device="cpu").manual_seed(seed)
    levels = levels[:len(counts)]
    value = torch.randn(B, sum(h * w for h, w in levels), H, D, generator=g, dtype=dtype)
    proj = torch.randn(B, Q, H, sum(counts), 3, generator=g, dtype=dtype) * 1.5
    ref = torch.rand(B, Q, 1, 4, generator=g, dtype=dtype)
    gout = torch.rand(B, Q, H, D, generator=g, dtype=dtype)
    return [t.to(DEV) for t in (value, torch.tensor(levels), proj, ref, gout)]


def run(fused, value, shapes, proj, ref, gout, pm, ac, counts, scale=0.5, level_shapes=None, need_img=True, need_ref=True):
    v = value.detach().clone().requires_grad_(need_img)
    pr, rf = proj.detach().clone().requires_grad_(True), ref.detach().clone().requires_grad_(need_ref)
    if fused:
        out = fused_hf_box_core(v, shapes, pr, rf, counts, scale, pm, ac, level_shapes)
    else:
        pts, att = hf_box_sampling_inputs(pr.to(rf.dtype), rf, counts, scale)
        out = multiscale_deformable_attention(v, shapes, pts, att, pm, ac, level_shapes=level_shapes, points_per_level=counts)
    out.backward(gout.to(out.dtype))
    return out.detach(), v.grad, pr.grad, rf.grad


def only_the_fused_pair(kt):
    n = names(kt)
    return n.count("msda_fwd_fused_hfbox") == 1 and n.count("msda_bwd_fused_hfbox") == 1 and \
        not any(k.startswith("msda_fwd") and k != "msda_fwd_fused_hfbox" for k in n)


@pytest.mark.parametrize("scale", [0.5, 0.3])
@pytest.mark.parametrize("cname", list(COUNTS))
@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("pm,ac", [("zeros", False), ("border", True)], ids=["zeros_0", "border_1"])
def test_fused_matches_composition(scale, cname, name, pm, ac):
    counts = COUNTS[cname]
    B, Q, H, D, levels = SHAPES[name]
    c = make(B, Q, H, D, levels, counts, zlib.crc32(f"{name}{cname}".encode()) + int(scale * 10))
    with KernelTimer() as kt:
        got = run(True, *c, pm, ac, counts, scale)
    assert only_the_fused_pair(kt), names(kt)
    assert tuple(got[3].shape) == (B, Q, 1, 4)
    want = run(False, *c, pm, ac, counts, scale)
    assert_fp32_close(got, want)
    assert_fp32_close(run(True, *c, pm, ac, counts, scale), want)  # (no timer: the C++ node)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_parked_sampling_points_are_the_host_rule_bit_for_bit(dtype):
    """The points the backward leaves for the grad_value passes (re-formed in phase 3 from the parked `o * s_l` by the
    forward's operations) against `hf_box_sampling_inputs` on the same GPU."""
    counts = [3, 6, 3]
    B, Q, H, D, levels = SHAPES["d32"]
    for scale in (0.5, 0.3):
        value, shapes, proj, ref, gout = make(B, 300, H, D, levels, counts, 41, dtype)
        res = ragged.hf_box_hip_bwd_fused(gout, value, shapes, proj, ref[:, :, 0], "zeros", False, tuple(counts), scale,
                                          parked_points=True)
        pts, _ = hf_box_sampling_inputs(proj, ref, counts, scale)
        assert res[3].dtype == dtype and torch.equal(res[3], pts)


@pytest.mark.parametrize("pm,ac", [("zeros", False), ("zeros", True), ("border", False), ("border", True)])
def test_fp64_backward_against_autograd_through_the_prologue(pm, ac):
    """(A double-precision 1 / 3 in the kernel instead of float32(1 / 3) widened misses this at ~1e-8.)"""
    counts = [3, 6, 3]
    B, Q, H, D, levels = SHAPES["d8"]
    c = make(B, Q, H, D, levels, counts, 5, torch.float64)
    with KernelTimer() as kt:
        got = run(True, *c, pm, ac, counts, 0.3)
    assert only_the_fused_pair(kt), names(kt)
    for a, b in zip(got, run(False, *c, pm, ac, counts, 0.3)):
        torch.testing.assert_close(a, b, atol=1e-8, rtol=1e-8)


def test_cpp_node_python_function_and_ctypes_launch_agree_bit_for_bit():
    ext = _ext.load()
    assert ext is not None and hasattr(ext, "msda_fused_hfbox"), "the C++ binding is part of the build"
    counts = [3, 6, 3]
    value, shapes, proj, ref, gout = make(2, 70, 8, 32, SHAPES["d32"][4], counts, 13)
    a = run(True, value, shapes, proj, ref, gout, "zeros", False, counts, 0.3)  # (no timer, no autocast: the C++ node)
    v, pr = value.clone().requires_grad_(True), proj.clone().requires_grad_(True)
    rf = ref[:, :, 0].clone().requires_grad_(True)
    out = ragged._HipFusedHfBoxCoreFunction.apply(v, shapes, pr, rf, "zeros", False, tuple(counts), 0.3, 0)
    out.backward(gout)
    for x, y in zip(a, (out.detach(), v.grad, pr.grad, rf.grad[:, :, None])):
        assert torch.equal(x, y)
    out2 = ragged.hf_box_hip_fwd_fused(value, shapes, proj, ref[:, :, 0], "zeros", False, tuple(counts), 0.3)
    gv, gp, gr = ragged.hf_box_hip_bwd_fused(gout, value, shapes, proj, ref[:, :, 0], "zeros", False, tuple(counts), 0.3)
    for x, y in zip(a, (out2, gv, gp, gr[:, :, None])):
        assert torch.equal(x, y)


@pytest.mark.parametrize("sdt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_storage_variants_match_fp32_on_the_rounded_inputs(sdt):
    counts = [3, 6, 3]
    levels = [(20, 16), (10, 8), (5, 4)]
    g = torch.Generator(device="cpu").manual_seed(35)
    B, Q, H, D = 2, 90, 4, 32
    value = torch.randn(B, sum(h * w for h, w in levels), H, D, generator=g).to(sdt).to(DEV)
    proj = (torch.randn(B, Q, H, sum(counts), 3, generator=g) * 1.5).to(sdt).to(DEV)
    ref = torch.rand(B, Q, 1, 4, generator=g).to(DEV)
    gout = torch.randn(B, Q, H, D, generator=g).to(sdt).to(DEV)
    shapes = torch.tensor(levels, device=DEV)
    want = run(True, value.float(), shapes, proj.float(), ref, gout.float(), "zeros", False, counts)
    # 16-bit value next to an fp32 projection (_vbf16 / _vf16): the fp32 kernels' numbers on the rounded rows
    with KernelTimer() as kt:
        got = run(True, value, shapes, proj.float(), ref, gout.float(), "zeros", False, counts)
    assert only_the_fused_pair(kt), names(kt)
    torch.testing.assert_close(got[0], want[0], atol=2e-5, rtol=1e-4)
    close16(got[1], want[1], sdt, "grad_value", scale_tol=3.0)
    torch.testing.assert_close(got[2], want[2], atol=1e-3, rtol=1e-3)
    torch.testing.assert_close(got[3], want[3], atol=1e-3, rtol=1e-3)
    # 16-bit value and projection next to fp32 boxes (_sbf16 / _sf16)
    assert functional.fused_storage_dtypes(value.dtype, proj.dtype, ref.dtype)
    with KernelTimer() as kt:
        out, gv, gp, gr = run(True, value, shapes, proj, ref, gout, "zeros", False, counts)
    assert only_the_fused_pair(kt), names(kt)
    assert gr.dtype == torch.float32
    close16(out, want[0], sdt, "out")
    close16(gp, want[2], sdt, "grad_proj")
    close16(gv, want[1], sdt, "grad_value", scale_tol=3.0)
    torch.testing.assert_close(gr, want[3], rtol=2e-4, atol=2e-4 * float(want[3].abs().max()))
    # one 16-bit dtype for every tensor (_bf16 / _f16): the same kernels' 16-bit instantiation
    with KernelTimer() as kt:
        out, gv, gp, gr = run(True, value, shapes, proj, ref.to(sdt), gout, "zeros", False, counts)
    assert only_the_fused_pair(kt), names(kt)
    want16 = run(True, value.float(), shapes, proj.float(), ref.to(sdt).float(), gout.float(), "zeros", False, counts)
    close16(out, want16[0], sdt, "out")


def test_frozen_pyramid_and_frozen_reference_points():
    counts = [3, 6, 3]
    c = make(2, 70, 8, 32, SHAPES["d32"][4], counts, 17)
    with KernelTimer():
        a = run(True, *c, "zeros", False, counts)
        d = run(True, *c, "zeros", False, counts, need_img=False)
        e = run(True, *c, "zeros", False, counts, need_ref=False)
    assert d[1] is None and torch.equal(d[2], a[2]) and torch.equal(d[3], a[3])
    assert e[3] is None and torch.equal(e[2], a[2]) and torch.equal(e[1], a[1])
    f = run(True, *c, "zeros", False, counts, need_img=False, need_ref=False)  # (the C++ node)
    assert f[1] is None and f[3] is None and torch.equal(f[2], a[2])


def test_beyond_the_limits_takes_the_composition():
    # S = 1281 samples per unit do not fit one LDS pass
    counts = [640, 641]
    c = make(1, 6, 2, 8, [(6, 6), (3, 3)], counts, 77)
    assert not ragged.fused_ragged_limits_ok(8, 4, counts)
    with KernelTimer() as kt:
        got = run(True, *c, "border", False, counts, 0.3)
    assert "msda_fwd_fused_hfbox" in names(kt)  # (asked, declined: nothing was launched by that call)
    want = run(False, *c, "border", False, counts, 0.3)
    assert_fp32_close(got, want)
    assert_fp32_close(run(True, *c, "border", False, counts, 0.3), want)  # (no timer: not the C++ node either)
    # nine levels: beyond the fused kernels' level scan
    counts = [1, 2, 1, 3, 1, 2, 1, 1, 2]
    levels = [(6, 5), (5, 4), (4, 4), (4, 3), (3, 3), (3, 2), (2, 2), (2, 1), (1, 1)]
    c = make(2, 21, 3, 8, levels, counts, 78)
    assert not ragged.fused_ragged_limits_ok(8, 4, counts)
    with KernelTimer() as kt:
        got = run(True, *c, "zeros", False, counts)
    assert "msda_fwd_fused_hfbox" in names(kt)
    want = run(False, *c, "zeros", False, counts)
    assert_fp32_close(got, want)
    assert_fp32_close(run(True, *c, "zeros", False, counts), want)


def test_equal_counts_run_the_box_kernels():
    counts = [4, 4, 4]
    B, Q, H, D, levels = SHAPES["d32"]
    c = make(B, Q, H, D, levels, counts, 9)
    with KernelTimer() as kt:
        got = run(True, *c, "zeros", False, counts, 0.3)
    assert names(kt) == ["msda_fwd_fused_hfbox", "msda_bwd_fused_hfbox"], names(kt)
    want = run(False, *c, "zeros", False, counts, 0.3)
    assert_fp32_close(got, want)
    assert_fp32_close(run(True, *c, "zeros", False, counts, 0.3), want)


def test_host_resident_img_shapes_follow_img():
    counts = [3, 6, 3]
    c = make(*SHAPES["d8"][:4], SHAPES["d8"][4], counts, 3)
    a = fused_hf_box_core(c[0], c[1], c[2], c[3], counts)
    b = fused_hf_box_core(c[0], c[1].cpu(), c[2], c[3], counts)
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------ whole models
def run_model(model, x, autocast_dtype=None):
    """tests/test_hf_dfine.py's `run` (the decoder's last hidden state and its parameter gradients) under a loss that the
    decoder can move: the mean of the hidden state times a fixed standard-normal tensor.  `run`'s own loss, the mean square
    of the hidden state, is constant behind a final norm with unit weight (every row of RMSNorm's output has mean square 1
    up to its epsilon), so its decoder gradients are what cancellation leaves of zero."""
    model.zero_grad(set_to_none=True)
    ctx = torch.autocast(x.device.type, dtype=autocast_dtype) if autocast_dtype is not None else \
        torch.autocast(x.device.type, enabled=False)
    with ctx:
        out = model(pixel_values=x)
    hs = out.last_hidden_state.float()
    t = torch.randn(hs.shape, generator=torch.Generator().manual_seed(3)).to(hs.device)
    (hs * t).mean().backward()
    grads = {n: p.grad.detach().float().clone() for n, p in model.named_parameters()
             if p.grad is not None and n.startswith("decoder.")}
    return hs.detach(), grads


@pytest.mark.parametrize("kind", ["d_fine", "deimv2", "rt_detr_v2"])
def test_wrapped_models_match_transformers_fp32_and_bf16_autocast(kind):
    """Tiny models wrapped with `fused=True` against transformers' own forward and backward, at tests/test_hf_dfine.py's GPU
    bounds (hidden states atol 1e-4 / rtol 1e-3, decoder gradients rel < 5e-2; bf16 autocast: its noise-relative bound).

    The gradients are those of `run_model`'s loss above.  Under the mean-square loss this test first had, the gradient that
    enters DEIMv2's final RMSNorm (norm 2.3e-2) leaves it with norm 1.7e-8, and in fp64 on the host a change of the image by
    1e-10 moved that remainder by 1.8e-2 relative and the worst decoder parameter gradient by 5.5e-3 (1e-8: 4.7e-2): the
    comparison was of noise, and transformers' fp32 model differed from itself by 4.7e-2 between two runs on an MI355X.
    Under this loss the same 1e-10 moves the worst decoder gradient by 3.4e-8 in fp64 (D-FINE 1.2e-10, RT-DETRv2 7.7e-11),
    and 1e-7 moves it by 1.7e-6 in fp32, so the 5e-2 bound now measures the wrapper.  Measured on an MI355X in two runs,
    fp32, worst decoder gradient against transformers: D-FINE 3.0e-7 / 3.0e-7, DEIMv2 1.2e-6 / 1.2e-6, RT-DETRv2 3.1e-6 /
    9.9e-7."""
    pytest.importorskip("transformers")
    from msda_triton_amd.hf_adapter import replace_hf_msda
    from test_hf_box_fused import tiny, x128
    from test_hf_dfine import rel
    model = tiny(kind).to(DEV)
    x = x128(DEV)
    hs0, g0 = run_model(model, x)
    b0, gb0 = run_model(model, x, torch.bfloat16)
    layers = 2
    assert replace_hf_msda(model, fused=True) == (layers if kind == "rt_detr_v2" else 2 * layers)
    with KernelTimer() as kt:
        hs1, g1 = run_model(model, x)
        torch.cuda.synchronize()
    s = kt.summary()
    assert s["msda_fwd_fused_hfbox"][0] == layers and s["msda_bwd_fused_hfbox"][0] == layers, s
    assert not any(k.startswith("msda_fwd") and k != "msda_fwd_fused_hfbox" for k in s), s
    torch.testing.assert_close(hs1, hs0, atol=1e-4, rtol=1e-3)
    assert g0.keys() == g1.keys() and len(g0) > 0
    with KernelTimer() as kt:
        b1, gb1 = run_model(model, x, torch.bfloat16)
    s = kt.summary()
    assert s["msda_fwd_fused_hfbox"][0] == layers and s["msda_bwd_fused_hfbox"][0] == layers, s
    noise = rel(b0, hs0)  # the yardstick: how far bf16 autocast itself is from fp32
    assert rel(b1, b0) < max(3 * noise, 3e-2), (rel(b1, b0), noise)
    for k in gb0:
        assert torch.isfinite(gb1[k]).all(), k
        assert rel(gb1[k], gb0[k]) < 0.15 or float(gb0[k].norm()) < 1e-6, (k, rel(gb1[k], gb0[k]))
    worst = max(g0, key=lambda k: rel(g1[k], g0[k]) if float(g0[k].norm()) >= 1e-6 else 0.0)
    print(f"{kind}: worst fp32 decoder gradient {worst}: rel {rel(g1[worst], g0[worst]):.3e}")
    for k in g0:  # (fp32 round-off is amplified by the decoder: tests/test_hf_dfine.py)
        assert rel(g1[k], g0[k]) < 5e-2 or float(g0[k].norm()) < 1e-6, (k, rel(g1[k], g0[k]))
