"""GPU: the fused module kernels for per-level reference points and transformers' point rule
(msda_fwd_fused_levelref_ / msda_bwd_fused_levelref_<suffix>) against `hf_module_sampling_inputs` + the plain operator on
the same GPU, through `fused_hf_module_core` and `replace_hf_msda(model, fused=True)`.  Shapes and bounds are
tests/test_gpu_fused_ragged.py's; every level is non-square and every level's reference point is drawn independently, so
a wrong level index or a w / h swap moves samples by whole pixels.  Nothing is masked."""
import zlib

import pytest
import torch

from msda_triton_amd import _ext, _lib, functional
from msda_triton_amd.functional import (KernelTimer, fused_hf_module_core, hf_module_sampling_inputs,
                                        multiscale_deformable_attention)
from test_gpu_fused_ragged import SHAPES, assert_fp32_close, close16, names

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def make(B, Q, H, D, levels, P, ref_dim, seed, dtype=torch.float32):
    g = torch.Generator(device="cpu").manual_seed(seed)
    L = len(levels)
    value = torch.randn(B, sum(h * w for h, w in levels), H, D, generator=g, dtype=dtype)
    proj = torch.randn(B, Q, H, L, P, 3, generator=g, dtype=dtype) * 1.5
    ref = torch.rand(B, Q, L, ref_dim, generator=g, dtype=dtype)
    gout = torch.rand(B, Q, H, D, generator=g, dtype=dtype)
    return [t.to(DEV) for t in (value, torch.tensor(levels), proj, ref, gout)]


def run(fused, value, shapes, proj, ref, gout, pm, ac, level_shapes=None, need_img=True, need_ref=True):
    v = value.detach().clone().requires_grad_(need_img)
    pr, rf = proj.detach().clone().requires_grad_(True), ref.detach().clone().requires_grad_(need_ref)
    if fused:
        out = fused_hf_module_core(v, shapes, pr, rf, pm, ac, level_shapes)
    else:
        pts, att = hf_module_sampling_inputs(pr.to(rf.dtype), shapes, rf)
        out = multiscale_deformable_attention(v, shapes, pts, att, pm, ac, level_shapes=level_shapes)
    out.backward(gout.to(out.dtype))
    return out.detach(), v.grad, pr.grad, rf.grad


@pytest.mark.parametrize("ref_dim", [2, 4])
@pytest.mark.parametrize("P", [3, 4])
@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("pm,ac", [("zeros", False), ("border", True)], ids=["zeros_0", "border_1"])
def test_fused_matches_composition(ref_dim, P, name, pm, ac):
    B, Q, H, D, levels = SHAPES[name]
    c = make(B, Q, H, D, levels, P, ref_dim, zlib.crc32(f"{name}{P}".encode()) + ref_dim)
    with KernelTimer() as kt:
        got = run(True, *c, pm, ac)
    assert names(kt).count("msda_fwd_fused_levelref") == 1 and names(kt).count("msda_bwd_fused_levelref") == 1, names(kt)
    assert tuple(got[3].shape) == (B, Q, len(levels), ref_dim)
    want = run(False, *c, pm, ac)
    assert_fp32_close(got, want)
    assert_fp32_close(run(True, *c, pm, ac), want)  # (no timer: the C++ node where it is built)


@pytest.mark.parametrize("ref_dim", [2, 4])
def test_grad_value_routes(ref_dim):
    """The c2-like shape (sorted grad_value pipeline, LDS-served levels) and a decoder-sized call with the level sizes given
    (single-launch grad_value kernel): grad_value is the uniform pipeline on the points the backward parked."""
    levels = [(64, 48), (32, 24), (16, 12), (8, 6)]
    c = make(4, 10000, 8, 32, levels, 4, ref_dim, 21 + ref_dim)
    got = run(True, *c, "zeros", False)
    info = _lib.last_launch_info()
    assert info["value_path"] == 2 and info["sample_variant"] == 1 and info["sample_lds_level_bytes"] > 0, info
    assert_fp32_close(got, run(False, *c, "zeros", False))
    levels = [(80, 60), (40, 30), (20, 15)]
    c = make(8, 300, 8, 32, levels, 4, ref_dim, 23 + ref_dim)
    got = run(True, *c, "zeros", False, level_shapes=levels)
    assert _lib.last_launch_info()["value_path"] == 1
    assert_fp32_close(got, run(False, *c, "zeros", False, level_shapes=levels))


def test_cpp_node_python_function_and_ctypes_launch_agree_bit_for_bit():
    ext = _ext.load()
    assert ext is not None and hasattr(ext, "msda_fused_levelref"), "the C++ binding is part of the build"
    for ref_dim in (2, 4):
        value, shapes, proj, ref, gout = make(2, 70, 8, 32, SHAPES["d32"][4], 4, ref_dim, 13)
        a = run(True, value, shapes, proj, ref, gout, "zeros", False)  # (no timer, no autocast: the C++ node)
        v, pr, rf = value.clone().requires_grad_(True), proj.clone().requires_grad_(True), ref.clone().requires_grad_(True)
        out = functional._HipFusedHFModuleCoreFunction.apply(v, shapes, pr, rf, "zeros", False, 0)
        out.backward(gout)
        for x, y in zip(a, (out.detach(), v.grad, pr.grad, rf.grad)):
            assert torch.equal(x, y)
        out2 = functional.msda_hip_fwd_fused(value, shapes, proj, ref, "zeros", False, levelref=True)
        gv, gp, gr = functional.msda_hip_bwd_fused(gout, value, shapes, proj, ref, "zeros", False, levelref=True)
        for x, y in zip(a, (out2, gv, gp, gr)):
            assert torch.equal(x, y)


@pytest.mark.parametrize("pm,ac", [("zeros", False), ("zeros", True), ("border", False), ("border", True)])
@pytest.mark.parametrize("ref_dim", [2, 4])
def test_fp64_backward_against_autograd_through_the_prologue(pm, ac, ref_dim):
    c = make(2, 37, 4, 16, [(9, 7), (5, 6), (3, 2)], 3, ref_dim, 5 + ref_dim, torch.float64)
    with KernelTimer() as kt:
        got = run(True, *c, pm, ac)
    assert names(kt).count("msda_fwd_fused_levelref") == 1 and names(kt).count("msda_bwd_fused_levelref") == 1, names(kt)
    for a, b in zip(got, run(False, *c, pm, ac)):
        torch.testing.assert_close(a, b, atol=1e-8, rtol=1e-8)


@pytest.mark.parametrize("sdt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("ref_dim", [2, 4])
def test_storage_variants_match_fp32_on_the_rounded_inputs(sdt, ref_dim):
    levels = [(20, 16), (10, 8), (5, 4)]
    g = torch.Generator(device="cpu").manual_seed(31 + ref_dim)
    B, Q, H, D, P = 2, 90, 4, 32, 4
    value = torch.randn(B, sum(h * w for h, w in levels), H, D, generator=g).to(sdt).to(DEV)
    proj = (torch.randn(B, Q, H, len(levels), P, 3, generator=g) * 1.5).to(sdt).to(DEV)
    ref = torch.rand(B, Q, len(levels), ref_dim, generator=g).to(DEV)
    gout = torch.randn(B, Q, H, D, generator=g).to(sdt).to(DEV)
    shapes = torch.tensor(levels, device=DEV)
    want = run(True, value.float(), shapes, proj.float(), ref, gout.float(), "zeros", False)
    # 16-bit value next to an fp32 projection (_vbf16 / _vf16): the fp32 kernels' numbers on the rounded rows
    with KernelTimer() as kt:
        got = run(True, value, shapes, proj.float(), ref, gout.float(), "zeros", False)
    assert "msda_fwd_fused_levelref" in names(kt) and "msda_bwd_fused_levelref" in names(kt)
    torch.testing.assert_close(got[0], want[0], atol=2e-5, rtol=1e-4)
    close16(got[1], want[1], sdt, "grad_value", scale_tol=3.0)
    torch.testing.assert_close(got[2], want[2], atol=1e-3, rtol=1e-3)
    torch.testing.assert_close(got[3], want[3], atol=1e-3, rtol=1e-3)
    # 16-bit value and projection next to fp32 reference points (_sbf16 / _sf16)
    assert functional.fused_storage_dtypes(value.dtype, proj.dtype, ref.dtype)
    with KernelTimer() as kt:
        out, gv, gp, gr = run(True, value, shapes, proj, ref, gout, "zeros", False)
    assert "msda_fwd_fused_levelref" in names(kt) and "msda_bwd_fused_levelref" in names(kt)
    assert gr.dtype == torch.float32
    close16(out, want[0], sdt, "out")
    close16(gp, want[2], sdt, "grad_proj")
    close16(gv, want[1], sdt, "grad_value", scale_tol=3.0)
    torch.testing.assert_close(gr, want[3], rtol=2e-4, atol=2e-4 * float(want[3].abs().max()))
    # one 16-bit dtype for every tensor (_bf16 / _f16): runs the same kernels' 16-bit instantiation
    with KernelTimer() as kt:
        out, gv, gp, gr = run(True, value, shapes, proj, ref.to(sdt), gout, "zeros", False)
    assert "msda_fwd_fused_levelref" in names(kt) and "msda_bwd_fused_levelref" in names(kt)
    want16 = run(True, value.float(), shapes, proj.float(), ref.to(sdt).float(), gout.float(), "zeros", False)
    close16(out, want16[0], sdt, "out")


def test_frozen_pyramid_and_frozen_reference_points():
    c = make(2, 70, 8, 32, SHAPES["d32"][4], 4, 4, 17)
    with KernelTimer():
        a = run(True, *c, "zeros", False)
        d = run(True, *c, "zeros", False, need_img=False)
        e = run(True, *c, "zeros", False, need_ref=False)
    assert d[1] is None and torch.equal(d[2], a[2]) and torch.equal(d[3], a[3])
    assert e[3] is None and torch.equal(e[2], a[2]) and torch.equal(e[1], a[1])
    f = run(True, *c, "zeros", False, need_img=False, need_ref=False)  # (the C++ node)
    assert f[1] is None and f[3] is None and torch.equal(f[2], a[2])


def test_beyond_the_one_pass_limit_takes_the_composition():
    P = 641
    c = make(1, 6, 2, 8, [(6, 5), (3, 4)], P, 4, 77)
    assert 2 * P > _lib.load().msda_fused_lp_limit(8, 4)
    with KernelTimer() as kt:
        got = run(True, *c, "border", False)
    assert "msda_fwd_fused_levelref" in names(kt) and "msda_fwd" in names(kt)  # (asked, declined, composed)
    assert_fp32_close(got, run(False, *c, "border", False))
    assert_fp32_close(run(True, *c, "border", False), run(False, *c, "border", False))  # (no timer: not the C++ node either)


def test_host_resident_img_shapes_follow_img():
    c = make(2, 19, 3, 8, SHAPES["d8"][4], 4, 2, 3)
    a = fused_hf_module_core(c[0], c[1], c[2], c[3], "zeros", False)
    b = fused_hf_module_core(c[0], c[1].cpu(), c[2], c[3], "zeros", False)
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------ whole models
def test_wrapped_deformable_detr_matches_hf_fp32_and_bf16_autocast():
    pytest.importorskip("transformers")
    from msda_triton_amd.hf_adapter import replace_hf_msda
    from test_hf_model import WATCHED, _inputs, run_model, tiny_deformable_detr
    model = tiny_deformable_detr().to(DEV)
    x, mask = _inputs(DEV)
    hs0, enc0, g0 = run_model(model, x, mask)
    b0 = run_model(model, x, mask, torch.bfloat16)
    assert replace_hf_msda(model, fused=True) == 8
    with KernelTimer() as kt:
        hs1, enc1, g1 = run_model(model, x, mask)
        torch.cuda.synchronize()
    s = kt.summary()
    assert s["msda_fwd_fused_levelref"][0] == 4 and s["msda_bwd_fused_levelref"][0] == 4 and "msda_fwd" not in s, s
    torch.testing.assert_close(enc1, enc0, atol=1e-4, rtol=1e-3)
    torch.testing.assert_close(hs1, hs0, atol=1e-4, rtol=1e-3)
    for k in WATCHED:
        err = float((g1[k] - g0[k]).norm() / g0[k].norm().clamp_min(1e-30))
        assert err < 2e-3, (k, err)
    with KernelTimer() as kt:
        b1 = run_model(model, x, mask, torch.bfloat16)
    assert kt.summary()["msda_fwd_fused_levelref"][0] == 4 and kt.summary()["msda_bwd_fused_levelref"][0] == 4

    def rel(a, b):
        return float((a - b).norm() / b.norm().clamp_min(1e-12))

    noise = rel(b0[0], hs0)
    assert rel(b1[0], b0[0]) < max(3 * noise, 3e-2), (rel(b1[0], b0[0]), noise)
    assert rel(b1[1], b0[1]) < 3e-2
    for k in WATCHED:
        assert torch.isfinite(b1[2][k]).all()
        assert rel(b1[2][k], b0[2][k]) < 0.15, (k, rel(b1[2][k], b0[2][k]))


def test_wrapped_grounding_dino_matches_hf_fp32_and_bf16_autocast(monkeypatch):
    pytest.importorskip("transformers")
    from msda_triton_amd.hf_adapter import replace_hf_msda
    from test_hf_model import GDINO_WATCHED, _gdino_inputs, _PinnedTopk, run_gdino, tiny_grounding_dino
    model = tiny_grounding_dino().to(DEV)
    inputs = _gdino_inputs(DEV)
    hs0, enc0, ref0, g0 = run_gdino(model, inputs)
    pin = _PinnedTopk(monkeypatch)
    pin.record()
    b0 = run_gdino(model, inputs, torch.bfloat16)
    pin.restore()
    assert replace_hf_msda(model, fused=True) == 8
    with KernelTimer() as kt:
        hs1, enc1, ref1, g1 = run_gdino(model, inputs)
        torch.cuda.synchronize()
    s = kt.summary()
    assert s["msda_fwd_fused_levelref"][0] == 4 and s["msda_bwd_fused_levelref"][0] == 4 and "msda_fwd" not in s, s
    torch.testing.assert_close(ref1, ref0, atol=1e-4, rtol=1e-3)
    torch.testing.assert_close(enc1, enc0, atol=1e-4, rtol=1e-3)
    torch.testing.assert_close(hs1, hs0, atol=1e-4, rtol=1e-3)
    for k in GDINO_WATCHED:
        err = float((g1[k] - g0[k]).norm() / g0[k].norm().clamp_min(1e-30))
        assert err < 2e-3, (k, err)
    pin.replay()
    with KernelTimer() as kt:
        b1 = run_gdino(model, inputs, torch.bfloat16)
    pin.restore()
    assert pin.calls == 1 and kt.summary()["msda_fwd_fused_levelref"][0] == 4

    def rel(a, b):
        return float((a - b).norm() / b.norm().clamp_min(1e-12))

    assert rel(b1[1], b0[1]) < 3e-2 and rel(b1[2], b0[2]) < 3e-2
    noise = rel(b0[0], hs0)
    assert rel(b1[0], b0[0]) < max(3 * noise, 3e-2), (rel(b1[0], b0[0]), noise)
    for k in GDINO_WATCHED:
        assert torch.isfinite(b1[3][k]).all()
        assert rel(b1[3][k], b0[3][k]) < 0.2, (k, rel(b1[3][k], b0[3][k]))
