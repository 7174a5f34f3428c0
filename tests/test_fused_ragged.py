"""CPU-only: per-level point counts in the module core and the nn.Module — the host formulation
(`ragged_module_sampling_inputs`), `fused_module_core(..., points_per_level=)` on host tensors, the module with
`num_points=[3, 6, 3]`, and the C ABI's new declarations."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

from msda_triton_amd import MultiscaleDeformableAttention
from msda_triton_amd.functional import fused_module_core, module_sampling_inputs, multiscale_deformable_attention
from msda_triton_amd.ragged import ragged_module_sampling_inputs

LEVELS = [(7, 5), (4, 6), (2, 3)]  # non-square: the (h, w) order of the 2-d rule matters


def _inputs(counts, ref_dim, dtype=torch.float64, B=2, Q=5, H=3, D=4, levels=LEVELS, seed=0):
    g = torch.Generator().manual_seed(seed)
    S = sum(counts)
    value = torch.randn(B, sum(h * w for h, w in levels), H, D, generator=g, dtype=dtype)
    proj = torch.randn(B, Q, H, S, 3, generator=g, dtype=dtype) * 1.5
    ref = torch.rand(B, Q, ref_dim, generator=g, dtype=dtype)
    return value, torch.tensor(levels), proj, ref


@pytest.mark.parametrize("ref_dim", [2, 4])
def test_equal_counts_are_the_uniform_prologue_on_a_view(ref_dim):
    _, shapes, proj, ref = _inputs([3, 3, 3], ref_dim, torch.float32)
    B, Q, H, S, _ = proj.shape
    pts, att = ragged_module_sampling_inputs(proj, shapes, ref, [3, 3, 3])
    pts_u, att_u = module_sampling_inputs(proj.reshape(B, Q, H, 3, 3, 3), shapes, ref)
    assert pts.shape == (B, Q, H, S, 2) and att.shape == (B, Q, H, S)
    torch.testing.assert_close(pts, pts_u.reshape(B, Q, H, S, 2), atol=0, rtol=0)
    torch.testing.assert_close(att, att_u.reshape(B, Q, H, S), atol=0, rtol=0)


@pytest.mark.parametrize("ref_dim", [2, 4])
@pytest.mark.parametrize("counts", [[3, 6, 3], [1, 2, 5]])
def test_unequal_counts_match_a_per_sample_loop(ref_dim, counts):
    _, shapes, proj, ref = _inputs(counts, ref_dim)
    B, Q, H, S, _ = proj.shape
    pts, att = ragged_module_sampling_inputs(proj, shapes, ref, counts)
    level = [l for l, p in enumerate(counts) for _ in range(p)]
    want_pts, want_att = torch.empty(B, Q, H, S, 2, dtype=torch.float64), torch.empty(B, Q, H, S, dtype=torch.float64)
    for b in range(B):
        for q in range(Q):
            for h in range(H):
                logits = proj[b, q, h, :, 2]
                e = (logits - logits.max()).exp()
                want_att[b, q, h] = e / e.sum()
                for s in range(S):
                    l = level[s]
                    ox, oy = proj[b, q, h, s, 0], proj[b, q, h, s, 1]
                    if ref_dim == 2:
                        want_pts[b, q, h, s, 0] = ref[b, q, 0] + ox / LEVELS[l][0]
                        want_pts[b, q, h, s, 1] = ref[b, q, 1] + oy / LEVELS[l][1]
                    else:
                        want_pts[b, q, h, s, 0] = ref[b, q, 0] + ox * ref[b, q, 2] / (2 * counts[l])
                        want_pts[b, q, h, s, 1] = ref[b, q, 1] + oy * ref[b, q, 3] / (2 * counts[l])
    torch.testing.assert_close(pts, want_pts, atol=1e-12, rtol=1e-12)
    torch.testing.assert_close(att, want_att, atol=1e-12, rtol=1e-12)
    torch.testing.assert_close(att.sum(-1), torch.ones(B, Q, H, dtype=torch.float64), atol=1e-12, rtol=0)


@pytest.mark.parametrize("pm,ac", [("zeros", False), ("zeros", True), ("border", False), ("border", True)])
@pytest.mark.parametrize("ref_dim", [2, 4])
def test_host_core_is_the_composition_and_passes_gradcheck(pm, ac, ref_dim):
    counts = [2, 3, 1]
    value, shapes, proj, ref = _inputs(counts, ref_dim, B=1, Q=2, H=2, D=3, levels=[(3, 4), (2, 3), (2, 2)], seed=3)
    proj = proj * 0.2  # (stay off the bilinear kinks: gradcheck differentiates numerically)
    ref = ref * 0.5 + 0.25
    out = fused_module_core(value, shapes, proj, ref, pm, ac, points_per_level=counts)
    pts, att = ragged_module_sampling_inputs(proj, shapes, ref, counts)
    want = multiscale_deformable_attention(value, shapes, pts, att, pm, ac, points_per_level=counts)
    torch.testing.assert_close(out, want, atol=0, rtol=0)
    v, p, r = (t.clone().requires_grad_(True) for t in (value, proj, ref))
    assert torch.autograd.gradcheck(lambda a, b, c: fused_module_core(a, shapes, b, c, pm, ac, points_per_level=counts),
                                    (v, p, r), eps=1e-6, atol=1e-5, rtol=1e-4, nondet_tol=0.0)


def test_core_validation_errors():
    value, shapes, proj, ref = _inputs([3, 6, 3], 4)
    with pytest.raises(ValueError, match="2 entries"):
        fused_module_core(value, shapes, proj, ref, "zeros", False, points_per_level=[6, 6])
    with pytest.raises(ValueError, match="at least 1"):
        fused_module_core(value, shapes, proj, ref, "zeros", False, points_per_level=[3, 9, 0])
    with pytest.raises(ValueError, match="sums to 11"):
        fused_module_core(value, shapes, proj, ref, "zeros", False, points_per_level=[3, 5, 3])
    with pytest.raises(ValueError, match=r"\[B,N,H,S,3\]"):
        fused_module_core(value, shapes, proj[..., :2], ref, "zeros", False, points_per_level=[3, 6, 3])
    with pytest.raises(ValueError, match="either 2 or 4"):
        fused_module_core(value, shapes, proj, ref[..., :3], "zeros", False, points_per_level=[3, 6, 3])


def test_module_with_per_level_counts_on_host_tensors():
    torch.manual_seed(0)
    m = MultiscaleDeformableAttention(32, 32, 3, 4, [3, 6, 3], "zeros", False)
    assert m.query_input_proj.weight.shape == (4 * 12 * 3, 32)
    shapes = torch.tensor(LEVELS)
    img = torch.randn(2, sum(h * w for h, w in LEVELS), 32, requires_grad=True)
    q, ref = torch.randn(2, 9, 32, requires_grad=True), torch.rand(2, 9, 4)
    out = m(img, shapes, q, ref)
    assert out.shape == (2, 9, 32)
    out.square().sum().backward()
    for name, prm in m.named_parameters():
        assert prm.grad is not None and bool(prm.grad.abs().sum() > 0), name
    assert img.grad is not None and q.grad is not None
    pts, att = m.sampling_inputs(shapes, q, ref)
    assert pts.shape == (2, 9, 4, 12, 2) and att.shape == (2, 9, 4, 12)
    # 2-d reference points too
    assert m(img, shapes, q, ref[..., :2]).shape == (2, 9, 32)


def test_module_equal_counts_is_the_int_module():
    torch.manual_seed(1)
    a = MultiscaleDeformableAttention(32, 32, 3, 4, 4, "border", True)
    b = MultiscaleDeformableAttention(32, 32, 3, 4, [4, 4, 4], "border", True)
    assert b.num_points == 4 and b.points_per_level is None
    b.load_state_dict(a.state_dict())
    shapes = torch.tensor(LEVELS)
    img, q = torch.randn(2, sum(h * w for h, w in LEVELS), 32), torch.randn(2, 9, 32)
    for ref in (torch.rand(2, 9, 4), torch.rand(2, 9, 2)):
        torch.testing.assert_close(a(img, shapes, q, ref), b(img, shapes, q, ref), atol=0, rtol=0)


def test_module_validation_errors():
    with pytest.raises(ValueError, match="2 entries"):
        MultiscaleDeformableAttention(32, 32, 3, 4, [3, 6], "zeros", False)
    with pytest.raises(ValueError, match="at least 1"):
        MultiscaleDeformableAttention(32, 32, 3, 4, [3, 0, 3], "zeros", False)
    m = MultiscaleDeformableAttention(32, 32, 3, 4, [3, 6, 3], "zeros", False)
    img, q = torch.randn(1, sum(h * w for h, w in LEVELS), 32), torch.randn(1, 2, 32)
    with pytest.raises(ValueError, match="either 2 or 4"):
        m(img, torch.tensor(LEVELS), q, torch.rand(1, 2, 3))


def test_header_declares_and_library_exports_the_fused_ragged_entry_points():
    from msda_triton_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    text = open(os.path.join(ROOT, "include", "msda_hip.h")).read()
    assert re.search(r"#define\s+MSDA_ABI_VERSION\s+12\b", text)
    assert "msda_fwd_fused_ragged_##SUF" in text and "msda_bwd_fused_ragged_##SUF" in text
    assert "msda_bwd_fused_ragged_workspace_bytes" in text
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for suf in ("f32", "f16", "bf16", "f64", "f32_vbf16", "f32_vf16", "f32_sbf16", "f32_sf16"):
        for d in ("fwd", "bwd"):
            name = f"msda_{d}_fused_ragged_{suf}"
            assert name in _lib.EXPORTED_SYMBOLS
            assert getattr(lib, name) is not None
    assert _lib.has_fused_ragged()
    handle = _lib.load()
    arr = (ctypes.c_int32 * 3)(3, 6, 3)
    # host arithmetic only: a decoder-sized call takes the single-launch grad_value kernel — the workspace is the parked
    # points and weights alone (3 elements per sample, rounded up to 256 bytes)
    got = handle.msda_bwd_fused_ragged_workspace_bytes(8, 8400, 8, 32, 300, 3, arr, 4, 4, 81 * 81, 0)
    assert got == (8 * 300 * 8 * 12 * 3 * 4 + 255) // 256 * 256
    bad = (ctypes.c_int32 * 3)(3, 0, 3)
    assert handle.msda_bwd_fused_ragged_workspace_bytes(8, 8400, 8, 32, 300, 3, bad, 4, 4, 0, 0) == 0
    # argument checks run before anything touches a device: a count below 1 is MSDA_ERR_BAD_ARG
    assert handle.msda_fwd_fused_ragged_f32(None, None, None, None, None, 1, 10, 1, 8, 1, 3, bad, 4, 1, 0, 0, None) == -1
