"""GPU: Hugging Face's box rule fused in front of DISCRETE sampling (msda_fwd_fused_hfbox_discrete_ /
msda_bwd_fused_hfbox_discrete_<suffix>) against the composition — `hf_box_sampling_inputs` plus the discrete operator on
the same GPU — through `fused_hf_box_core(..., sampling_mode="discrete")`, the launchers of msda_triton_amd.discrete and
`replace_hf_msda(model, fused=True, discrete=True, fuse_discrete=True)` on a tiny D-FINE.

A wrong scale, a fused multiply-add in the point, a dropped offset_scale or a swapped level moves a sample to ANOTHER pixel:
the pixel-choice tests (exact value rows, one-hot weights) and the parked-point test hold those bit for bit; with the pixels
equal, only the softmax's rounding separates the fused kernels from the composition, which the project's fp32 bounds
(tests/test_gpu_fused_ragged.assert_fp32_close) cover."""
import zlib

import numpy as np
import pytest
import torch

from msda_triton_amd import _ext, _lib, discrete, functional
from msda_triton_amd.functional import (KernelTimer, fused_hf_box_core, hf_box_sampling_inputs,
                                        multiscale_deformable_attention)
from test_gpu_fused_ragged import COUNTS, SHAPES, assert_fp32_close, close16, names
from test_gpu_hf_box_fused import make

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FWD, BWD = "msda_fwd_fused_hfbox_discrete", "msda_bwd_fused_hfbox_discrete"


def composition(v, shapes, pr, rf, counts, scale):
    pts, att = hf_box_sampling_inputs(pr.to(rf.dtype), rf, counts, scale)
    return multiscale_deformable_attention(v, shapes, pts, att, "border", False, points_per_level=counts,
                                           sampling_mode="discrete")


def run(fused, value, shapes, proj, ref, gout, counts, scale=0.5, need_img=True):
    v = value.detach().clone().requires_grad_(need_img)
    pr, rf = proj.detach().clone().requires_grad_(True), ref.detach().clone().requires_grad_(True)
    if fused:
        out = fused_hf_box_core(v, shapes, pr, rf, counts, scale, sampling_mode="discrete")
    else:
        out = composition(v, shapes, pr, rf, counts, scale)
    out.backward(gout.to(out.dtype))
    return out.detach(), v.grad, pr.grad, rf.grad


def only_the_fused_pair(kt):
    n = names(kt)
    return n.count(FWD) == 1 and n.count(BWD) == 1 and not any(k.startswith("msda_fwd") and k != FWD for k in n)


def assert_matches(got, want, check=assert_fp32_close):
    """out, grad_value and the logit slots of grad_proj within `check`; the offset slots exact zeros; no box gradient."""
    assert got[3] is None and (want[3] is None or not bool(want[3].any()))
    assert bool((got[2][..., :2] == 0).all()) and bool((want[2][..., :2] == 0).all())
    check((got[0], got[1], got[2][..., 2]), (want[0], want[1], want[2][..., 2]))


# ------------------------------------------------------------------------------------------ the pixel, exactly
def one_hot_problem(ref, proj_xy, levels, counts, H, dtype):
    """Value rows hold their own pixel index and query q's logits are -30000 except at sample q % S: exp underflows, the
    weights are exactly 1.0 and 0.0, and out IS the index of the pixel sample q % S picks."""
    B, Q = ref.shape[:2]
    S, D = sum(counts), 4
    n = sum(h * w for h, w in levels)
    value = torch.arange(n, dtype=dtype).reshape(1, n, 1, 1).expand(B, n, H, D).contiguous()
    logits = torch.full((B, Q, H, S), -30000.0, dtype=dtype)
    logits[:, torch.arange(Q), :, torch.arange(Q) % S] = 0.0
    proj = torch.cat([proj_xy.to(dtype), logits[..., None]], -1)
    return [t.to(DEV) for t in (value, torch.tensor(levels), proj, ref.to(dtype))]


def assert_same_pixels(value, shapes, proj, ref, counts, scale):
    got = fused_hf_box_core(value, shapes, proj, ref, counts, scale, sampling_mode="discrete")
    want = composition(value, shapes, proj, ref, counts, scale)
    wrong = (got != want).any(-1).nonzero()
    assert wrong.numel() == 0, (len(wrong), wrong[:4].tolist(), got[tuple(wrong[0])], want[tuple(wrong[0])])
    assert torch.equal(got, want)
    assert bool((want == want.round()).all())  # (every row is one pixel's index: the weights were exactly one-hot)
    return got


@pytest.mark.parametrize("scale", [0.5, 0.3])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_pixel_choice_is_exact_on_random_boxes(dtype, scale):
    counts = [3, 6, 3]
    B, Q, H, D, levels = SHAPES["d32"]
    levels = levels[:3]
    g = torch.Generator().manual_seed(71)
    ref = torch.rand(B, 40 * Q, 1, 4, generator=g, dtype=dtype)
    xy = torch.randn(B, 40 * Q, H, sum(counts), 2, generator=g, dtype=dtype) * 1.5
    got = assert_same_pixels(*one_hot_problem(ref, xy, levels, counts, H, dtype), counts, scale)
    assert len(torch.unique(got)) > sum(h * w for h, w in levels) // 2  # (the samples do spread over the pyramid)


def boundary_coords(n, npdt):
    """coordinates on, and one and two ulps either side of, every (k + 0.5) / n boundary of an axis of n pixels (the
    construction of tests/test_discrete_sampling.py::test_gpu_pixel_choice_is_exact, in either precision), the ends and far
    out of range"""
    c = ((np.arange(-1, n + 1, dtype=np.float64) + 0.5) / n).astype(npdt)
    up, dn = np.nextafter(c, npdt(np.inf)), np.nextafter(c, npdt(-np.inf))
    far = np.array([0.0, 1.0, -0.0, 1e30, -1e30, 0.5], dtype=npdt)
    return np.concatenate([c, up, dn, np.nextafter(up, npdt(np.inf)), np.nextafter(dn, npdt(-np.inf)), far])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_pixel_choice_is_exact_on_every_rounding_boundary(dtype):
    """Boxes with w = h = 0: the point is ref.xy exactly.  Every boundary coordinate of every level's axes meets every
    sample slot (query c * S + s carries coordinate pair c and its hot sample is s), so each level rounds each of them."""
    counts = [3, 6, 3]
    levels = SHAPES["d32"][4][:3]
    npdt = np.float32 if dtype == torch.float32 else np.float64
    xs = np.concatenate([boundary_coords(w, npdt) for _, w in levels])
    ys = np.concatenate([boundary_coords(h, npdt) for h, _ in levels])
    n = max(len(xs), len(ys))
    x = np.concatenate([np.resize(xs, n), np.resize(xs, n), np.resize(xs[::-1], n)])
    y = np.concatenate([np.resize(ys, n), np.resize(ys[::-1], n), np.resize(ys, n)])
    S, H = sum(counts), 2
    xy = torch.from_numpy(np.stack([x, y], -1)).repeat_interleave(S, 0)  # [C * S, 2]
    Q = xy.shape[0]
    ref = torch.cat([xy, torch.zeros(Q, 2, dtype=dtype)], -1).reshape(1, Q, 1, 4)
    offsets = torch.randn(1, Q, H, S, 2, generator=torch.Generator().manual_seed(5), dtype=dtype) * 1.5
    got = assert_same_pixels(*one_hot_problem(ref, offsets, levels, counts, H, dtype), counts, 0.5)
    # ... and it is the host formulation's pixel too (an independent check of the composition's side)
    pts = ref[:, :, None, :, :2].expand(1, Q, H, S, 2)
    hot = torch.arange(Q) % S
    start, s0, want = 0, 0, torch.empty(Q, dtype=torch.int64)
    for (h, w), P in zip(levels, counts):
        sel = (hot >= s0) & (hot < s0 + P)
        px, py = pts[0, sel, 0, 0, 0], pts[0, sel, 0, 0, 1]
        ix = torch.clamp(torch.trunc(px * w + 0.5), 0, w - 1).to(torch.int64)
        iy = torch.clamp(torch.trunc(py * h + 0.5), 0, h - 1).to(torch.int64)
        want[sel] = start + iy * w + ix
        start, s0 = start + h * w, s0 + P
    assert torch.equal(got[0, :, 0, 0].cpu().to(torch.int64), want)


# ------------------------------------------------------------------------------------------ parked points and weights
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_parked_points_are_the_host_rule_bit_for_bit_and_the_forward_is_reproducible(dtype):
    counts = [3, 6, 3]
    B, Q, H, D, levels = SHAPES["d32"]
    for scale in (0.5, 0.3):
        value, shapes, proj, ref, gout = make(B, 300, H, D, levels, counts, 41, dtype)
        res = discrete.hf_box_discrete_hip_bwd_fused(gout, value, shapes, proj, ref[:, :, 0], tuple(counts), scale,
                                                     parked_points=True)
        pts, att = hf_box_sampling_inputs(proj, ref, counts, scale)
        assert res[2].dtype == dtype and torch.equal(res[2], pts)
        # the parked weights are the kernel's softmax (exp(l - m) * (1 / sum)): torch's to rounding
        torch.testing.assert_close(res[3], att, atol=0.0, rtol=1e-5 if dtype == torch.float32 else 1e-13)
        a = discrete.hf_box_discrete_hip_fwd_fused(value, shapes, proj, ref[:, :, 0], tuple(counts), scale)
        b = discrete.hf_box_discrete_hip_fwd_fused(value, shapes, proj, ref[:, :, 0], tuple(counts), scale)
        assert torch.equal(a, b)
        # the forward's weights are the parked ones: the discrete operator on the parked buffers gives the forward's sum
        # (same pixels, same weights; the row FMAs run in the same order in both kernels)
        c = discrete.discrete_hip_fwd(value, shapes, res[2], res[3], tuple(counts))
        assert torch.equal(a, c)


# ------------------------------------------------------------------------------------------ fused against composition
@pytest.mark.parametrize("cname", list(COUNTS))
@pytest.mark.parametrize("name", list(SHAPES))
def test_fused_matches_composition(cname, name):
    counts = COUNTS[cname]
    B, Q, H, D, levels = SHAPES[name]
    scale = 0.3 if cname == "1_2_5_1" else 0.5
    c = make(B, Q, H, D, levels, counts, zlib.crc32(f"{name}{cname}".encode()))
    with KernelTimer() as kt:
        got = run(True, *c, counts, scale)
    assert only_the_fused_pair(kt), names(kt)
    want = run(False, *c, counts, scale)
    assert_matches(got, want)
    assert_matches(run(True, *c, counts, scale), want)  # (no timer: the C++ node)
    assert _lib.last_launch_info()["fwd_variant"] == 4 and _lib.last_launch_info()["sample_variant"] == 3


def test_fp64_against_autograd_through_the_prologue():
    """(A double-precision 1 / 3 in the kernel instead of float32(1 / 3) widened moves points by ~1e-8 of a box: pixels.)"""
    counts = [3, 6, 3]
    B, Q, H, D, levels = SHAPES["d8"]
    c = make(B, Q, H, D, levels, counts, 5, torch.float64)
    with KernelTimer() as kt:
        got = run(True, *c, counts, 0.3)
    assert only_the_fused_pair(kt), names(kt)

    def close(a, b):
        for x, y in zip(a, b):
            torch.testing.assert_close(x, y, atol=1e-8, rtol=1e-8)
    assert_matches(got, run(False, *c, counts, 0.3), close)


EDGES = {
    # Q no multiple of the units per workgroup; S one each side of a multiple of the group (G = 8); scalar rows
    "q13_d5_s9": (2, 13, 3, 5, SHAPES["d5"][4], [1, 2, 5, 1]),
    "q70_d32_s16": (2, 70, 8, 32, SHAPES["d32"][4], [2, 4, 6, 4]),
    "d64_s9": (1, 33, 4, 64, SHAPES["d64"][4], [1, 2, 5, 1]),
    "d260_chunks": (1, 5, 1, 260, [(5, 4), (3, 2)], [3, 2]),       # several channel chunks per sample
    "level_1x3": (2, 19, 3, 8, SHAPES["d8"][4], [1, 2, 5, 1]),     # the last level is (1, 3)
    "equal_4_4_4": (2, 70, 8, 32, SHAPES["d32"][4], [4, 4, 4]),
}


@pytest.mark.parametrize("name", list(EDGES))
def test_edge_shapes(name):
    B, Q, H, D, levels, counts = EDGES[name]
    c = make(B, Q, H, D, levels, counts, zlib.crc32(name.encode()))
    with KernelTimer() as kt:
        got = run(True, *c, counts, 0.3)
    assert only_the_fused_pair(kt), names(kt)
    if name == "d260_chunks":
        assert _lib.last_launch_info()["fwd_chunks"] > 1 and _lib.last_launch_info()["sample_chunks"] > 1
    want = run(False, *c, counts, 0.3)
    assert_matches(got, want)
    assert_matches(run(True, *c, counts, 0.3), want)


# ------------------------------------------------------------------------------------------ routes
def test_cpp_node_python_function_and_ctypes_launch_agree_bit_for_bit():
    ext = _ext.load()
    assert ext is not None and hasattr(ext, "box_discrete") and hasattr(ext.box_discrete, "msda_fused_hfbox_discrete"), \
        "the C++ binding is part of the build"
    counts = [3, 6, 3]
    value, shapes, proj, ref, gout = make(2, 70, 8, 32, SHAPES["d32"][4], counts, 13)
    a = run(True, value, shapes, proj, ref, gout, counts, 0.3)  # (no timer, no autocast: the C++ node)
    v, pr = value.clone().requires_grad_(True), proj.clone().requires_grad_(True)
    rf = ref[:, :, 0].clone().requires_grad_(True)
    out = discrete._HipFusedHfBoxDiscreteFunction.apply(v, shapes, pr, rf, tuple(counts), 0.3, 0)
    out.backward(gout)
    assert a[3] is None and rf.grad is None
    for x, y in zip(a[:3], (out.detach(), v.grad, pr.grad)):
        assert torch.equal(x, y)
    out2 = discrete.hf_box_discrete_hip_fwd_fused(value, shapes, proj, ref[:, :, 0], tuple(counts), 0.3)
    gv, gp = discrete.hf_box_discrete_hip_bwd_fused(gout, value, shapes, proj, ref[:, :, 0], tuple(counts), 0.3)
    for x, y in zip(a[:3], (out2, gv, gp)):
        assert torch.equal(x, y)


@pytest.mark.parametrize("sdt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_storage_variants_match_fp32_on_the_rounded_inputs(sdt):
    """Against the fp32 fused discrete kernels on the .float() of the same stored inputs: the same fp32 point, the same pixel
    (a 16-bit composition forms the point in 16 bits and may land on the neighbouring pixel — not the comparison here)."""
    counts = [3, 6, 3]
    levels = [(20, 16), (10, 8), (5, 4)]
    g = torch.Generator(device="cpu").manual_seed(35)
    B, Q, H, D = 2, 90, 4, 32
    value = torch.randn(B, sum(h * w for h, w in levels), H, D, generator=g).to(sdt).to(DEV)
    proj = (torch.randn(B, Q, H, sum(counts), 3, generator=g) * 1.5).to(sdt).to(DEV)
    ref = torch.rand(B, Q, 1, 4, generator=g).to(DEV)
    gout = torch.randn(B, Q, H, D, generator=g).to(sdt).to(DEV)
    shapes = torch.tensor(levels, device=DEV)
    want = run(True, value.float(), shapes, proj.float(), ref, gout.float(), counts)
    # 16-bit value next to an fp32 projection (_vbf16 / _vf16): the fp32 kernels' numbers on the rounded rows
    with KernelTimer() as kt:
        got = run(True, value, shapes, proj.float(), ref, gout.float(), counts)
    assert only_the_fused_pair(kt), names(kt)
    torch.testing.assert_close(got[0], want[0], atol=2e-5, rtol=1e-4)
    close16(got[1], want[1], sdt, "grad_value", scale_tol=3.0)
    torch.testing.assert_close(got[2], want[2], atol=1e-3, rtol=1e-3)
    # 16-bit value and projection next to fp32 boxes (_sbf16 / _sf16)
    assert functional.fused_storage_dtypes(value.dtype, proj.dtype, ref.dtype)
    with KernelTimer() as kt:
        out, gv, gp, gr = run(True, value, shapes, proj, ref, gout, counts)
    assert only_the_fused_pair(kt), names(kt)
    assert gr is None and bool((gp[..., :2] == 0).all())
    close16(out, want[0], sdt, "out")
    close16(gp, want[2], sdt, "grad_proj")
    close16(gv, want[1], sdt, "grad_value", scale_tol=3.0)
    # one 16-bit dtype for every tensor (_bf16 / _f16): the same kernels' 16-bit instantiation, the point still in fp32
    with KernelTimer() as kt:
        out, gv, gp, gr = run(True, value, shapes, proj, ref.to(sdt), gout, counts)
    assert only_the_fused_pair(kt), names(kt)
    want16 = run(True, value.float(), shapes, proj.float(), ref.to(sdt).float(), gout.float(), counts)
    close16(out, want16[0], sdt, "out")
    close16(gp, want16[2], sdt, "grad_proj")
    close16(gv, want16[1], sdt, "grad_value", scale_tol=3.0)


def test_frozen_pyramid_needs_no_workspace(monkeypatch):
    counts = [3, 6, 3]
    value, shapes, proj, ref, gout = make(2, 70, 8, 32, SHAPES["d32"][4], counts, 17)
    args = (gout, value, shapes, proj, ref[:, :, 0], tuple(counts), 0.3)
    gv, gp = discrete.hf_box_discrete_hip_bwd_fused(*args)
    lib = _lib.load()
    asked = []
    real = lib.msda_bwd_fused_hfbox_discrete_workspace_bytes
    monkeypatch.setattr(lib, "msda_bwd_fused_hfbox_discrete_workspace_bytes", lambda *a: asked.append(a) or real(*a))
    with KernelTimer() as kt:
        gv0, gp0 = discrete.hf_box_discrete_hip_bwd_fused(*args, need_img=False)
    assert gv0 is None and not asked and names(kt) == [BWD]
    assert torch.equal(gp0, gp)
    discrete.hf_box_discrete_hip_bwd_fused(*args)
    assert len(asked) == 1
    a = run(True, value, shapes, proj, ref, gout, counts, 0.3)
    d = run(True, value, shapes, proj, ref, gout, counts, 0.3, need_img=False)  # (the C++ node)
    assert d[1] is None and torch.equal(d[0], a[0]) and torch.equal(d[2], a[2]) and torch.equal(a[1], gv)


def test_nine_levels_take_the_composition():
    counts = [1, 2, 1, 3, 1, 2, 1, 1, 2]
    levels = [(6, 5), (5, 4), (4, 4), (4, 3), (3, 3), (3, 2), (2, 2), (2, 1), (1, 1)]
    c = make(2, 21, 3, 8, levels, counts, 78)
    with KernelTimer() as kt:
        got = run(True, *c, counts)
    assert not any("fused_hfbox_discrete" in n for n in names(kt)), names(kt)
    want = run(False, *c, counts)
    for a, b in zip(got[:3], want[:3]):
        assert torch.equal(a, b)
    assert got[3] is None
    for a, b in zip(run(True, *c, counts)[:3], want[:3]):  # (no timer: not the C++ node either)
        assert torch.equal(a, b)
    assert discrete.hf_box_discrete_hip_fwd_fused(c[0], c[1], c[2], c[3][:, :, 0], tuple(counts)) is None


def test_buffer_contract():
    """Both launchers inside tests/guarded_alloc.py's banded, pre-filled allocations: the bands stay intact, every element
    of out, grad_value and grad_proj is written (the backward leaves g_s in grad_proj on the way: nothing of it may stay),
    and the results are those of a plain call."""
    from guarded_alloc import contract_violations
    counts = [1, 2, 5, 1]
    value, shapes, proj, ref, gout = make(2, 13, 3, 5, SHAPES["d5"][4], counts, 23)
    bad, _, _ = contract_violations(
        lambda: discrete.hf_box_discrete_hip_fwd_fused(value, shapes, proj, ref[:, :, 0], tuple(counts), 0.3), 1, DEV)
    assert not bad, bad
    bad, _, _ = contract_violations(
        lambda: discrete.hf_box_discrete_hip_bwd_fused(gout, value, shapes, proj, ref[:, :, 0], tuple(counts), 0.3), 3, DEV,
        names=["grad_value", "grad_proj"])
    assert not bad, bad
    value, shapes, proj, ref, gout = make(2, 70, 8, 32, SHAPES["d32"][4], [3, 6, 3], 24)
    bad, _, _ = contract_violations(
        lambda: discrete.hf_box_discrete_hip_bwd_fused(gout, value.bfloat16(), shapes, proj.bfloat16(), ref[:, :, 0],
                                                       (3, 6, 3), 0.3, need_img=False), 1, DEV, names=["grad_proj"])
    assert not bad, bad  # (16-bit projection: g_s waits as two halves in the offset slots)


# ------------------------------------------------------------------------------------------ whole models
def run_model(model, x, autocast_dtype=None, backward=True):
    """tests/test_gpu_hf_box_fused.py's `run_model` (a loss the decoder can move), plus the parameters left without a
    gradient.  `backward=False`: the hidden state only (a leg that is compared in the forward alone)."""
    model.zero_grad(set_to_none=True)
    ctx = torch.autocast(x.device.type, dtype=autocast_dtype) if autocast_dtype is not None else \
        torch.autocast(x.device.type, enabled=False)
    with ctx, torch.set_grad_enabled(backward):
        out = model(pixel_values=x)
    hs = out.last_hidden_state.float() if autocast_dtype is not None else out.last_hidden_state
    if not backward:
        return hs.detach(), {}, set()
    t = torch.randn(hs.shape, generator=torch.Generator().manual_seed(3)).to(hs.device, hs.dtype)
    (hs * t).mean().backward()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None and n.startswith("decoder.")}
    return hs.detach(), grads, {n for n, p in model.named_parameters() if p.grad is None}


def test_tiny_dfine_fp64_matches_the_unpatched_model():
    """fp64 on the GPU: a point that differs from transformers' in any bit but the softmax's would show as a whole pixel."""
    pytest.importorskip("transformers")
    from msda_triton_amd.hf_adapter import replace_hf_msda
    from test_hf_dfine_discrete import _x, tiny_dfine
    model = tiny_dfine().double().to(DEV)
    x = _x(DEV).double()
    hs0, g0, none0 = run_model(model, x)
    assert replace_hf_msda(model, fused=True, discrete=True, fuse_discrete=True) == 4
    hs1, g1, none1 = run_model(model, x)  # (no timer: the C++ node)
    info = _lib.last_launch_info()
    assert info["fwd_variant"] == 4 and info["sample_variant"] == 3, info
    assert none0 == none1 and any("sampling_offsets" in n for n in none1)
    torch.testing.assert_close(hs1, hs0, atol=1e-8, rtol=1e-7)
    assert g0.keys() == g1.keys() and len(g0) > 0
    for k in g0:
        torch.testing.assert_close(g1[k], g0[k], atol=1e-8, rtol=1e-7, msg=lambda m: f"{k}: {m}")


def test_tiny_dfine_fp32_and_bf16_autocast():
    """Only `rel(hs_fused, hs_unfused_adapter) < max(3 * noise, 3e-2)` here, with `noise` the distance of bf16 autocast from
    fp32 on the unpatched model — NO elementwise fp32 bound: the wrapper's single GEMM and the kernel's softmax differ from
    transformers' in the last bits, and from the second layer on a point within that distance of a rounding boundary
    legitimately lands on the neighbouring pixel.  The elementwise claim is carried by the pixel-choice, parked-point and
    fused-against-composition tests above, where the projection tensor is shared, and by the fp64 model test.

    (Duration: 1.0 s behind another model test in the same process; as the FIRST model test of a process it also pays the
    backbone's one-time fp32 / bf16 convolution set-up, 11 s measured — which tests/test_gpu_hf_box_fused.py's D-FINE case,
    17 s when it is first, paid before this file sorted in front of it.)"""
    pytest.importorskip("transformers")
    from msda_triton_amd.hf_adapter import replace_hf_msda
    from test_hf_dfine import rel
    from test_hf_dfine_discrete import _x, tiny_dfine
    x = _x(DEV)
    plain = tiny_dfine().to(DEV)
    hs0, _, none0 = run_model(plain, x)
    b0, _, _ = run_model(plain, x, torch.bfloat16, backward=False)
    noise = rel(b0, hs0)
    unfused = tiny_dfine().to(DEV)
    assert replace_hf_msda(unfused, discrete=True) == 2
    fused = tiny_dfine().to(DEV)
    assert replace_hf_msda(fused, fused=True, discrete=True, fuse_discrete=True) == 4
    layers = 2
    for dt in (None, torch.bfloat16):
        hsu, _, _ = run_model(unfused, x, dt, backward=False)
        with KernelTimer() as kt:
            hsf, gf, nonef = run_model(fused, x, dt)
            torch.cuda.synchronize()
        s = kt.summary()
        assert s[FWD][0] == layers and s[BWD][0] == layers, s
        assert not any(k.startswith("msda_fwd") and k != FWD for k in s), s
        assert torch.isfinite(hsf).all() and all(torch.isfinite(g).all() for g in gf.values()) and len(gf) > 0
        assert nonef == none0
        print(f"autocast {dt}: rel(fused, unfused adapter) {rel(hsf, hsu):.3e}, noise {noise:.3e}")
        assert rel(hsf, hsu) < max(3 * noise, 3e-2), (dt, rel(hsf, hsu), noise)
