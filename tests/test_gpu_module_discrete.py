"""GPU: the reference module's rule fused in front of DISCRETE sampling (msda_fwd_fused_discrete_ /
msda_bwd_fused_discrete_<suffix>) through `fused_module_core(..., sampling_mode="discrete", fuse_discrete=True)`, the
launchers of msda_triton_amd.discrete and `MultiscaleDeformableAttention(sampling_mode="discrete")`.

The yardstick for the PIXEL is formed on the host: `ragged_module_sampling_inputs` on CPU tensors in the kernel's arithmetic
type, moved to the GPU and handed to the discrete operator.  A one-ulp difference in the point picks another pixel, and
whether torch's GPU division by a Python scalar is the true division (the kernels' is) is not something these tests depend
on.  With the pixels equal, only the softmax's rounding separates the kernels from that composition, which the project's
fp32 bounds (tests/test_gpu_fused_ragged.assert_fp32_close) cover."""
import zlib

import numpy as np
import pytest
import torch

from msda_triton_amd import _lib, discrete, functional
from msda_triton_amd.functional import KernelTimer, fused_module_core, multiscale_deformable_attention
from msda_triton_amd.module import MultiscaleDeformableAttention
from msda_triton_amd.ragged import ragged_module_sampling_inputs
from test_discrete_sampling import options
from test_gpu_fused_ragged import COUNTS, SHAPES, assert_fp32_close, close16, make, names
from test_gpu_hf_box_discrete import boundary_coords, one_hot_problem
from test_gpu_parity import BWD_TOL, FWD_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FWD, BWD = "msda_fwd_fused_discrete", "msda_bwd_fused_discrete"
ALL_COUNTS = dict(COUNTS, p4=[4, 4, 4, 4], p3=[3, 3, 3, 3])


def host_points(proj, shapes, ref, counts):
    """the yardstick: the module's rule on CPU tensors, in the dtype of the reference points (the kernel's arithmetic type)"""
    ref = ref.detach().cpu()
    return ragged_module_sampling_inputs(proj.detach().cpu().to(ref.dtype), shapes.cpu(), ref, tuple(counts))


def composition(v, shapes, pr, rf, counts):
    """host-formed points, the softmax as a differentiable PyTorch op on the GPU, the discrete operator"""
    pts, _ = host_points(pr, shapes, rf, counts)
    att = pr[..., 2].to(rf.dtype).softmax(-1)
    return multiscale_deformable_attention(v, shapes, pts.to(DEV), att, "border", False, points_per_level=counts,
                                           sampling_mode="discrete")


def run(fused, value, shapes, proj, ref, gout, counts, need_img=True, level_shapes=None):
    v = value.detach().clone().requires_grad_(need_img)
    pr, rf = proj.detach().clone().requires_grad_(True), ref.detach().clone().requires_grad_(True)
    if fused:
        out = fused_module_core(v, shapes, pr, rf, "border", False, level_shapes, points_per_level=counts,
                                sampling_mode="discrete", fuse_discrete=True)
    else:
        out = composition(v, shapes, pr, rf, counts)
    out.backward(gout.to(out.dtype))
    return out.detach(), v.grad, pr.grad, rf.grad


def only_the_new_pair(kt, bwd=1):
    n = names(kt)
    others = [k for k in n if k.startswith(("msda_fwd", "msda_bwd")) and k not in (FWD, BWD)]
    return n.count(FWD) == 1 and n.count(BWD) == bwd and not others


def assert_matches(got, want, check=assert_fp32_close):
    """out, grad_value and the logit slots of grad_proj within `check`; the offset slots exact zeros; no reference-point gradient."""
    assert got[3] is None and (want[3] is None or not bool(want[3].any()))
    assert bool((got[2][..., :2] == 0).all()) and bool((want[2][..., :2] == 0).all())
    check((got[0], got[1], got[2][..., 2]), (want[0], want[1], want[2][..., 2]))


def fused(value, shapes, proj, ref, counts):
    return fused_module_core(value, shapes, proj, ref, "border", False, points_per_level=counts, sampling_mode="discrete",
                             fuse_discrete=True)


# ------------------------------------------------------------------------------------------ the pixel, exactly
def host_pixels(pts, levels, counts):
    """the integer formula on the host: pts [..., S, 2] -> the pyramid index of every sample's pixel"""
    out, s0, start = [], 0, 0
    for (h, w), P in zip(levels, counts):
        xy = pts[..., s0:s0 + P, :]
        ix = torch.clamp(torch.trunc(xy[..., 0] * w + 0.5), 0, w - 1)
        iy = torch.clamp(torch.trunc(xy[..., 1] * h + 0.5), 0, h - 1)
        out.append(start + torch.nan_to_num(iy).to(torch.int64) * w + torch.nan_to_num(ix).to(torch.int64))
        s0, start = s0 + P, start + h * w
    return torch.cat(out, -1)


def assert_same_pixels(value, shapes, proj, ref, levels, counts):
    with KernelTimer() as kt:
        got = fused(value, shapes, proj, ref, counts)
    assert names(kt) == [FWD], names(kt)
    pts, att = host_points(proj, shapes, ref, counts)
    assert bool(((att == 0) | (att == 1)).all())  # (exactly one-hot)
    want = multiscale_deformable_attention(value, shapes, pts.to(DEV), att.to(DEV), "border", False, points_per_level=counts,
                                           sampling_mode="discrete")
    wrong = (got != want).any(-1).nonzero()
    assert wrong.numel() == 0, (len(wrong), wrong[:4].tolist(), got[tuple(wrong[0])], want[tuple(wrong[0])])
    assert torch.equal(got, want)
    # ... and the integer formula on the host-formed points: query q's hot sample is q % S
    Q, S = proj.shape[1], proj.shape[3]
    pix = host_pixels(pts, levels, counts)  # [B, Q, H, S]
    hot = (torch.arange(Q) % S)[None, :, None, None].expand(pix.shape[0], Q, pix.shape[2], 1)
    assert torch.equal(got[..., 0].cpu().to(torch.int64), pix.gather(3, hot)[..., 0])
    return got


@pytest.mark.parametrize("cname", ["3_6_3", "p3"])
@pytest.mark.parametrize("ref_dim", [2, 4])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_pixel_choice_is_exact_on_random_inputs(dtype, ref_dim, cname):
    counts = ALL_COUNTS[cname][:3]
    B, Q, H, D, levels = SHAPES["d32"]
    levels = levels[:3]
    g = torch.Generator().manual_seed(71 + ref_dim)
    ref = torch.rand(B, 40 * Q, ref_dim, generator=g, dtype=dtype)
    xy = torch.randn(B, 40 * Q, H, sum(counts), 2, generator=g, dtype=dtype) * 1.5
    got = assert_same_pixels(*one_hot_problem(ref, xy, levels, counts, H, dtype), levels, counts)
    assert len(torch.unique(got)) > sum(h * w for h, w in levels) // 2  # (the samples do spread over the pyramid)


@pytest.mark.parametrize("ref_dim", [2, 4])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_pixel_choice_is_exact_on_every_rounding_boundary(dtype, ref_dim):
    """Zero offsets (2-d) / boxes with w = h = 0 under random offsets (4-d): the point is the reference point exactly.  Every
    boundary coordinate of every level's axes meets every sample slot (query c * S + s carries coordinate pair c and its hot
    sample is s), so each level rounds each of them."""
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
    if ref_dim == 2:
        ref, offsets = xy.reshape(1, Q, 2), torch.zeros(1, Q, H, S, 2, dtype=dtype)
    else:
        ref = torch.cat([xy, torch.zeros(Q, 2, dtype=dtype)], -1).reshape(1, Q, 4)
        offsets = torch.randn(1, Q, H, S, 2, generator=torch.Generator().manual_seed(5), dtype=dtype) * 1.5
    got = assert_same_pixels(*one_hot_problem(ref, offsets, levels, counts, H, dtype), levels, counts)
    # the point IS the reference point: the pixel of the boundary coordinate itself
    want = host_pixels(xy[:, None, :].expand(Q, S, 2), levels, counts).gather(1, (torch.arange(Q) % S)[:, None])[:, 0]
    assert torch.equal(got[0, :, 0, 0].cpu().to(torch.int64), want)


# ------------------------------------------------------------------------------------------ parked points and weights
@pytest.mark.parametrize("cname", ["3_6_3", "p3"])
@pytest.mark.parametrize("ref_dim", [2, 4])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_parked_points_are_the_host_rule_bit_for_bit_and_the_forward_is_reproducible(dtype, ref_dim, cname):
    counts = tuple(ALL_COUNTS[cname][:3])
    B, Q, H, D, levels = SHAPES["d32"]
    value, shapes, proj, ref, gout = make(B, 300, H, D, levels, counts, ref_dim, 41 + ref_dim, dtype)
    res = discrete.module_discrete_hip_bwd_fused(gout, value, shapes, proj, ref, counts, parked_points=True)
    again = discrete.module_discrete_hip_bwd_fused(gout, value, shapes, proj, ref, counts, parked_points=True)
    pts, att = host_points(proj, shapes, ref, counts)
    assert res[2].dtype == dtype and torch.equal(res[2].cpu(), pts)  # (true division, the level's own count, (h, w) order)
    # the parked weights are the kernel's softmax (exp(l - m) * (1 / sum)): torch's to rounding, and the same in every run
    torch.testing.assert_close(res[3].cpu(), att, atol=0.0, rtol=1e-5 if dtype == torch.float32 else 1e-13)
    assert torch.equal(res[3], again[3]) and torch.equal(res[2], again[2])
    assert torch.equal(res[0], again[0]) and torch.equal(res[1], again[1])
    a = discrete.module_discrete_hip_fwd_fused(value, shapes, proj, ref, counts)
    b = discrete.module_discrete_hip_fwd_fused(value, shapes, proj, ref, counts)
    assert torch.equal(a, b)
    # the forward's weights are the parked ones: the discrete operator on the parked buffers gives the forward's sum
    assert torch.equal(a, discrete.discrete_hip_fwd(value, shapes, res[2], res[3], counts))


# ------------------------------------------------------------------------------------------ fused against composition
@pytest.mark.parametrize("ref_dim", [2, 4])
@pytest.mark.parametrize("cname", list(ALL_COUNTS))
@pytest.mark.parametrize("name", list(SHAPES))
def test_fused_matches_composition(name, cname, ref_dim):
    """Q = 13 / 19 / 33 / 70 leave dead units in the last workgroup; D = 5 takes the scalar path."""
    counts = ALL_COUNTS[cname]
    B, Q, H, D, levels = SHAPES[name]
    c = make(B, Q, H, D, levels, counts, ref_dim, zlib.crc32(f"{name}{cname}".encode()) + ref_dim)
    with KernelTimer() as kt:
        got = run(True, *c, counts)
    assert only_the_new_pair(kt), names(kt)
    info = _lib.last_launch_info()
    assert info["fwd_variant"] == 4 and info["sample_variant"] == 3, info
    assert info["fwd_chunks"] == 1 and info["sample_chunks"] == 1, info  # (D <= 64: one trip over the channels)
    want = run(False, *c, counts)
    assert_matches(got, want)
    assert_matches(run(True, *c, counts), want)  # (no timer: the same Python Function)


def group_of(D):
    """G, the lanes per unit the launcher picks for this head dimension: read off a launch"""
    value, shapes, proj, ref, _ = make(1, 3, 1, D, [(2, 2)], [1], 2, 1)
    fused(value, shapes, proj, ref, [1])
    return _lib.last_launch_info()["fwd_group"]


EDGES = {
    # several channel chunks per sample (one D beyond the widest group's 256 channels), odd Q, scalar rows, a (1, 3) level
    # (D = 64 still fits one trip of the widest group — 16 lanes of 4 channels — so the chunked trips start beyond it)
    "d260_chunks": (1, 5, 1, 260, [(5, 4), (3, 2)], [3, 2]),
    "d65_scalar_chunks": (1, 5, 2, 65, [(5, 4), (3, 2)], [3, 2]),
    "level_1x3": (2, 19, 3, 8, SHAPES["d8"][4], [1, 2, 5, 1]),
    "l8": (2, 21, 3, 8, [(6, 5), (5, 4), (4, 4), (4, 3), (3, 3), (3, 2), (2, 2), (2, 1)], [1, 2, 1, 3, 1, 2, 1, 1]),
}


@pytest.mark.parametrize("ref_dim", [2, 4])
@pytest.mark.parametrize("name", list(EDGES))
def test_edge_shapes(name, ref_dim):
    B, Q, H, D, levels, counts = EDGES[name]
    c = make(B, Q, H, D, levels, counts, ref_dim, zlib.crc32(name.encode()) + ref_dim)
    with KernelTimer() as kt:
        got = run(True, *c, counts)
    assert only_the_new_pair(kt), names(kt)
    if name in ("d260_chunks", "d65_scalar_chunks"):
        assert _lib.last_launch_info()["fwd_chunks"] > 1 and _lib.last_launch_info()["sample_chunks"] > 1
    assert_matches(got, run(False, *c, counts))


@pytest.mark.parametrize("ref_dim", [2, 4])
def test_samples_per_unit_around_the_group_width_on_one_level(ref_dim):
    """L = 1 with S = 1, G, G + 1, 2 G + 1: a lone sample, a full trip, a trip with one live lane behind it, two and a bit."""
    D = 32
    G = group_of(D)
    assert G in (4, 8, 16, 32, 64)
    for S in (1, G, G + 1, 2 * G + 1):
        c = make(2, 19, 3, D, [(7, 9)], [S], ref_dim, 100 + S + ref_dim)
        with KernelTimer() as kt:
            got = run(True, *c, [S])
        assert only_the_new_pair(kt), (S, names(kt))
        assert _lib.last_launch_info()["fwd_group"] == G
        assert_matches(got, run(False, *c, [S]))


@pytest.mark.parametrize("value_path", [2, 3], ids=["sorted", "single_launch"])
def test_grad_value_routes_and_padded_rows(value_path):
    counts = [3, 6, 3]
    value, shapes, proj, ref, gout = make(2, 70, 8, 32, SHAPES["d32"][4], counts, 4, 17)
    want = run(False, value, shapes, proj, ref, gout, counts)
    with options(value_path=value_path):
        a = run(True, value, shapes, proj, ref, gout, counts)
        assert _lib.last_launch_info()["value_path"] == (2 if value_path == 2 else 1)
        b = run(True, value, shapes, proj, ref, gout, counts)
        B, I, H, D = value.shape
        padded = functional.padded_value_rows(B, I, H, D, value.dtype, value.device)
        padded.copy_(value)
        assert not padded.is_contiguous()
        c = run(True, padded, shapes, proj, ref, gout, counts)
    assert_matches(a, want)
    for x, y, z in zip(a[:3], b[:3], c[:3]):  # reproducible, and the padded rows change nothing
        assert torch.equal(x, y) and torch.equal(x, z)


def test_frozen_pyramid_needs_no_workspace_and_runs_one_kernel(monkeypatch):
    counts = (3, 6, 3)
    value, shapes, proj, ref, gout = make(2, 70, 8, 32, SHAPES["d32"][4], counts, 4, 19)
    args = (gout, value, shapes, proj, ref, counts)
    gv, gp = discrete.module_discrete_hip_bwd_fused(*args)
    lib = _lib.load()
    asked = []
    real = lib.msda_bwd_fused_discrete_workspace_bytes
    monkeypatch.setattr(lib, "msda_bwd_fused_discrete_workspace_bytes", lambda *a: asked.append(a) or real(*a))
    with options(profile=1):
        _lib.profile_read()
        with KernelTimer() as kt:
            gv0, gp0 = discrete.module_discrete_hip_bwd_fused(*args, need_img=False)
        kernels = _lib.profile_read()
    assert gv0 is None and not asked and names(kt) == [BWD]
    assert set(kernels) == {"msda_bwd_module_discrete_kernel"} and kernels["msda_bwd_module_discrete_kernel"][0] == 1, kernels
    assert torch.equal(gp0, gp)
    discrete.module_discrete_hip_bwd_fused(*args)
    assert len(asked) == 1 and real(*asked[0]) > 0
    d = run(True, value, shapes, proj, ref, gout, list(counts), need_img=False)
    assert d[1] is None and torch.equal(d[2], gp)
    assert torch.equal(run(True, value, shapes, proj, ref, gout, list(counts))[1], gv)


def test_nine_levels_take_the_composition():
    counts = [1, 2, 1, 3, 1, 2, 1, 1, 2]
    levels = [(6, 5), (5, 4), (4, 4), (4, 3), (3, 3), (3, 2), (2, 2), (2, 1), (1, 1)]
    c = make(2, 21, 3, 8, levels, counts, 4, 78)
    with KernelTimer() as kt:
        got = run(True, *c, counts)
    assert not any("fused_discrete" in n for n in names(kt)), names(kt)
    v = c[0].clone().requires_grad_(True)
    pr, rf = c[2].clone().requires_grad_(True), c[3].clone().requires_grad_(True)
    out = fused_module_core(v, c[1], pr, rf, "border", False, points_per_level=counts, sampling_mode="discrete", fuse_discrete=False)
    out.backward(c[4])
    for a, b in zip(got[:3], (out.detach(), v.grad, pr.grad)):
        assert torch.equal(a, b)
    assert got[3] is None
    assert discrete.module_discrete_hip_fwd_fused(c[0], c[1], c[2], c[3], tuple(counts)) is None
    assert discrete.module_discrete_hip_bwd_fused(c[4], c[0], c[1], c[2], c[3], tuple(counts)) is None


@pytest.mark.parametrize("ref_dim", [2, 4])
def test_fp64_against_autograd_through_the_host_composition(ref_dim):
    counts = [3, 6, 3]
    B, Q, H, D, levels = SHAPES["d8"]
    value, shapes, proj, ref, gout = make(B, Q, H, D, levels, counts, ref_dim, 5 + ref_dim, torch.float64)
    with KernelTimer() as kt:
        got = run(True, value, shapes, proj, ref, gout, counts)
    assert only_the_new_pair(kt), names(kt)
    v, pr, rf = [t.cpu().clone().requires_grad_(True) for t in (value, proj, ref)]
    pts, att = ragged_module_sampling_inputs(pr, shapes.cpu(), rf, counts)
    out = multiscale_deformable_attention(v, shapes.cpu(), pts, att, "border", False, points_per_level=counts,
                                          sampling_mode="discrete")
    out.backward(gout.cpu())
    assert got[3] is None and (rf.grad is None or not bool(rf.grad.any()))
    assert bool((got[2][..., :2] == 0).all()) and bool((pr.grad[..., :2] == 0).all())
    torch.testing.assert_close(got[0].cpu(), out.detach(), **FWD_TOL[torch.float64])
    torch.testing.assert_close(got[1].cpu(), v.grad, **BWD_TOL[torch.float64])
    torch.testing.assert_close(got[2].cpu(), pr.grad, **BWD_TOL[torch.float64])


@pytest.mark.parametrize("ref_dim", [2, 4])
@pytest.mark.parametrize("sdt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_storage_variants_match_fp32_on_the_rounded_inputs(sdt, ref_dim):
    """Against the fp32 kernels on the .float() of the same stored inputs: the same fp32 point, the same pixel."""
    counts = [3, 6, 3]
    levels = [(20, 16), (10, 8), (5, 4)]
    g = torch.Generator(device="cpu").manual_seed(35 + ref_dim)
    B, Q, H, D = 2, 90, 4, 32
    value = torch.randn(B, sum(h * w for h, w in levels), H, D, generator=g).to(sdt).to(DEV)
    proj = (torch.randn(B, Q, H, sum(counts), 3, generator=g) * 1.5).to(sdt).to(DEV)
    ref = torch.rand(B, Q, ref_dim, generator=g).to(DEV)
    gout = torch.randn(B, Q, H, D, generator=g).to(sdt).to(DEV)
    shapes = torch.tensor(levels, device=DEV)
    want = run(True, value.float(), shapes, proj.float(), ref, gout.float(), counts)
    # 16-bit value next to an fp32 projection (_vbf16 / _vf16): the fp32 kernels' numbers on the rounded rows
    with KernelTimer() as kt:
        got = run(True, value, shapes, proj.float(), ref, gout.float(), counts)
    assert only_the_new_pair(kt), names(kt)
    torch.testing.assert_close(got[0], want[0], atol=2e-5, rtol=1e-4)
    close16(got[1], want[1], sdt, "grad_value", scale_tol=3.0)
    torch.testing.assert_close(got[2], want[2], atol=1e-3, rtol=1e-3)
    # 16-bit value and projection next to fp32 reference points (_sbf16 / _sf16)
    assert functional.fused_storage_dtypes(value.dtype, proj.dtype, ref.dtype)
    with KernelTimer() as kt:
        out, gv, gp, gr = run(True, value, shapes, proj, ref, gout, counts)
    assert only_the_new_pair(kt), names(kt)
    assert gr is None and bool((gp[..., :2] == 0).all())
    close16(out, want[0], sdt, "out")
    close16(gp, want[2], sdt, "grad_proj")
    close16(gv, want[1], sdt, "grad_value", scale_tol=3.0)
    # one 16-bit dtype for every tensor (_bf16 / _f16): the same kernels' 16-bit instantiation, the point still in fp32
    with KernelTimer() as kt:
        out, gv, gp, gr = run(True, value, shapes, proj, ref.to(sdt), gout, counts)
    assert only_the_new_pair(kt), names(kt)
    want16 = run(True, value.float(), shapes, proj.float(), ref.to(sdt).float(), gout.float(), counts)
    close16(out, want16[0], sdt, "out")
    close16(gp, want16[2], sdt, "grad_proj")
    close16(gv, want16[1], sdt, "grad_value", scale_tol=3.0)


def test_buffer_contract():
    """Both launchers inside tests/guarded_alloc.py's banded, pre-filled allocations: the bands stay intact, every element
    of out, grad_value and grad_proj is written (the backward leaves g_s in grad_proj on the way: nothing of it may stay),
    the results are those of a plain call, and grad_proj's offset slots are exact zeros."""
    from guarded_alloc import contract_violations
    for ref_dim in (2, 4):
        counts = (1, 2, 5, 1)
        value, shapes, proj, ref, gout = make(2, 13, 3, 5, SHAPES["d5"][4], counts, ref_dim, 23)
        bad, _, _ = contract_violations(lambda: discrete.module_discrete_hip_fwd_fused(value, shapes, proj, ref, counts), 1, DEV)
        assert not bad, bad
        bad, _, res = contract_violations(lambda: discrete.module_discrete_hip_bwd_fused(gout, value, shapes, proj, ref, counts),
                                          3, DEV, names=["grad_value", "grad_proj"])
        assert not bad, bad
        for r in res:
            assert bool((r[1][..., :2] == 0).all())
        value, shapes, proj, ref, gout = make(2, 70, 8, 32, SHAPES["d32"][4], (3, 6, 3), ref_dim, 24)
        bad, _, res = contract_violations(
            lambda: discrete.module_discrete_hip_bwd_fused(gout, value.bfloat16(), shapes, proj.bfloat16(), ref, (3, 6, 3),
                                                           need_img=False), 1, DEV, names=["grad_proj"])
        assert not bad, bad  # (16-bit projection: g_s waits as two halves in the offset slots)
        for r in res:
            assert bool((r[0][..., :2] == 0).all())


# ------------------------------------------------------------------------------------------ the nn.Module
def test_fuse_discrete_none_takes_the_kernels_for_the_measured_dtypes_only():
    counts = [3, 6, 3]
    value, shapes, proj, ref, _ = make(2, 70, 8, 32, SHAPES["d32"][4], counts, 4, 29)
    for v, pr, want in ((value, proj, True), (value.bfloat16(), proj, True), (value.bfloat16(), proj.bfloat16(), True),
                        (value.half(), proj, False), (value.double(), proj.double(), False)):
        with KernelTimer() as kt:
            out = fused_module_core(v, shapes, pr, ref.to(pr.dtype) if pr.dtype == torch.float64 else ref, "border", False,
                                    points_per_level=counts, sampling_mode="discrete")
        assert (names(kt) == [FWD]) == want and (want or names(kt) == []), (v.dtype, pr.dtype, names(kt))
        assert out.dtype == pr.dtype


def module_run(m, fuse, img, shapes, q, ref, autocast, masks):
    m.fuse_discrete = fuse
    m.zero_grad(set_to_none=True)
    with KernelTimer() as kt, torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        out = m(img, shapes, q, ref, **masks)
        out.float().square().sum().backward()
    return out.detach().float(), {n: p.grad.detach().float().clone() for n, p in m.named_parameters()}, names(kt)


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masks"])
@pytest.mark.parametrize("value_dtype", [None, torch.bfloat16], ids=["fp32", "bf16_autocast"])
def test_module_on_the_gpu(value_dtype, masked):
    """The same module, the same projections (the rounded inputs of the core), with `fuse_discrete` True against False —
    the composition, masks included (`apply_value_mask` / `apply_query_mask` around the route in both legs).  fp32: the
    parity bounds (tests/test_gpu_parity.py); bf16 under autocast: tests/test_gpu_fused_ragged.test_module_under_autocast's
    bound on the result scaled to 1, for the result and every parameter gradient."""
    torch.manual_seed(4)
    autocast = value_dtype is not None
    m = MultiscaleDeformableAttention(32, 32, 3, 4, [3, 6, 3], "border", False, value_dtype=value_dtype,
                                      sampling_mode="discrete").to(DEV)
    levels = [(12, 10), (6, 5), (3, 3)]
    s = torch.tensor(levels, device=DEV)
    g = torch.Generator().manual_seed(9)
    I = sum(h * w for h, w in levels)  # noqa: E741
    img, q = torch.randn(2, I, 32, generator=g).to(DEV), torch.randn(2, 40, 32, generator=g).to(DEV)
    ref = torch.rand(2, 40, 4, generator=g).to(DEV)
    masks = {}
    if masked:
        vm, qm = torch.rand(2, I, generator=g) < 0.7, torch.rand(2, 40, generator=g) < 0.7
        masks = dict(value_mask=vm.to(DEV), query_mask=qm.to(DEV))
    out, grads, kn = module_run(m, True, img, s, q, ref, autocast, masks)
    assert kn.count(FWD) == 1 and kn.count(BWD) == 1, kn
    want, wgrads, kn0 = module_run(m, False, img, s, q, ref, autocast, masks)
    assert not any("fused_discrete" in n for n in kn0), kn0
    assert grads.keys() == wgrads.keys() and all(torch.isfinite(v).all() for v in grads.values())
    if autocast:
        for a, b in [(out, want)] + [(grads[n], wgrads[n]) for n in grads]:
            scale = b.abs().max().clamp_min(1e-30)
            torch.testing.assert_close(a / scale, b / scale, rtol=3e-2, atol=2e-2)
    else:
        torch.testing.assert_close(out, want, **FWD_TOL[torch.float32])
        for n in grads:
            torch.testing.assert_close(grads[n], wgrads[n], msg=lambda t: f"{n}: {t}", **BWD_TOL[torch.float32])
    if masked:  # a masked query's row is the output projection's bias in either leg
        rows = out[~masks["query_mask"]]
        torch.testing.assert_close(rows, m.query_output_proj.bias.detach().float().expand_as(rows), rtol=1e-2, atol=1e-2)
