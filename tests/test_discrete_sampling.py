"""Discrete (nearest-pixel) sampling, ``multiscale_deformable_attention(..., sampling_mode="discrete")``.

The yardstick is never the code under test: ``ref_discrete`` below is this file's own index formulation of the contract

    ix = clamp(trunc(x * w + 0.5), 0, w - 1)        iy = clamp(trunc(y * h + 0.5), 0, h - 1)
    out[b, q, head, :] += attention_weight * value[b, start_l + iy * w + ix, head, :]

(the index in the coordinates' own precision — fp32 for 16-bit ones —, the sums in fp64), and, where transformers
imports, its ``multi_scale_deformable_attention_v2(method="discrete")``.
"""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

from msda_triton_amd import multiscale_deformable_attention

F32, F64, BF16, F16 = torch.float32, torch.float64, torch.bfloat16, torch.float16

try:
    from transformers.models.d_fine.modeling_d_fine import multi_scale_deformable_attention_v2 as hf_core
except Exception:  # transformers absent or without D-FINE
    hf_core = None


# ----------------------------------------------------------------------------------------- the test-local formulation
def pixel_index(loc, shapes, counts):
    """[B, Q, H, S] int64: the plane-wide index of every sample's pixel; arithmetic in loc's dtype (fp32 / fp64), clamped
    in floating point before the conversion."""
    out, start, s0 = [], 0, 0
    for (h, w), P in zip(shapes, counts):
        x, y = loc[..., s0:s0 + P, 0], loc[..., s0:s0 + P, 1]
        ix = torch.clamp(torch.trunc(x * w + 0.5), 0, w - 1).to(torch.int64)
        iy = torch.clamp(torch.trunc(y * h + 0.5), 0, h - 1).to(torch.int64)
        out.append(start + iy * w + ix)
        start += h * w
        s0 += P
    return torch.cat(out, dim=-1)


def ref_discrete(value, shapes, loc, attn, counts):
    """fp64 output [B, Q, H, D]; differentiable in value and attn (fp64 leaves)."""
    B, I, H, D = value.shape
    Q, S = loc.shape[1], loc.shape[3]
    idt = loc.dtype if loc.dtype in (F32, F64) else F32
    pix = pixel_index(loc.detach().to(idt), shapes, counts)                       # [B, Q, H, S]
    idx = pix.permute(0, 2, 1, 3).reshape(B, H, Q * S, 1).expand(B, H, Q * S, D)
    rows = torch.gather(value.double().permute(0, 2, 1, 3), 2, idx).reshape(B, H, Q, S, D)
    return (rows * attn.double().permute(0, 2, 1, 3).unsqueeze(-1)).sum(3).permute(0, 2, 1, 3)


def make(shapes, counts, B=2, Q=17, H=2, D=8, dtype=F64, seed=0, lo=-0.3, hi=1.3):
    g = torch.Generator().manual_seed(seed)
    I = sum(h * w for h, w in shapes)  # noqa: E741
    S = sum(counts)
    value = torch.randn(B, I, H, D, generator=g, dtype=F64).to(dtype)
    loc = (torch.rand(B, Q, H, S, 2, generator=g, dtype=F64) * (hi - lo) + lo).to(dtype)
    attn = torch.rand(B, Q, H, S, generator=g, dtype=F64).to(dtype)
    return value, torch.tensor(shapes, dtype=torch.int64), loc, attn


def discrete(value, shp, loc, attn, counts=None, **kw):
    return multiscale_deformable_attention(value, shp, loc, attn, "border", False, points_per_level=counts,
                                           sampling_mode="discrete", **kw)


HOST_CASES = {
    "uniform": ([(6, 5), (3, 4)], [4, 4]),
    "d_fine_363": ([(8, 8), (4, 4), (2, 2)], [3, 6, 3]),
    "unequal_1425": ([(7, 9), (5, 3), (2, 2), (1, 1)], [1, 4, 2, 5]),
    "degenerate_levels": ([(1, 7), (6, 1), (1, 1)], [3, 2, 4]),
}


# ----------------------------------------------------------------------------------------- CPU: host path
@pytest.mark.parametrize("name", list(HOST_CASES))
@pytest.mark.parametrize("dtype,tol", [(F32, 1e-4), (F64, 1e-12)], ids=["f32", "f64"])
def test_host_matches_local_formulation_and_transformers(name, dtype, tol):
    shapes, counts = HOST_CASES[name]
    value, shp, loc, attn = make(shapes, counts, dtype=dtype)
    got = discrete(value, shp, loc, attn, counts)
    assert got.dtype == dtype and got.shape == (2, 17, 2, 8)
    torch.testing.assert_close(got.double(), ref_discrete(value, shapes, loc, attn, counts), atol=tol, rtol=tol)
    if hf_core is not None:
        hf = hf_core(value, shapes, loc, attn, counts, "discrete").reshape(got.shape)
        torch.testing.assert_close(got, hf, atol=tol, rtol=tol)


def test_host_uniform_six_d_layout_is_equal_counts_on_a_view():
    shapes, counts = HOST_CASES["uniform"]
    value, shp, loc, attn = make(shapes, counts)
    a = discrete(value, shp, loc, attn, counts)
    b = discrete(value, shp, loc.reshape(2, 17, 2, 2, 4, 2), attn.reshape(2, 17, 2, 2, 4))
    assert torch.equal(a, b)


def test_host_gradcheck_and_no_gradient_for_the_sampling_points():
    shapes, counts = [(4, 3), (2, 2), (1, 1)], [2, 3, 1]
    value, shp, loc, attn = make(shapes, counts, B=1, Q=3, H=2, D=3)
    value.requires_grad_(True)
    attn.requires_grad_(True)
    assert torch.autograd.gradcheck(lambda v, a: discrete(v, shp, loc, a, counts), (value, attn))
    loc.requires_grad_(True)
    discrete(value, shp, loc, attn, counts).sum().backward()
    assert loc.grad is None and value.grad is not None and attn.grad is not None


def test_host_gradients_match_local_formulation():
    shapes, counts = HOST_CASES["unequal_1425"]
    value, shp, loc, attn = make(shapes, counts)
    go = torch.randn(2, 17, 2, 8, dtype=F64, generator=torch.Generator().manual_seed(5))
    res = []
    for fn in (lambda v, a: discrete(v, shp, loc, a, counts), lambda v, a: ref_discrete(v, shapes, loc, a, counts)):
        v, a = value.clone().requires_grad_(True), attn.clone().requires_grad_(True)
        fn(v, a).backward(go)
        res.append((v.grad, a.grad))
    for x, y in zip(*res):
        torch.testing.assert_close(x, y, atol=1e-12, rtol=1e-12)


# ----------------------------------------------------------------------------------------- CPU: validation
def test_validation():
    shapes, counts = HOST_CASES["d_fine_363"]
    value, shp, loc, attn = make(shapes, counts)
    with pytest.raises(ValueError, match="sampling_mode"):
        multiscale_deformable_attention(value, shp, loc, attn, "border", False, points_per_level=counts,
                                        sampling_mode="nearest")
    with pytest.raises(ValueError, match="padding_mode"):
        multiscale_deformable_attention(value, shp, loc, attn, "zeros", False, points_per_level=counts,
                                        sampling_mode="discrete")
    with pytest.raises(ValueError, match="align_corners"):
        multiscale_deformable_attention(value, shp, loc, attn, "border", True, points_per_level=counts,
                                        sampling_mode="discrete")
    with pytest.raises(ValueError, match="entries"):
        discrete(value, shp, loc, attn, [6, 6])
    with pytest.raises(ValueError, match="sums to"):
        discrete(value, shp, loc, attn, [3, 6, 4])
    with pytest.raises(ValueError, match="at least 1"):
        discrete(value, shp, loc, attn, [3, 9, 0])
    with pytest.raises(ValueError, match="attention_weights"):
        discrete(value, shp, loc, attn[..., :-1], counts)
    with pytest.raises(ValueError):
        discrete(value, shp, loc, attn)  # 5-D points without counts


def test_bilinear_keyword_is_the_call_without_it():
    shapes, counts = HOST_CASES["d_fine_363"]
    value, shp, loc, attn = make(shapes, counts, dtype=F32)
    for pm, ac in (("zeros", False), ("border", True)):
        a = multiscale_deformable_attention(value, shp, loc, attn, pm, ac, points_per_level=counts)
        b = multiscale_deformable_attention(value, shp, loc, attn, pm, ac, points_per_level=counts, sampling_mode="bilinear")
        assert torch.equal(a, b)
        l6, a6 = loc[..., :12, :].reshape(2, 17, 2, 3, 4, 2), attn[..., :12].reshape(2, 17, 2, 3, 4)
        assert torch.equal(multiscale_deformable_attention(value, shp, l6, a6, pm, ac),
                           multiscale_deformable_attention(value, shp, l6, a6, pm, ac, None, None, "bilinear"))


# ----------------------------------------------------------------------------------------- CPU: library surface
GPU_SHAPES = {
    # name: (B, Q, H, D, levels, counts) — the D values of tests/test_gpu_parity.py's SHAPE_MATRIX: every lane grouping
    "d32_vec_g8_uniform": (2, 70, 8, 32, [(16, 16), (8, 8), (4, 4), (2, 2)], [4, 4, 4, 4]),
    "d64_vec_g16": (1, 33, 4, 64, [(9, 7), (5, 4)], [3, 6]),
    "d128_vec_g32": (1, 9, 2, 128, [(6, 6)], [2]),
    "d256_vec_g64": (1, 5, 1, 256, [(4, 5), (2, 3)], [2, 1]),
    "d512_two_channel_chunks": (1, 3, 1, 512, [(3, 3)], [2]),
    "d8_vec_g4_odd_s": (2, 19, 3, 8, [(7, 9), (3, 4)], [5, 2]),
    "d5_scalar_363": (2, 13, 3, 5, [(6, 4), (3, 2), (2, 5)], [3, 6, 3]),
    "d36_scalar_g64": (1, 7, 2, 36, [(5, 5), (2, 2)], [2, 2]),
    "d65_scalar_two_channel_chunks": (1, 5, 2, 65, [(4, 5), (2, 3)], [2, 3]),
    "d1": (1, 11, 2, 1, [(5, 6)], [3]),
    "pairs_not_multiple_of_8": (3, 21, 5, 16, [(8, 8), (4, 4)], [1, 4]),
    "s1": (1, 6, 2, 8, [(4, 4)], [1]),
    "s64": (1, 6, 2, 8, [(6, 6), (3, 3), (2, 2), (1, 1), (4, 2), (2, 4), (5, 1), (1, 5)], [8] * 8),
    "one_query": (1, 1, 1, 32, [(4, 4)], [1]),
    "level_1x1_1425": (2, 37, 2, 16, [(13, 9), (6, 7), (3, 2), (1, 1)], [1, 4, 2, 5]),
    "big_level_pixel_ranges": (1, 50, 1, 3, [(210, 200), (10, 10)], [2, 3]),
    "sorted_route": (2, 1200, 2, 32, [(32, 32), (16, 16), (8, 8), (4, 4)], [2, 4, 6, 4]),
}


def _lib_handle():
    from msda_triton_amd import _lib
    return _lib.load_discrete()


def _arr(counts):
    return (ctypes.c_int32 * len(counts))(*counts)


def test_library_exports_the_discrete_entry_points_within_abi_12():
    from msda_triton_amd import _lib
    lib = _lib_handle()
    assert lib.msda_abi_version() == 12
    for suf in _lib.DTYPE_SUFFIXES:
        assert hasattr(lib, f"msda_fwd_discrete_{suf}") and hasattr(lib, f"msda_bwd_discrete_{suf}")
    assert hasattr(lib, "msda_bwd_discrete_workspace_bytes") and hasattr(lib, "msda_bwd_discrete_supported")


def test_library_rejects_bad_arguments_without_launching():
    lib = _lib_handle()
    buf = ctypes.create_string_buffer(1 << 12)  # (host memory: a call that got past its checks would fault, not pass)
    p = ctypes.addressof(buf)
    BAD_ARG, TOO_MANY = -1, -2
    ok = _arr([3, 6, 3])
    dims = (1, 84, 2, 8, 5, 3)
    assert lib.msda_fwd_discrete_f32(None, p, p, p, p, *dims, ok, 0, None) == BAD_ARG          # value
    assert lib.msda_fwd_discrete_f32(p, p, p, p, None, *dims, ok, 0, None) == BAD_ARG          # out
    assert lib.msda_fwd_discrete_f32(p, p, p, p, p, *dims, None, 0, None) == BAD_ARG           # counts
    assert lib.msda_fwd_discrete_f32(p, p, p, p, p, *dims, _arr([3, 0, 3]), 0, None) == BAD_ARG
    assert lib.msda_fwd_discrete_f32(p, p, p, p, p, 1, 84, 2, 8, 5, 33, _arr([1] * 33), 0, None) == TOO_MANY
    assert lib.msda_fwd_discrete_f32(p, p, p, p, p, 1, 84, -2, 8, 5, 3, ok, 0, None) == BAD_ARG
    assert lib.msda_bwd_discrete_f32(None, p, p, p, p, p, p, *dims, ok, 0, 0, None, 0, None) == BAD_ARG
    assert lib.msda_bwd_discrete_f32(p, p, p, p, p, p, p, *dims, _arr([3, -1, 3]), 0, 0, None, 0, None) == BAD_ARG
    assert lib.msda_bwd_discrete_f32(p, p, p, p, p, p, p, 1, 84, 2, 8, 5, 33, _arr([1] * 33), 0, 0, None, 0, None) == TOO_MANY
    assert lib.msda_bwd_discrete_workspace_bytes(1, 84, 2, 8, 5, 3, _arr([3, 0, 3]), 4, 4, 0, 0) == 0
    assert lib.msda_bwd_discrete_supported(1, 84, 2, 8, 5, 3, _arr([3, 0, 3]), 4) == 0


UNSUPPORTED = [  # (B, I, H, D, Q, counts): no grad_value route — a plane of 2^22 pixels or more, too large for one workgroup
    (1, 1 << 22, 1, 8, 5000, [4]), (2, (1 << 22) + 5, 4, 32, 300, [3, 6, 3]), (1, 1 << 23, 1, 4, 10000, [2, 2]),
]


@pytest.mark.parametrize("name", list(GPU_SHAPES))
def test_workspace_query_and_supported_agree(name):
    """supported == 1: the query gives the size the call needs — 0 exactly where the call takes the single-launch kernel
    (Q * max P_l <= 4096 and the level fits its LDS; the GPU tests assert that route per shape), more than 0 on the sorted
    route, less for two passes than for one.  (That a call given exactly that size succeeds and one byte less is refused:
    test_gpu_workspace_query_is_sufficient_and_needed.)"""
    lib = _lib_handle()
    B, Q, H, D, levels, counts = GPU_SHAPES[name]
    I = sum(h * w for h, w in levels)  # noqa: E741
    sorted_route = name in ("sorted_route", "big_level_pixel_ranges")
    for es, ves in ((4, 4), (8, 8), (2, 2), (4, 2)):
        assert lib.msda_bwd_discrete_supported(B, I, H, D, Q, len(counts), _arr(counts), es) == 1
        ws = lib.msda_bwd_discrete_workspace_bytes(B, I, H, D, Q, len(counts), _arr(counts), es, ves, 0, 0)
        if not sorted_route:
            assert ws == 0, (name, es, ws)
            continue
        assert ws > 0 and ws % 256 == 0
        if B > 1:
            half = lib.msda_bwd_discrete_workspace_bytes(B, I, H, D, Q, len(counts), _arr(counts), es, ves, 0, 2 << 8)
            assert 0 < half < ws


@pytest.mark.parametrize("case", UNSUPPORTED, ids=[f"I{c[1]}" for c in UNSUPPORTED])
def test_workspace_query_is_zero_where_grad_value_is_unsupported(case):
    lib = _lib_handle()
    B, I, H, D, Q, counts = case  # noqa: E741
    for es, ves in ((4, 4), (8, 8), (2, 2), (4, 2)):
        assert lib.msda_bwd_discrete_supported(B, I, H, D, Q, len(counts), _arr(counts), es) == 0
        assert lib.msda_bwd_discrete_workspace_bytes(B, I, H, D, Q, len(counts), _arr(counts), es, ves, 0, 0) == 0


# ----------------------------------------------------------------------------------------- GPU
DEV = "cuda:0"


@contextlib.contextmanager
def options(**kw):
    from msda_triton_amd import _lib
    old = {k: _lib.get_option(k) for k in kw}
    try:
        for k, v in kw.items():
            _lib.set_option(k, v)
        yield
    finally:
        for k, v in old.items():
            _lib.set_option(k, v)


def run_gpu(value, shp, loc, attn, go, counts, needs=(True, True), pad=False, fn=None):
    v = value.to(DEV)
    if pad:
        from msda_triton_amd.functional import padded_value_rows
        vp = padded_value_rows(*v.shape, v.dtype, v.device, pad_bytes=128)
        vp.copy_(v)
        v = vp
    v.requires_grad_(needs[0])
    lo = loc.to(DEV).requires_grad_(True)
    at = attn.to(DEV).requires_grad_(needs[1])
    out = (fn or discrete)(v, shp.to(DEV), lo, at, counts)
    out.backward(go.to(DEV, out.dtype))
    assert lo.grad is None  # the sampling points: no gradient
    return out.detach().cpu(), (v.grad.cpu() if needs[0] else None), (at.grad.cpu() if needs[1] else None)


def check_gpu(name, img_dtype=F32, cdt=F32, out_tol=None, gv_tol=None, ga_tol=None, pad=False, seed=0):
    B, Q, H, D, levels, counts = GPU_SHAPES[name]
    value, shp, loc, attn = make(levels, counts, B=B, Q=Q, H=H, D=D, seed=seed)
    go = torch.rand(B, Q, H, D, dtype=F64, generator=torch.Generator().manual_seed(seed + 1))
    # inputs already rounded to their storage types: the comparison sees the kernels' arithmetic, not the rounding
    value, loc, attn, go = value.to(img_dtype), loc.to(cdt), attn.to(cdt), go.to(cdt)
    out, gv, ga = run_gpu(value, shp, loc, attn, go, counts, pad=pad)
    rv, ra = value.double().requires_grad_(True), attn.double().requires_grad_(True)
    ref = ref_discrete(rv, levels, loc, ra, counts)
    ref.backward(go.double())
    assert out.dtype == cdt and gv.dtype == img_dtype and ga.dtype == cdt
    for nm, got, want, tol in (("out", out, ref.detach(), out_tol), ("grad_value", gv, rv.grad, gv_tol),
                               ("grad_attn", ga, ra.grad, ga_tol)):
        err = float((got.double() - want).abs().max())
        print(f"{name} {img_dtype} {cdt} {nm}: max abs err {err:.3e}")
        torch.testing.assert_close(got.double(), want, msg=lambda m: f"{nm}: {m}", **tol)


TOL32 = dict(atol=1e-4, rtol=1e-4)  # fp32: the forward AND both gradients (no bilinear weights, no location gradient here)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GPU_SHAPES))
def test_gpu_f32_matches_local_formulation(name):
    check_gpu(name, out_tol=TOL32, gv_tol=TOL32, ga_tol=TOL32)
    from msda_triton_amd import _lib
    info = _lib.last_launch_info()
    assert info["fwd_variant"] == 3 and info["sample_variant"] == 2  # discrete kernels, no bilinear / host fallback
    # (the single-launch kernel wherever a level's cells and samples fit its LDS; else the sorted pipeline)
    assert info["value_path"] == (2 if name in ("sorted_route", "big_level_pixel_ranges") else 1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["d32_vec_g8_uniform", "d5_scalar_363", "d512_two_channel_chunks", "level_1x1_1425",
                                  "big_level_pixel_ranges", "sorted_route"])
def test_gpu_f64_matches_local_formulation(name):
    t = dict(atol=1e-8, rtol=1e-8)
    check_gpu(name, F64, F64, out_tol=t, gv_tol=t, ga_tol=t)


# 16-bit storage on pre-rounded inputs, at the tolerances of tests/test_gpu_parity.py (one 16-bit type for everything:
# fp16 2e-2 / 2e-2, bf16 4e-2 / 2e-2) and tests/test_gpu_mixed.py (16-bit value next to fp32: fp32 bounds for out and
# grad_attn, GV_TOL for the 16-bit grad_value)
STORAGE = {
    "f16": (F16, F16, dict(atol=2e-2, rtol=2e-2), dict(atol=2e-2, rtol=2e-2), dict(atol=2e-2, rtol=2e-2)),
    "bf16": (BF16, BF16, dict(atol=4e-2, rtol=2e-2), dict(atol=4e-2, rtol=2e-2), dict(atol=4e-2, rtol=2e-2)),
    "f32_vbf16": (BF16, F32, TOL32, dict(atol=2e-2, rtol=1e-2), TOL32),
    "f32_vf16": (F16, F32, TOL32, dict(atol=3e-3, rtol=2e-3), TOL32),
}


@pytest.mark.gpu
@pytest.mark.parametrize("storage", list(STORAGE))
@pytest.mark.parametrize("name", ["d32_vec_g8_uniform", "d5_scalar_363", "level_1x1_1425", "sorted_route",
                                  "d65_scalar_two_channel_chunks"])
def test_gpu_16_bit_storage(name, storage):
    img_dtype, cdt, ot, gvt, gat = STORAGE[storage]
    check_gpu(name, img_dtype, cdt, out_tol=ot, gv_tol=gvt, ga_tol=gat)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["d32_vec_g8_uniform", "d64_vec_g16", "sorted_route"])
def test_gpu_padded_value_rows(name):
    check_gpu(name, out_tol=TOL32, gv_tol=TOL32, ga_tol=TOL32, pad=True)


def boundary_coords(n):
    """fp32 coordinates on, and one ulp either side of, every (k + 0.5) / n boundary of an axis of n pixels; the ends;
    and far out of range."""
    k = np.arange(-1, n + 1, dtype=np.float64)
    c = ((k + 0.5) / n).astype(np.float32)
    up, dn = np.nextafter(c, np.float32(np.inf)), np.nextafter(c, np.float32(-np.inf))
    far = np.array([0.0, 1.0, -0.0, 1e30, -1e30, np.inf, -np.inf, 3.0e9, -3.0e9, 0.5], dtype=np.float32)
    return np.concatenate([c, up, dn, np.nextafter(up, np.float32(np.inf)), np.nextafter(dn, np.float32(-np.inf)), far])


def fma_sensitive_coords(n):
    """The fp32 coordinates x of an axis of n pixels at which a fused multiply-add picks ANOTHER pixel than the contract's
    rounded multiply followed by a rounded add: trunc(fl(fl(x * n) + 0.5)) != trunc(fl(x * n + 0.5)), the right-hand side
    being the exact product plus 0.5 rounded once (fp64 holds the fp32 product exactly).  Searched over the fp32
    neighbours of every (k + 0.5) / n.  They are rare by construction: fl(x * n) and fl(x * n + 0.5) round on the same
    grid unless k + 0.5 and k + 1 lie in different binades, which happens only at k = 0 (0.5 | 1), and there the window
    0.5 - 2^-25 < x * n < 0.5 - 2^-26 holds at most one fp32 x — for some axis sizes (19, 23, 38, 43, 134 ...), none for
    the others.  So an axis contributes one such coordinate or none."""
    out = []
    for k in range(n):
        x = np.float32((k + 0.5) / n)
        for _ in range(6):
            x = np.nextafter(x, np.float32(-np.inf))
        for _ in range(13):
            two = np.trunc(np.float32(np.float32(x * np.float32(n)) + np.float32(0.5)))
            one = np.trunc(np.float32(np.float64(x) * n + 0.5))
            if two != one:
                out.append(x)
            x = np.nextafter(x, np.float32(np.inf))
    return np.array(out, dtype=np.float32)


# axis sizes that HAVE an FMA-sensitive coordinate (asserted below), paired into level shapes
FMA_SHAPES = [(19, 23), (38, 43), (67, 71), (86, 87), (134, 135), (250, 251)]


def test_fma_sensitive_coordinates_exist_for_the_tested_axes():
    """The discriminating power of the exact-pixel tests, stated: each axis of FMA_SHAPES (and 134 of the 100 x 134 case)
    has a coordinate at which a contracted index picks the neighbouring pixel, and 40 or more axis sizes below 260 do."""
    for h, w in FMA_SHAPES:
        assert len(fma_sensitive_coords(h)) == 1 and len(fma_sensitive_coords(w)) == 1, (h, w)
    assert sum(len(fma_sensitive_coords(n)) for n in range(2, 260)) >= 40


@pytest.mark.gpu
def test_gpu_pixel_choice_at_every_fma_sensitive_coordinate():
    """Every axis size below 260 that has an FMA-sensitive coordinate, as an n x n level sampled at that coordinate (and
    its fp32 neighbours) in x and in y: the GPU picks the host formulation's pixel at each, where a contracted index would
    pick its neighbour."""
    checked = 0
    for n in range(2, 260):
        xs = fma_sensitive_coords(n)
        if len(xs) == 0:
            continue
        c = np.concatenate([xs, np.nextafter(xs, np.float32(1)), np.nextafter(xs, np.float32(0))])
        loc = torch.from_numpy(np.stack([c, c[::-1].copy()], -1)).reshape(1, len(c), 1, 1, 2)
        value = torch.arange(n * n, dtype=F32).reshape(1, n * n, 1, 1).expand(1, n * n, 1, 4).contiguous()
        want = pixel_index(loc, [(n, n)], [1]).reshape(-1)
        fused = torch.trunc((loc.double() * n + 0.5).float()).clamp(0, n - 1).to(torch.int64)  # what an FMA index picks
        assert (fused[..., 1] * n + fused[..., 0]).reshape(-1).ne(want).any(), n  # (the case discriminates)
        got = discrete(value.to(DEV), torch.tensor([[n, n]], device=DEV), loc.to(DEV), torch.ones(1, len(c), 1, 1, device=DEV),
                       [1]).cpu()
        assert torch.equal(got[0, :, 0, 0].to(torch.int64), want), (n, got[0, :, 0, 0], want)
        checked += 1
    print(f"{checked} axis sizes with an FMA-sensitive coordinate checked")
    assert checked >= 40


@pytest.mark.gpu
@pytest.mark.parametrize("hw", [(7, 13), (33, 50), (1, 1), (100, 134), (3, 1), (1, 6), (80, 80), (21, 37)] + FMA_SHAPES,
                         ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_gpu_pixel_choice_is_exact(hw):
    """The value rows hold their own pixel index and every unit has ONE sample of weight 1, so the output IS the chosen
    pixel: the GPU must pick exactly the pixel the host formulation picks — at, and one / two ulps either side of, every
    rounding boundary, at the axes' FMA-sensitive coordinates (fma_sensitive_coords: FMA_SHAPES and the 134 axis have one
    each) and far out of range; no case excluded."""
    h, w = hw
    fx, fy = fma_sensitive_coords(w), fma_sensitive_coords(h)
    if (h, w) in FMA_SHAPES:
        assert len(fx) == 1 and len(fy) == 1  # a coordinate per axis at which an FMA index picks another pixel
    xs, ys = np.concatenate([boundary_coords(w), fx]), np.concatenate([boundary_coords(h), fy])
    n = max(len(xs), len(ys))
    # every x against three different y (and the other way round)
    x = np.concatenate([np.resize(xs, n), np.resize(xs, n), np.resize(xs[::-1], n)])
    y = np.concatenate([np.resize(ys, n), np.resize(ys[::-1], n), np.resize(ys, n)])
    Q = len(x)
    loc = torch.from_numpy(np.stack([x, y], -1).astype(np.float32)).reshape(1, Q, 1, 1, 2)
    attn = torch.ones(1, Q, 1, 1)
    value = torch.arange(h * w, dtype=F32).reshape(1, h * w, 1, 1).expand(1, h * w, 1, 4).contiguous()
    shp = torch.tensor([[h, w]])
    want = pixel_index(loc, [(h, w)], [1]).reshape(-1)
    assert int(want.min()) >= 0 and int(want.max()) < h * w
    got = discrete(value.to(DEV), shp.to(DEV), loc.to(DEV), attn.to(DEV), [1]).cpu()
    wrong = (got[0, :, 0, 0].to(torch.int64) != want).nonzero().reshape(-1)
    print(f"{h}x{w}: {Q} samples, {len(wrong)} pixel choices differ")
    assert len(wrong) == 0, [(float(x[i]), float(y[i]), int(got[0, i, 0, 0]), int(want[i])) for i in wrong[:8].tolist()]
    assert torch.equal(got, ref_discrete(value, [(h, w)], loc, attn, [1]).float())
    if hf_core is not None:  # transformers converts with .to(int64) before it clamps: finite moderate coordinates only
        keep = torch.from_numpy((np.abs(x) < 4) & (np.abs(y) < 4))
        hf = hf_core(value, [(h, w)], loc[:, keep], attn[:, keep], [1], "discrete").reshape(1, -1, 1, 4)
        assert torch.equal(got[:, keep], hf)


@pytest.mark.gpu
def test_gpu_grad_value_bitwise_reproducible_both_routes_and_passes():
    from msda_triton_amd import _lib
    from msda_triton_amd.discrete import discrete_hip_bwd
    for name, path in (("sorted_route", 2), ("level_1x1_1425", 1)):
        B, Q, H, D, levels, counts = GPU_SHAPES[name]
        value, shp, loc, attn = make(levels, counts, B=B, Q=Q, H=H, D=D, dtype=F32)
        for hot in (False, True):
            if hot:  # every sample of a plane hits one pixel per level
                loc = torch.full_like(loc, 0.5)
            go = torch.randn(B, Q, H, D)
            args = [t.to(DEV) for t in (go, value, shp, loc, attn)]
            runs = []
            for passes in (1, 1, 2):
                gv, ga = discrete_hip_bwd(*args, tuple(counts), (True, True), ws_passes=passes)
                info = _lib.last_launch_info()
                assert info["value_path"] == path, (name, info)
                if path == 2:
                    assert info["value_passes"] == passes
                runs.append((gv.cpu(), ga.cpu()))
            for gv, ga in runs[1:]:
                assert torch.equal(gv, runs[0][0]) and torch.equal(ga, runs[0][1])
            rv, ra = value.double().requires_grad_(True), attn.double().requires_grad_(True)
            ref_discrete(rv, levels, loc, ra, counts).backward(go.double())
            print(f"{name} hot={hot} grad_value: max abs err {float((runs[0][0].double() - rv.grad).abs().max()):.3e}, "
                  f"largest |grad_value| {float(rv.grad.abs().max()):.3e}")
            torch.testing.assert_close(runs[0][0].double(), rv.grad, **TOL32)
            torch.testing.assert_close(runs[0][1].double(), ra.grad, **TOL32)


@pytest.mark.gpu
@pytest.mark.parametrize("value_path", [2, 3])
def test_gpu_forced_value_paths(value_path):
    with options(value_path=value_path):
        check_gpu("level_1x1_1425", out_tol=TOL32, gv_tol=TOL32, ga_tol=TOL32)
        from msda_triton_amd import _lib
        assert _lib.last_launch_info()["value_path"] == (2 if value_path == 2 else 1)


@pytest.mark.gpu
@pytest.mark.parametrize("needs", [(True, False), (False, True)], ids=["img_only", "weights_only"])
def test_gpu_needs_subsets(needs):
    B, Q, H, D, levels, counts = GPU_SHAPES["d5_scalar_363"]
    value, shp, loc, attn = make(levels, counts, B=B, Q=Q, H=H, D=D, dtype=F32)
    go = torch.randn(B, Q, H, D)
    _, gv, ga = run_gpu(value, shp, loc, attn, go, counts, needs=needs)
    _, gv2, ga2 = run_gpu(value, shp, loc, attn, go, counts)
    assert (gv is None) == (not needs[0]) and (ga is None) == (not needs[1])
    if needs[0]:
        assert torch.equal(gv, gv2)
    if needs[1]:
        assert torch.equal(ga, ga2)


@pytest.mark.gpu
def test_gpu_unsupported_grad_value_raises_at_forward_time():
    I = 1 << 22  # noqa: E741  (a plane of 2^22 pixels: beyond the cell pipelines' record format)
    value = torch.zeros(1, I, 1, 4, device=DEV)
    shp = torch.tensor([[2048, 2048]], device=DEV)
    loc, attn = torch.rand(1, 5000, 1, 2, 2, device=DEV), torch.rand(1, 5000, 1, 2, device=DEV)
    out = discrete(value, shp, loc, attn, [2])  # forward only: fine
    assert out.shape == (1, 5000, 1, 4)
    with pytest.raises(ValueError, match="grad_value is not available"):
        discrete(value.requires_grad_(True), shp, loc, attn, [2])


@pytest.mark.gpu
def test_gpu_cpp_node_function_and_torch_compile_route_agree_bitwise():
    from msda_triton_amd import _ext, _lib
    from msda_triton_amd.discrete import _HipDiscreteFunction
    assert _ext.load() is not None and hasattr(_ext.load(), "msda_discrete")
    B, Q, H, D, levels, counts = 2, 64, 4, 32, [(8, 8), (4, 4), (2, 2)], [3, 6, 3]
    value, shp, loc, attn = make(levels, counts, B=B, Q=Q, H=H, D=D, dtype=F32)

    def f(v, s, lo, at):
        return multiscale_deformable_attention(v, s, lo, at, "border", False, points_per_level=counts,
                                               sampling_mode="discrete")

    def python_function(v, s, lo, at):
        return _HipDiscreteFunction.apply(v, s, lo, at, tuple(counts), 0)

    res = []
    for route, fn in (("cpp", f), ("python", python_function), ("compile", torch.compile(f, fullgraph=True))):
        v, lo, at = (t.to(DEV).requires_grad_(True) for t in (value, loc, attn))
        out = fn(v, shp.to(DEV), lo, at)
        if route == "cpp":
            assert "_HipDiscreteFunction" not in type(out.grad_fn).__name__  # (the C++ node)
        out.square().sum().backward()
        assert lo.grad is None
        info = _lib.last_launch_info()
        assert info["fwd_variant"] == 3 and info["sample_variant"] == 2
        res.append((out.detach(), v.grad, at.grad))
    for other in res[1:]:
        for x, y in zip(res[0], other):
            assert torch.equal(x, y)


@pytest.mark.gpu
def test_gpu_autocast_serves_mixed_storage_in_place():
    B, Q, H, D, levels, counts = GPU_SHAPES["d32_vec_g8_uniform"]
    value, shp, loc, attn = make(levels, counts, B=B, Q=Q, H=H, D=D, dtype=F32)
    v16 = value.to(BF16).to(DEV).requires_grad_(True)
    with torch.autocast("cuda", dtype=BF16):
        out = discrete(v16, shp.to(DEV), loc.to(DEV), attn.to(DEV), counts)
    assert out.dtype == F32
    out.sum().backward()
    assert v16.grad.dtype == BF16
    torch.testing.assert_close(out.double().cpu(), ref_discrete(value.to(BF16), levels, loc, attn, counts), **TOL32)


@pytest.mark.gpu
def test_gpu_workspace_query_is_sufficient_and_needed():
    """The sorted route with one batch element (no smaller pass to fall back to) and a level beyond the single-launch
    kernel (no workspace-free route to fall back to): a backward given exactly
    msda_bwd_discrete_workspace_bytes succeeds and is right; half of it, or no workspace, is MSDA_ERR_BAD_ARG, names the
    discrete query, and launches nothing.  (Not "one byte less": the query returns the larger of the 16-byte-vector and
    the scalar layout, because which one a call takes depends on its pointers' alignment, so it is an upper bound.)"""
    from msda_triton_amd import _lib
    from msda_triton_amd.functional import _stream_ptr
    lib = _lib_handle()
    # (a level too large for the single-launch kernel's LDS, which would otherwise serve a call without workspace)
    B, Q, H, D, levels, counts = GPU_SHAPES["big_level_pixel_ranges"]
    assert B == 1
    value, shp, loc, attn = make(levels, counts, B=B, Q=Q, H=H, D=D, dtype=F32)
    go = torch.randn(B, Q, H, D)
    I = value.shape[1]  # noqa: E741
    ws_bytes = lib.msda_bwd_discrete_workspace_bytes(B, I, H, D, Q, len(counts), _arr(counts), 4, 4, 0, 0)
    assert ws_bytes > 0
    dv, ds, dl, da, dg = (t.to(DEV).contiguous() for t in (value, shp, loc, attn, go))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    assert ws.data_ptr() % 256 == 0
    gv, ga = torch.full_like(dv, 7.0), torch.empty_like(da)

    def call(nbytes, wptr):
        with torch.cuda.device(0):
            return lib.msda_bwd_discrete_f32(dg.data_ptr(), dv.data_ptr(), ds.data_ptr(), dl.data_ptr(), da.data_ptr(),
                                             gv.data_ptr(), None, B, I, H, D, Q, len(counts), _arr(counts), 0, 0, wptr, nbytes,
                                             _stream_ptr(torch.device(DEV)))

    for nbytes, wptr in ((ws_bytes // 2, ws.data_ptr()), (0, None)):
        assert call(nbytes, wptr) == -1  # MSDA_ERR_BAD_ARG
        assert b"msda_bwd_discrete_workspace_bytes" in lib.msda_last_error()
    torch.cuda.synchronize()
    assert bool((gv == 7.0).all())  # nothing was launched
    assert call(ws_bytes, ws.data_ptr()) == 0
    torch.cuda.synchronize()
    assert _lib.last_launch_info()["value_path"] == 2
    rv = value.double().requires_grad_(True)
    ref_discrete(rv, levels, loc, attn.double(), counts).backward(go.double())
    torch.testing.assert_close(gv.cpu().double(), rv.grad, **TOL32)
