"""Per-level sampling-point counts (``points_per_level``): the D-FINE / DEIMv2 layout, [B, Q, H, S, 2] with
S = sum(P_l), level-major.  Host path against transformers' formulation and against the zero-padded dense call; GPU
kernels against the CPU oracle on zero-padded inputs."""
import contextlib

import numpy as np
import pytest
import torch

from msda_triton_amd import multiscale_deformable_attention

MODES = [("zeros", False), ("zeros", True), ("border", False), ("border", True)]
SHAPES = [(6, 5), (3, 4), (2, 2)]


def make(counts, B=2, Q=7, H=2, D=8, shapes=SHAPES, dtype=torch.float64, seed=0):
    g = torch.Generator().manual_seed(seed)
    I = sum(h * w for h, w in shapes)  # noqa: E741
    S = sum(counts)
    img = torch.randn(B, I, H, D, generator=g, dtype=dtype)
    loc = torch.rand(B, Q, H, S, 2, generator=g, dtype=dtype) * 1.4 - 0.2
    attn = torch.rand(B, Q, H, S, generator=g, dtype=dtype)
    return img, torch.tensor(shapes, dtype=torch.int64), loc, attn


def pad_dense(loc, attn, counts, fill=0.5):
    """Zero-pad every level to max(P_l): padded points carry weight 0 (location `fill`)."""
    B, Q, H, S, _ = loc.shape
    L, Pm = len(counts), max(counts)
    ploc = torch.full((B, Q, H, L, Pm, 2), fill, dtype=loc.dtype, device=loc.device)
    patt = torch.zeros((B, Q, H, L, Pm), dtype=attn.dtype, device=attn.device)
    s0 = 0
    for lvl, p in enumerate(counts):
        ploc[:, :, :, lvl, :p] = loc[:, :, :, s0:s0 + p]
        patt[:, :, :, lvl, :p] = attn[:, :, :, s0:s0 + p]
        s0 += p
    return ploc, patt


def unpad(t, counts):
    """[..., L, Pm, (2)] -> [..., S, (2)]: drop the padded entries."""
    return torch.cat([t[:, :, :, lvl, :p] for lvl, p in enumerate(counts)], dim=3)


# ----------------------------------------------------------------------------------------- host
@pytest.mark.parametrize("pm,ac", MODES)
def test_host_matches_zero_padded_dense_call(pm, ac):
    counts = [3, 6, 1]
    img, shp, loc, attn = make(counts)
    got = multiscale_deformable_attention(img, shp, loc, attn, pm, ac, points_per_level=counts)
    ploc, patt = pad_dense(loc, attn, counts)
    ref = multiscale_deformable_attention(img, shp, ploc, patt, pm, ac)
    torch.testing.assert_close(got, ref, rtol=1e-12, atol=1e-12)


def test_host_matches_transformers_v2_formulation():
    transformers = pytest.importorskip("transformers")  # noqa: F841
    try:
        from transformers.models.d_fine.modeling_d_fine import multi_scale_deformable_attention_v2
    except ImportError:
        pytest.skip("this transformers has no D-FINE")
    counts = [3, 6, 3]
    img, shp, loc, attn = make(counts, H=2, D=8)
    got = multiscale_deformable_attention(img, shp, loc, attn, "zeros", False, points_per_level=counts)
    B, I, H, D = img.shape  # noqa: E741
    ref = multi_scale_deformable_attention_v2(img, [tuple(s) for s in shp.tolist()], loc, attn, counts, "default")
    torch.testing.assert_close(got.reshape(B, loc.shape[1], H * D), ref, rtol=1e-10, atol=1e-10)


def test_host_gradcheck():
    counts = [1, 3]
    img, shp, loc, attn = make(counts, B=1, Q=2, H=1, D=2, shapes=[(3, 3), (2, 2)])
    for t in (img, loc, attn):
        t.requires_grad_(True)
    assert torch.autograd.gradcheck(
        lambda a, b, c: multiscale_deformable_attention(a, shp, b, c, "zeros", False, points_per_level=counts),
        (img, loc, attn))


def test_equal_counts_are_the_uniform_call():
    counts = [4, 4, 4]
    img, shp, loc, attn = make(counts)
    got = multiscale_deformable_attention(img, shp, loc, attn, "border", True, points_per_level=counts)
    B, Q, H, S, _ = loc.shape
    ref = multiscale_deformable_attention(img, shp, loc.reshape(B, Q, H, 3, 4, 2), attn.reshape(B, Q, H, 3, 4), "border",
                                          True)
    assert torch.equal(got, ref)


@pytest.mark.parametrize("counts,attn_shape,match", [
    ([3, 6], None, "entries"),
    ([3, 6, 4], None, "sums to"),
    ([3, 0, 9], None, "at least 1"),
    ([3, 6, 3], (2, 7, 2, 11), "attention_weights"),
])
def test_value_errors(counts, attn_shape, match):
    img, shp, loc, attn = make([3, 6, 3])
    if attn_shape is not None:
        attn = torch.rand(attn_shape, dtype=attn.dtype)
    with pytest.raises(ValueError, match=match):
        multiscale_deformable_attention(img, shp, loc, attn, "zeros", False, points_per_level=counts)


def test_library_exports_the_ragged_entry_points():
    from msda_triton_amd import _lib
    lib = _lib.load()
    assert lib.msda_abi_version() == 12
    for sym in ("msda_fwd_ragged_f32", "msda_bwd_ragged_f32_vbf16", "msda_bwd_ragged_workspace_bytes",
                "msda_bwd_ragged_supported"):
        getattr(lib, sym)
    import ctypes
    bad = (ctypes.c_int32 * 3)(3, 0, 3)
    assert lib.msda_bwd_ragged_supported(1, 100, 8, 32, 30, 3, bad, 4) == 0
    good = (ctypes.c_int32 * 3)(3, 6, 3)
    assert lib.msda_bwd_ragged_supported(1, 336, 8, 32, 30, 3, good, 4) == 1


# ----------------------------------------------------------------------------------------- GPU
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


def oracle_ragged(img, shp, loc, attn, grad_out, counts, pm, ac):
    """CPU oracle on zero-padded inputs; gradients of the padded entries dropped."""
    from oracle import msda_oracle
    ploc, patt = pad_dense(loc.double().cpu(), attn.double().cpu(), counts)
    v = img.double().cpu().numpy()
    s = shp.cpu().numpy()
    out = msda_oracle.forward(v, s, ploc.numpy(), patt.numpy(), pm, ac)
    gv, gl, ga = msda_oracle.backward(grad_out.double().cpu().numpy(), v, s, ploc.numpy(), patt.numpy(), pm, ac)
    return (torch.from_numpy(np.asarray(out)), torch.from_numpy(np.asarray(gv)),
            unpad(torch.from_numpy(np.asarray(gl)), counts), unpad(torch.from_numpy(np.asarray(ga)), counts))


def run_gpu(img, shp, loc, attn, grad_out, counts, pm, ac, img_dtype, cdt, needs=(True, True, True)):
    dev = torch.device("cuda:0")
    v = img.to(dev, img_dtype).requires_grad_(needs[0])
    lo = loc.to(dev, cdt).requires_grad_(needs[1])
    at = attn.to(dev, cdt).requires_grad_(needs[2])
    out = multiscale_deformable_attention(v, shp.to(dev), lo, at, pm, ac, points_per_level=counts)
    out.backward(grad_out.to(dev, cdt))
    torch.cuda.synchronize()
    return out.detach(), v.grad, lo.grad, at.grad


TOL = {torch.float64: (1e-9, 1e-9), torch.float32: (2e-4, 2e-4), torch.float16: (3e-2, 3e-2),
       torch.bfloat16: (1.5e-1, 1.5e-1)}
STORAGE = [(torch.float32, torch.float32), (torch.float64, torch.float64), (torch.float16, torch.float16),
           (torch.bfloat16, torch.bfloat16), (torch.bfloat16, torch.float32), (torch.float16, torch.float32)]


def check_against_oracle(counts, pm, ac, img_dtype, cdt, B=2, Q=37, H=2, D=32, shapes=SHAPES, needs=(True, True, True),
                         seed=0):
    img, shp, loc, attn = make(counts, B=B, Q=Q, H=H, D=D, shapes=shapes, seed=seed)
    # round the inputs to the storage types so the oracle sees what the kernels see
    img, loc, attn = img.to(img_dtype).double(), loc.to(cdt).double(), attn.to(cdt).double()
    grad_out = torch.randn(B, Q, H, D, dtype=torch.float64).to(cdt).double()
    got = run_gpu(img, shp, loc, attn, grad_out, counts, pm, ac, img_dtype, cdt, needs)
    ref = oracle_ragged(img, shp, loc, attn, grad_out, counts, pm, ac)
    tol = TOL[img_dtype if img_dtype != cdt else cdt]
    for name, g, r, want in zip(("out", "grad_value", "grad_loc", "grad_attn"), got, ref, (True,) + tuple(needs)):
        if not want:
            assert g is None, name
            continue
        torch.testing.assert_close(g.double().cpu(), r, rtol=tol[0], atol=tol[1], msg=lambda m: f"{name}: {m}")
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("img_dtype,cdt", STORAGE)
@pytest.mark.parametrize("pm,ac", MODES)
def test_gpu_matches_oracle_every_storage_and_mode(img_dtype, cdt, pm, ac):
    check_against_oracle([3, 6, 3], pm, ac, img_dtype, cdt)


@pytest.mark.gpu
@pytest.mark.parametrize("opt", [dict(lds_levels=2), dict(lds_levels=2, lds_planes=2), dict(unit_fwd=2),
                                 dict(unit_fwd=2, unit_waves=2), dict(value_path=2), dict(value_path=3),
                                 dict(value_path=2, place_path=1)])
def test_gpu_forced_variants(opt):
    with options(**opt):
        check_against_oracle([2, 4, 6], "zeros", False, torch.float32, torch.float32, Q=300, H=4)
        check_against_oracle([5, 1, 2], "border", True, torch.float32, torch.float32, Q=300, H=4, seed=1)
        # level starts 0, 2, 8: the last one starts an exchange batch of the sample-gradient kernel (G = 8 lanes per unit
        # at D = 32 fp32), so the LDS-served levels do run in the ragged sample-gradient kernel
        check_against_oracle([2, 6, 4], "zeros", True, torch.float32, torch.float32, Q=300, H=4, seed=2)


@pytest.mark.gpu
@pytest.mark.parametrize("value_path", [0, 2, 3])
def test_gpu_level_with_more_points_than_a_workgroup_has_threads(value_path):
    with options(value_path=value_path):
        check_against_oracle([3, 1100], "zeros", False, torch.float32, torch.float32, B=1, Q=3, H=1,
                             shapes=[(6, 5), (3, 4)])


@pytest.mark.gpu
@pytest.mark.parametrize("needs", [(True, False, False), (False, True, True), (False, True, False), (True, True, False)])
def test_gpu_needs_subsets(needs):
    check_against_oracle([3, 6, 3], "zeros", False, torch.float32, torch.float32, needs=needs)


@pytest.mark.gpu
def test_gpu_padded_value_rows():
    from msda_triton_amd.functional import padded_value_rows
    counts = [3, 6, 3]
    img, shp, loc, attn = make(counts, Q=50, D=32)
    dev = torch.device("cuda:0")
    B, I, H, D = img.shape  # noqa: E741
    padded = padded_value_rows(B, I, H, D, torch.float32, dev)
    padded.copy_(img.float())
    dense = img.float().to(dev)
    a = multiscale_deformable_attention(padded, shp.to(dev), loc.float().to(dev), attn.float().to(dev), "zeros", False,
                                        points_per_level=counts)
    b = multiscale_deformable_attention(dense, shp.to(dev), loc.float().to(dev), attn.float().to(dev), "zeros", False,
                                        points_per_level=counts)
    assert torch.equal(a, b)
    # ... and the backward reads the padded rows too
    grads = []
    for v in (padded, dense):
        v = v.detach().requires_grad_(True)
        lo, at = loc.float().to(dev).requires_grad_(True), attn.float().to(dev).requires_grad_(True)
        out = multiscale_deformable_attention(v, shp.to(dev), lo, at, "zeros", False, points_per_level=counts)
        out.backward(torch.ones_like(out))
        grads.append((v.grad, lo.grad, at.grad))
    for x, y in zip(*grads):
        assert torch.equal(x, y)


def test_records_stay_out_of_misaligned_gradient_buffers():
    """MSDA_WS_RECORDS_IN_GRADS with two passes: an odd S (3 + 4 = 7, H = 1, Q = 333: 9 324 bytes of grad_attn per batch
    element) leaves group offsets that are not 16-byte aligned, so the workspace is sized for records in the workspace —
    whatever the pass count; an aligned shape keeps the smaller size."""
    import ctypes
    from msda_triton_amd import _lib
    lib = _lib.load()

    def ws(counts, Q, flags):
        arr = (ctypes.c_int32 * len(counts))(*counts)
        return lib.msda_bwd_ragged_workspace_bytes(8, 42, 1, 32, Q, 2, arr, 4, 4, 0, flags)

    with options(value_path=2):
        for n in (2, 3, 4):
            assert ws([3, 4], 333, _lib.WS_RECORDS_IN_GRADS | _lib.ws_passes(n)) == ws([3, 4], 333, _lib.ws_passes(n)), n
            assert ws([3, 5], 334, _lib.WS_RECORDS_IN_GRADS | _lib.ws_passes(n)) < ws([3, 5], 334, _lib.ws_passes(n)), n
        # one pass: the records of the whole batch start at the buffers' own (aligned) beginning
        assert ws([3, 4], 333, _lib.WS_RECORDS_IN_GRADS) < ws([3, 4], 333, 0)


@pytest.mark.gpu
def test_gpu_odd_samples_several_passes():
    """S = 7, H = 1: a group's share of grad_loc / grad_attn is not 16-byte aligned under MSDA_WS_PASSES(2), so the
    records stay in the workspace; the result is still right."""
    with options(ws_passes=2, value_path=2):
        check_against_oracle([3, 4], "zeros", False, torch.float32, torch.float32, B=3, Q=333, H=1,
                             shapes=[(6, 5), (3, 4)])


@pytest.mark.gpu
@pytest.mark.parametrize("value_path", [2, 3])
def test_gpu_grad_value_is_bitwise_reproducible(value_path):
    counts = [3, 6, 3]
    img, shp, loc, attn = make(counts, Q=400, H=4)
    grad_out = torch.randn(2, 400, 4, 8, dtype=torch.float64)
    with options(value_path=value_path):
        a = run_gpu(img, shp, loc, attn, grad_out, counts, "zeros", False, torch.float32, torch.float32)
        b = run_gpu(img, shp, loc, attn, grad_out, counts, "zeros", False, torch.float32, torch.float32)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.gpu
def test_gpu_ragged_is_the_padded_call_up_to_rounding():
    counts = [3, 6, 3]
    img, shp, loc, attn = make(counts, B=2, Q=300, H=8, D=32, dtype=torch.float32)
    dev = torch.device("cuda:0")
    ploc, patt = pad_dense(loc, attn, counts)
    a = multiscale_deformable_attention(img.to(dev), shp.to(dev), loc.to(dev), attn.to(dev), "zeros", False,
                                        points_per_level=counts)
    b = multiscale_deformable_attention(img.to(dev), shp.to(dev), ploc.to(dev), patt.to(dev), "zeros", False)
    torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-5)


@pytest.mark.gpu
def test_gpu_cpp_route_and_python_route_agree():
    from msda_triton_amd import _ext
    from msda_triton_amd.ragged import _HipRaggedFunction
    assert _ext.load() is not None and hasattr(_ext.load(), "msda_ragged")
    counts = [3, 6, 3]
    img, shp, loc, attn = make(counts, Q=100, H=4, D=32, dtype=torch.float32)
    dev = torch.device("cuda:0")
    grad = torch.randn(2, 100, 4, 32, device=dev)
    res = []
    for route in ("cpp", "python"):
        v, lo, at = (t.to(dev).requires_grad_(True) for t in (img, loc, attn))
        if route == "cpp":
            out = multiscale_deformable_attention(v, shp.to(dev), lo, at, "zeros", False, points_per_level=counts)
            assert "_HipRaggedFunction" not in type(out.grad_fn).__name__  # (the C++ node)
        else:
            out = _HipRaggedFunction.apply(v, shp.to(dev), lo, at, "zeros", False, tuple(counts), 0)
        out.backward(grad)
        res.append((out.detach(), v.grad, lo.grad, at.grad))
    for x, y in zip(*res):
        assert torch.equal(x, y)


@pytest.mark.gpu
def test_gpu_torch_compile_fullgraph():
    counts = [3, 6, 3]
    img, shp, loc, attn = make(counts, Q=64, H=4, D=32, dtype=torch.float32)
    dev = torch.device("cuda:0")

    def f(v, s, lo, at):
        return multiscale_deformable_attention(v, s, lo, at, "border", True, points_per_level=counts)

    compiled = torch.compile(f, fullgraph=True)
    res = []
    for fn in (f, compiled):
        v, lo, at = (t.to(dev).requires_grad_(True) for t in (img, loc, attn))
        out = fn(v, shp.to(dev), lo, at)
        out.square().sum().backward()
        res.append((out.detach(), v.grad, lo.grad, at.grad))
    for x, y in zip(*res):
        torch.testing.assert_close(x, y, rtol=1e-6, atol=1e-6)

