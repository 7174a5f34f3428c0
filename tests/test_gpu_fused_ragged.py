"""GPU: the fused module kernels with per-level point counts (msda_fwd_fused_ragged_ / msda_bwd_fused_ragged_<suffix>)
against the prologue in PyTorch around the ragged operator, through `fused_module_core(..., points_per_level=)` and the
nn.Module with `num_points=[3, 6, 3]`."""
import zlib

import pytest
import torch

from msda_triton_amd import MultiscaleDeformableAttention, _ext, _lib, functional, ragged
from msda_triton_amd.functional import KernelTimer, fused_module_core, multiscale_deformable_attention
from msda_triton_amd.ragged import ragged_module_sampling_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (B, Q, H, D, levels): head dims of the vector (32, 8, 64) and scalar (5) kernels, non-square levels
SHAPES = {
    "d32": (2, 70, 8, 32, [(16, 12), (8, 9), (4, 4), (2, 3)]),
    "d5": (2, 13, 3, 5, [(6, 4), (3, 2), (2, 5), (3, 3)]),
    "d8": (2, 19, 3, 8, [(7, 9), (3, 4), (2, 2), (1, 3)]),
    "d64": (1, 33, 4, 64, [(9, 7), (5, 4), (3, 2), (2, 2)]),
}
COUNTS = {"3_6_3": [3, 6, 3], "1_2_5_1": [1, 2, 5, 1], "2_4_6_4": [2, 4, 6, 4]}


def names(kt):
    return [r[0] for r in kt.records]


def make(B, Q, H, D, levels, counts, ref_dim, seed, dtype=torch.float32):
    g = torch.Generator(device="cpu").manual_seed(seed)
    levels = levels[:len(counts)]
    value = torch.randn(B, sum(h * w for h, w in levels), H, D, generator=g, dtype=dtype)
    proj = torch.randn(B, Q, H, sum(counts), 3, generator=g, dtype=dtype) * 1.5
    ref = torch.rand(B, Q, ref_dim, generator=g, dtype=dtype)
    gout = torch.rand(B, Q, H, D, generator=g, dtype=dtype)
    return [t.to(DEV) for t in (value, torch.tensor(levels), proj, ref, gout)]


def run(fused, value, shapes, proj, ref, gout, pm, ac, counts, level_shapes=None, need_img=True):
    v = value.detach().clone().requires_grad_(need_img)
    pr, rf = proj.detach().clone().requires_grad_(True), ref.detach().clone().requires_grad_(True)
    if fused:
        out = fused_module_core(v, shapes, pr, rf, pm, ac, level_shapes, points_per_level=counts)
    else:
        pts, att = ragged_module_sampling_inputs(pr.to(rf.dtype), shapes, rf, counts)
        out = multiscale_deformable_attention(v, shapes, pts, att, pm, ac, level_shapes=level_shapes, points_per_level=counts)
    out.backward(gout.to(out.dtype))
    return out.detach(), v.grad, pr.grad, rf.grad


def assert_fp32_close(got, want):
    torch.testing.assert_close(got[0], want[0], atol=2e-5, rtol=1e-4)
    for a, b in zip(got[1:], want[1:]):
        torch.testing.assert_close(a, b, atol=1e-3, rtol=1e-3)


@pytest.mark.parametrize("ref_dim", [2, 4])
@pytest.mark.parametrize("cname", list(COUNTS))
@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("pm,ac", [("zeros", False), ("border", True)], ids=["zeros_0", "border_1"])
def test_fused_matches_unfused(ref_dim, cname, name, pm, ac):
    counts = COUNTS[cname]
    B, Q, H, D, levels = SHAPES[name]
    c = make(B, Q, H, D, levels, counts, ref_dim, zlib.crc32(f"{name}{cname}".encode()) + ref_dim)
    with KernelTimer() as kt:
        got = run(True, *c, pm, ac, counts)
    assert "msda_fwd_fused_ragged" in names(kt) and "msda_bwd_fused_ragged" in names(kt), names(kt)
    assert_fp32_close(run(True, *c, pm, ac, counts), run(False, *c, pm, ac, counts))
    assert_fp32_close(got, run(False, *c, pm, ac, counts))


@pytest.mark.parametrize("ref_dim", [2, 4])
def test_sorted_pipeline_and_decoder_sized_calls(ref_dim):
    """c2 @ 10k-like with [2, 4, 6, 4] (sorted grad_value pipeline, LDS-served levels) and a decoder-sized call with the
    level sizes given (single-launch grad_value kernel)."""
    counts = [2, 4, 6, 4]
    levels = [(64, 64), (32, 32), (16, 16), (8, 8)]
    c = make(4, 10000, 8, 32, levels, counts, ref_dim, 21 + ref_dim)
    got = run(True, *c, "zeros", False, counts)
    assert _lib.last_launch_info()["value_path"] == 2
    assert_fp32_close(got, run(False, *c, "zeros", False, counts))
    counts = [3, 6, 3]
    levels = [(80, 80), (40, 40), (20, 20)]
    c = make(8, 300, 8, 32, levels, counts, ref_dim, 23 + ref_dim)
    got = run(True, *c, "zeros", False, counts, level_shapes=levels)
    assert _lib.last_launch_info()["value_path"] == 1
    assert_fp32_close(got, run(False, *c, "zeros", False, counts, level_shapes=levels))


@pytest.mark.parametrize("pm,ac", [("zeros", False), ("zeros", True), ("border", False), ("border", True)])
@pytest.mark.parametrize("ref_dim", [2, 4])
def test_fp64_backward_against_autograd_through_the_prologue(pm, ac, ref_dim):
    counts = [3, 6, 3]
    c = make(2, 37, 4, 16, [(9, 7), (5, 6), (3, 2)], counts, ref_dim, 5 + ref_dim, torch.float64)
    with KernelTimer() as kt:
        got = run(True, *c, pm, ac, counts)
    assert names(kt).count("msda_fwd_fused_ragged") == 1 and names(kt).count("msda_bwd_fused_ragged") == 1, names(kt)
    want = run(False, *c, pm, ac, counts)
    for a, b in zip(got, want):
        torch.testing.assert_close(a, b, atol=1e-8, rtol=1e-8)


def test_equal_counts_are_bit_identical_to_the_uniform_call():
    value, shapes, proj, ref, gout = make(2, 50, 8, 32, SHAPES["d32"][4], [4, 4, 4, 4], 4, 9)
    a = run(True, value, shapes, proj, ref, gout, "zeros", False, [4, 4, 4, 4])
    v, pr, rf = value.clone().requires_grad_(True), proj.clone().requires_grad_(True), ref.clone().requires_grad_(True)
    out = fused_module_core(v, shapes, pr.reshape(2, 50, 8, 4, 4, 3), rf, "zeros", False)
    out.backward(gout)
    for x, y in zip(a, (out.detach(), v.grad, pr.grad, rf.grad)):
        assert torch.equal(x, y)


ULP = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


def close16(a, b32, sdt, what, scale_tol=2.0):
    """`a` (16-bit) against the fp32 result: within `scale_tol` 16-bit ulps of the value's scale (tests/test_gpu_fused_storage.py)."""
    assert a.dtype == sdt, (what, a.dtype)
    a, b = a.float(), b32.float()
    err = (a - b).abs()
    bound = ULP[sdt] * scale_tol * b.abs().clamp_min(b.abs().max() * 1e-3)
    assert bool((err <= bound + 1e-30).all()), (what, float((err / bound.clamp_min(1e-30)).max()))


@pytest.mark.parametrize("sdt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("ref_dim", [2, 4])
def test_storage_variants_match_fp32_on_the_rounded_inputs(sdt, ref_dim):
    counts = [3, 6, 3]
    levels = [(20, 16), (10, 8), (5, 4)]
    g = torch.Generator(device="cpu").manual_seed(31 + ref_dim)
    B, Q, H, D = 2, 90, 4, 32
    value = torch.randn(B, sum(h * w for h, w in levels), H, D, generator=g).to(sdt).to(DEV)
    proj = (torch.randn(B, Q, H, sum(counts), 3, generator=g) * 1.5).to(sdt).to(DEV)
    ref = torch.rand(B, Q, ref_dim, generator=g).to(DEV)
    gout = torch.randn(B, Q, H, D, generator=g).to(sdt).to(DEV)
    shapes = torch.tensor(levels, device=DEV)
    want = run(True, value.float(), shapes, proj.float(), ref, gout.float(), "zeros", False, counts)
    # 16-bit value next to an fp32 projection (_vbf16 / _vf16): the fp32 kernels' numbers on the rounded rows
    with KernelTimer() as kt:
        got = run(True, value, shapes, proj.float(), ref, gout.float(), "zeros", False, counts)
    assert "msda_fwd_fused_ragged" in names(kt)
    torch.testing.assert_close(got[0], want[0], atol=2e-5, rtol=1e-4)
    close16(got[1], want[1], sdt, "grad_value", scale_tol=3.0)
    torch.testing.assert_close(got[2], want[2], atol=1e-3, rtol=1e-3)
    torch.testing.assert_close(got[3], want[3], atol=1e-3, rtol=1e-3)
    # 16-bit value and projection next to fp32 reference points (_sbf16 / _sf16)
    assert functional.fused_storage_dtypes(value.dtype, proj.dtype, ref.dtype)
    with KernelTimer() as kt:
        out, gv, gp, gr = run(True, value, shapes, proj, ref, gout, "zeros", False, counts)
    assert "msda_fwd_fused_ragged" in names(kt) and "msda_bwd_fused_ragged" in names(kt)
    assert gr.dtype == torch.float32
    close16(out, want[0], sdt, "out")
    close16(gp, want[2], sdt, "grad_proj")
    close16(gv, want[1], sdt, "grad_value", scale_tol=3.0)
    torch.testing.assert_close(gr, want[3], rtol=2e-4, atol=2e-4 * float(want[3].abs().max()))


@pytest.mark.parametrize("value_dtype", [None, torch.bfloat16], ids=["plain", "value_bf16"])
def test_module_under_autocast(value_dtype):
    torch.manual_seed(4)
    m = MultiscaleDeformableAttention(32, 32, 3, 4, [3, 6, 3], "zeros", False, value_dtype=value_dtype).to(DEV)
    levels = [(12, 10), (6, 5), (3, 3)]
    s = torch.tensor(levels, device=DEV)
    img = torch.randn(2, sum(h * w for h, w in levels), 32, device=DEV)
    q, ref = torch.randn(2, 40, 32, device=DEV), torch.rand(2, 40, 4, device=DEV)
    want = m(img, s, q, ref)
    with KernelTimer() as kt, torch.autocast("cuda", dtype=torch.bfloat16):
        out = m(img, s, q, ref)
        out.float().square().sum().backward()
    assert "msda_fwd_fused_ragged" in names(kt) and "msda_bwd_fused_ragged" in names(kt), names(kt)
    assert m.query_input_proj.weight.grad is not None and m.img_input_proj.weight.grad is not None
    scale = want.abs().max()
    torch.testing.assert_close(out.float() / scale, want / scale, rtol=3e-2, atol=2e-2)


def test_module_on_gpu_equals_host_and_falls_back_beyond_the_one_pass_limit():
    torch.manual_seed(3)
    m = MultiscaleDeformableAttention(64, 64, 3, 4, [3, 6, 3], "zeros", False)
    shapes = [(7, 5), (4, 3), (2, 2)]
    I = sum(h * w for h, w in shapes)  # noqa: E741
    img, q, ref = torch.randn(2, I, 64), torch.randn(2, 50, 64), torch.rand(2, 50, 4)
    out_cpu = m(img, torch.tensor(shapes), q, ref)
    m = m.to(DEV)
    with KernelTimer() as kt:
        out_gpu = m(img.to(DEV), torch.tensor(shapes, device=DEV), q.to(DEV), ref.to(DEV))
    assert names(kt) == ["msda_fwd_fused_ragged"], names(kt)
    torch.testing.assert_close(out_gpu.cpu(), out_cpu, atol=1e-4, rtol=1e-3)
    # host-resident img_shapes next to GPU tensors
    torch.testing.assert_close(m(img.to(DEV), torch.tensor(shapes), q.to(DEV), ref.to(DEV)), out_gpu, atol=0, rtol=0)
    # S = 1281 samples per unit do not fit one LDS pass: the prologue runs in PyTorch around the ragged operator
    counts = [640, 641]
    c = make(1, 6, 2, 8, [(6, 6), (3, 3)], counts, 4, 77)
    assert not ragged.fused_ragged_limits_ok(8, 4, counts)
    with KernelTimer() as kt:
        got = run(True, *c, "border", False, counts)
    assert "msda_fwd_fused_ragged" in names(kt)  # (asked, declined: nothing was launched by that call)
    assert_fp32_close(got, run(False, *c, "border", False, counts))


def test_cpp_node_and_python_function_agree_bit_for_bit():
    ext = _ext.load()
    if ext is None or not hasattr(ext, "msda_fused_ragged"):
        pytest.skip("the C++ binding is not built")
    counts = [3, 6, 3]
    for ref_dim in (2, 4):
        value, shapes, proj, ref, gout = make(2, 70, 8, 32, SHAPES["d32"][4], counts, ref_dim, 13)
        a = run(True, value, shapes, proj, ref, gout, "zeros", False, counts)  # (no timer, no autocast: the C++ node)
        v, pr, rf = value.clone().requires_grad_(True), proj.clone().requires_grad_(True), ref.clone().requires_grad_(True)
        out = ragged._HipFusedRaggedModuleCoreFunction.apply(v, shapes, pr, rf, "zeros", False, tuple(counts), 0)
        out.backward(gout)
        for x, y in zip(a, (out.detach(), v.grad, pr.grad, rf.grad)):
            assert torch.equal(x, y)


def test_padded_rows_reproducibility_and_frozen_pyramid(monkeypatch):
    counts = [3, 6, 3]
    value, shapes, proj, ref, gout = make(2, 70, 8, 32, SHAPES["d32"][4], counts, 4, 17)
    a = run(True, value, shapes, proj, ref, gout, "zeros", False, counts)
    b = run(True, value, shapes, proj, ref, gout, "zeros", False, counts)
    assert torch.equal(a[1], b[1])  # grad_value of two identical calls
    B, I, H, D = value.shape
    padded = functional.padded_value_rows(B, I, H, D, value.dtype, value.device)
    padded.copy_(value)
    assert not padded.is_contiguous()
    c = run(True, padded, shapes, proj, ref, gout, "zeros", False, counts)
    for x, y in zip(a, c):
        assert torch.equal(x, y)
    # a frozen pyramid asks for no workspace
    asked = []
    lib = _lib.load()
    real = lib.msda_bwd_fused_ragged_workspace_bytes

    class Spy:
        def __getattr__(self, name):
            if name == "msda_bwd_fused_ragged_workspace_bytes":
                return lambda *args: asked.append(args) or real(*args)
            return getattr(lib, name)

    monkeypatch.setattr(_lib, "_lib", Spy())
    with KernelTimer():  # (the Python Function: it is the route that sizes the workspace through _lib)
        d = run(True, value, shapes, proj, ref, gout, "zeros", False, counts, need_img=False)
    assert not asked and d[1] is None
    assert torch.equal(d[2], a[2]) and torch.equal(d[3], a[3])
    with KernelTimer():
        run(True, value, shapes, proj, ref, gout, "zeros", False, counts)
    assert len(asked) == 1


def test_compiled_module_core_matches_eager():
    import msda_triton_amd.compile_op  # noqa: F401
    counts = [3, 6, 3]
    value, shapes, proj, ref, _ = make(2, 21, 4, 32, [(6, 5), (3, 4), (2, 2)], counts, 4, 19)

    def core(v, p, r):
        return fused_module_core(v, shapes, p, r, "zeros", False, points_per_level=counts)

    want = core(value, proj, ref)
    got = torch.compile(core, fullgraph=True, backend="aot_eager")(value, proj, ref)
    torch.testing.assert_close(got, want, atol=2e-5, rtol=1e-4)
