"""The deformable convolution core on the GPU: msda_dcn_{fwd,bwd}_<dtype> through the public functions against the float64
index-arithmetic reference on the CPU (dcn_cases.py) — every element of out and the three gradients.  Few test ids on
purpose: the cases of one topic run inside one test, and a failure names its case."""
import pytest
import torch

import dcn_cases as dc
from test_gpu_parity import BWD_TOL, FWD_TOL
from test_ragged_points import TOL as TOL16

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64


def tolerances(dtype):
    if dtype in FWD_TOL:
        return FWD_TOL[dtype], BWD_TOL[dtype]
    atol, rtol = TOL16[dtype]
    return dict(atol=atol, rtol=rtol), dict(atol=atol, rtol=rtol)


def gpu_run(c, inputs, dtype, **kw):
    from msda_triton_amd import deformable_conv_core
    return dc.run(deformable_conv_core, c, inputs, dtype, "cuda", **kw)


def launch_info():
    from msda_triton_amd.dcn import last_launch_info
    return last_launch_info()


def check(dtype=F64, seed=0, offset_std=1.5, **over):
    c, inputs, want = dc.case(dtype, seed, offset_std, **over)
    got = gpu_run(c, inputs, dtype)
    info = launch_info()
    assert (info["fwd_variant"], info["sample_variant"]) == (6, 5), info
    dc.assert_close(got, want, *tolerances(dtype), label=f"{dtype} {over}: ")
    return got, info


# the base case both ways; then the group's channels: D = 16 the 16-byte path, D = 36 the scalar one — in every type
@pytest.mark.parametrize("dtypes", [(F64, F32), (torch.bfloat16, torch.float16)], ids=["f64-f32", "bf16-f16"])
def test_base_case_storage_types_and_group_widths(dtypes):
    for dtype in dtypes:
        for softmax, D in [(False, 4), (True, 4), (True, 16), (False, 36)]:
            _, info = check(dtype, softmax=softmax, D=D)
            size = torch.empty((), dtype=dtype).element_size()
            assert info["fwd_vec"] == info["sample_vec"] == (16 // size if (D * size) % 16 == 0 else 1), (dtype, softmax, D)


# where a swapped tap order, a wrong centre or a wrong output size shows; and 484 pixels x 9 taps > 4096 samples per plane:
# grad_input through the sorted pipeline (every other case here takes the single-launch kernel)
SHAPES = [(F64, dict(kernel=(1, 3))), (F64, dict(kernel=(3, 1))), (F64, dict(kernel=(5, 5), pad=(2, 2))),
          (F64, dict(stride=(2, 2), pad=(0, 0))), (F64, dict(dil=(2, 2))), (F64, dict(scale=0.5)),
          (F32, dict(N=1, Hi=22, Wi=22, G=2, D=8))]


def test_geometry_and_the_sorted_pipeline():
    for dtype, over in SHAPES:
        for softmax in (False, True):
            _, info = check(dtype, seed=1, softmax=softmax, **over)
            assert info["value_path"] == (2 if over.get("Hi") == 22 else 1), (over, softmax)


def test_regular_grid_is_the_box_sum_exactly():
    """4 x 8 pixels (powers of two: the normalised round trip is exact), small integers, zero offsets, a mask of ones."""
    for dtype in (F32, F64):
        regular_grid(dtype)


def regular_grid(dtype):
    from msda_triton_amd import deformable_conv_core
    g = torch.Generator().manual_seed(2)
    x = torch.randint(-8, 9, (2, 4, 8, 3, 4), generator=g).to(dtype).cuda().requires_grad_()
    grad_out = torch.randint(-8, 9, (2, 4, 8, 3, 4), generator=g).to(dtype).cuda()
    off = torch.zeros(2, 4, 8, 3, 9, 2, dtype=dtype, device="cuda")
    out = deformable_conv_core(x, off, torch.ones(2, 4, 8, 3, 9, dtype=dtype, device="cuda"), 3)
    out.backward(grad_out)
    box = lambda t: torch.nn.functional.avg_pool2d(t.permute(0, 3, 4, 1, 2).reshape(2, 12, 4, 8), 3, 1, 1, divisor_override=1)  # noqa: E731
    back = lambda t: t.reshape(2, 3, 4, 4, 8).permute(0, 3, 4, 1, 2)  # noqa: E731
    assert launch_info()["fwd_variant"] == 6
    assert torch.equal(out.detach(), back(box(x.detach()))) and torch.equal(x.grad, back(box(grad_out)))


def test_window_on_and_off_are_the_same_bits():
    """17 x 17 output pixels: one more than two tiles each way, G = 5: a second, partial group block.  Offsets of std 2.5
    pixels against a halo of 1: a share of the corners leaves the staged window."""
    for dtype in (F32, torch.bfloat16):
        window_on_and_off(dtype)


def window_on_and_off(dtype):
    from msda_triton_amd import _lib
    c, inputs, want = dc.case(dtype, 3, 2.5, N=1, Hi=17, Wi=17, G=5, D=16, softmax=True)
    default = _lib.get_option("dcn_window")
    try:
        _lib.set_option("dcn_window", 1)
        on = gpu_run(c, inputs, dtype)
        assert launch_info()["dcn_window"] == 1 and launch_info()["sample_variant"] == 5
        _lib.set_option("dcn_window", 0)
        off = gpu_run(c, inputs, dtype)
        assert launch_info()["dcn_window"] == 0 and launch_info()["fwd_variant"] == 6
    finally:
        _lib.set_option("dcn_window", default)
    for name in dc.NAMES:
        assert torch.equal(on[name], off[name]), name
    dc.assert_close(on, want, *tolerances(dtype))


def test_packed_layout_frozen_input_and_rerun_are_bitwise():
    for softmax in (False, True):
        layouts_and_reruns(softmax)


def layouts_and_reruns(softmax):
    from msda_triton_amd import deformable_conv_core_packed
    from test_dcn import pack
    c, inputs, _ = dc.case(F32, softmax=softmax)
    split = gpu_run(c, inputs, F32)
    again = gpu_run(c, inputs, F32)
    frozen = gpu_run(c, inputs, F32, needs=(False, True, True))
    assert frozen["grad_input"] is None and launch_info()["sample_variant"] == 5
    for name in dc.NAMES:
        assert torch.equal(again[name], split[name]), name
        assert name == "grad_input" or torch.equal(frozen[name], split[name]), name
    om = pack(c, inputs["offset"], inputs["mask"]).float().cuda().requires_grad_()
    x = inputs["input"].float().cuda().requires_grad_()
    out = deformable_conv_core_packed(x, om, c["kernel"], c["stride"], c["pad"], c["dil"], c["scale"], softmax)
    out.backward(inputs["grad_out"].float().cuda())
    used = c["G"] * 27
    want = pack(c, split["grad_offset"], split["grad_mask"])[..., :used]
    assert torch.equal(out.detach().cpu().double(), split["out"]) and torch.equal(x.grad.cpu().double(), split["grad_input"])
    assert torch.equal(om.grad[..., :used].cpu().double(), want) and not om.grad[..., used:].any()


def test_module_matches_itself_on_the_cpu_in_float64():
    from msda_triton_amd import DeformableConv
    torch.manual_seed(5)
    ref = DeformableConv(24, 3, softmax=True).double()
    torch.nn.init.normal_(ref.offset_mask.weight, std=0.3)
    x = torch.randn(2, 6, 9, 24, dtype=F64)
    gpu = DeformableConv(24, 3, softmax=True).double().cuda()
    gpu.load_state_dict(ref.state_dict())
    xr, xg = x.clone().requires_grad_(), x.cuda().requires_grad_()
    ref(xr).square().sum().backward()
    gpu(xg).square().sum().backward()
    assert launch_info()["fwd_variant"] == 6 and launch_info()["sample_variant"] == 5
    torch.testing.assert_close(xg.grad.cpu(), xr.grad, **BWD_TOL[F64])
    for (name, a), b in zip(gpu.named_parameters(), ref.parameters()):
        torch.testing.assert_close(a.grad.cpu(), b.grad, **BWD_TOL[F64], msg=lambda m, n=name: f"{n}: {m}")
