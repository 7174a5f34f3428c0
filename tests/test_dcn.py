"""The deformable convolution core without a GPU: the package's PyTorch formulation against the index-arithmetic reference
(dcn_cases.py), the packed layout against the split one, and the argument errors."""
import pytest
import torch

import dcn_cases as dc
from msda_triton_amd import DeformableConv, deformable_conv_core, deformable_conv_core_packed
from msda_triton_amd.dcn import output_size, packed_channels

TOL = dict(atol=1e-9, rtol=1e-9)
GEOMETRIES = [dict(), dict(softmax=True), dict(kernel=(1, 3)), dict(kernel=(3, 1)), dict(kernel=(5, 5), pad=(2, 2)),
              dict(stride=(2, 2), pad=(0, 0)), dict(dil=(2, 2)), dict(scale=0.5), dict(stride=(2, 1), pad=(0, 2), dil=(1, 2))]


@pytest.mark.parametrize("over", GEOMETRIES, ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()) or "base")
def test_native_formulation_matches_the_reference(over):
    c, inputs, want = dc.case(**over)
    assert output_size(c["Hi"], c["Wi"], c["kernel"], c["stride"], c["pad"], c["dil"]) == tuple(want["out"].shape[1:3])
    dc.assert_close(dc.run(deformable_conv_core, c, inputs), want, TOL, TOL)


def pack(c, offset, mask):
    """DCNv4's layout from the split tensors; the padded tail holds ones, which nothing may read."""
    N, Ho, Wo, G, K = mask.shape
    per = torch.cat([offset.reshape(N, Ho, Wo, G, 2 * K), mask], -1).reshape(N, Ho, Wo, G * 3 * K)
    return torch.cat([per, per.new_ones((N, Ho, Wo, packed_channels(G, K) - G * 3 * K))], -1)


@pytest.mark.parametrize("softmax", [False, True])
def test_packed_layout_is_the_split_one(softmax):
    c, inputs, want = dc.case(softmax=softmax)
    om = pack(c, inputs["offset"], inputs["mask"]).requires_grad_()
    x = inputs["input"].clone().requires_grad_()
    out = deformable_conv_core_packed(x, om, c["kernel"], c["stride"], c["pad"], c["dil"], c["scale"], softmax)
    out.backward(inputs["grad_out"])
    N, Ho, Wo, G, K = inputs["mask"].shape
    assert om.shape[-1] == 88 and not om.grad[..., G * 3 * K:].any()
    torch.testing.assert_close(out.detach(), want["out"], **TOL)
    torch.testing.assert_close(x.grad, want["grad_input"], **TOL)
    torch.testing.assert_close(om.grad[..., :G * 3 * K], pack(c, want["grad_offset"], want["grad_mask"])[..., :G * 3 * K], **TOL)


def test_argument_errors():
    c, inputs, _ = dc.case()
    x, off, msk = inputs["input"], inputs["offset"], inputs["mask"]
    with pytest.raises(ValueError, match="kernel_size"):
        deformable_conv_core(x, off, msk, (3, 0))
    with pytest.raises(ValueError, match="stride"):
        deformable_conv_core(x, off, msk, 3, stride=0)
    with pytest.raises(ValueError, match="offset_scale"):
        deformable_conv_core(x, off, msk, 3, offset_scale=float("nan"))
    with pytest.raises(ValueError, match="`offset` should be"):
        deformable_conv_core(x, off, msk, 3, padding=0)  # (the output is 3 x 5 then)
    with pytest.raises(ValueError, match="`mask` should be"):
        deformable_conv_core(x, off, msk[..., :8], 3)
    with pytest.raises(ValueError, match="`input` should be"):
        deformable_conv_core(x[0], off, msk, 3)
    with pytest.raises(ValueError, match="`offset_mask` should be"):
        deformable_conv_core_packed(x, torch.zeros(2, 5, 7, 81, dtype=torch.float64), 3)
    with pytest.raises(ValueError, match="divisible"):
        DeformableConv(10, 3)


def test_module_starts_on_the_regular_grid():
    """Zero-initialised offset_mask: DCNv4 starts at zero, DCNv3 at the box mean of the projected values."""
    torch.manual_seed(0)
    x = torch.randn(1, 4, 6, 8, dtype=torch.float64)
    m = DeformableConv(8, 2, softmax=True).double()
    v = m.value_proj(x).permute(0, 3, 1, 2)
    box = torch.nn.functional.avg_pool2d(v, 3, 1, 1, count_include_pad=True).permute(0, 2, 3, 1)
    torch.testing.assert_close(m(x), m.output_proj(box), **TOL)
    assert not DeformableConv(8, 2).double()(x).detach().sub(m.output_proj.bias.detach()).any()
