"""The deformable convolution core of DCNv3 / DCNv4 (InternImage, FlashInternImage): deformable attention on the pixel lattice.

    lx = wo sw - pw + cx + s (i dw - cx + ox_k)      ly = ho sh - ph + cy + s (j dh - cy + oy_k)       k = i kh + j
    m = softmax_k(mask) | mask        out[n, ho, wo, g, :] = sum_k m_k bilinear(input[n, :, :, g, :], lx, ly)

with ``cx = (dw (kw - 1)) // 2``, ``cy = (dh (kh - 1)) // 2``, tap ``i`` the window's column (the OUTER index, DCNv3's loop
order) and zeros outside the image.  ``input`` is channels-last ``[N, Hi, Wi, G, D]``.

  deformable_conv_core          offsets ``[N, Ho, Wo, G, K, 2]`` (x, y) and mask ``[N, Ho, Wo, G, K]`` as two tensors (DCNv3)
  deformable_conv_core_packed   DCNv4's ``offset_mask [N, Ho, Wo, C]``: per group 2K offsets then K mask values, read in place
  native_deformable_conv_core   the operator in plain PyTorch: host tensors, traced calls, unsupported dtypes
  dcn_hip_fwd / dcn_hip_bwd     the launcher pair over ``msda_dcn_{fwd,bwd}_<dtype>`` (include/msda_hip.h)
  DeformableConv                a thin module: value projection, one offset_mask layer, output projection

GPU tensors of one dtype among float32, float64, bfloat16, float16 run the gfx950 kernels: no sampling-point
tensor is built, the softmax and its chain rule run in the kernels, and grad_input comes from the scatter-free grad_value
pipeline.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple, Union

import torch
from torch import nn
from torch.amp import custom_bwd, custom_fwd
from torch.autograd.function import Function, once_differentiable

from . import _lib
from ._linear import projection
from .functional import _SUFFIX, _check_devices, _fused_run

IntPair = Union[int, Sequence[int]]


def _hw(v: IntPair, name: str, lowest: int) -> Tuple[int, int]:
    h, w = (v, v) if isinstance(v, int) else tuple(v)
    if not all(isinstance(a, int) and a >= lowest for a in (h, w)):
        raise ValueError(f"`{name}` should be an int or an (h, w) pair of ints >= {lowest}, but got {v!r}.")
    return h, w


def output_size(Hi: int, Wi: int, kernel_size: IntPair, stride: IntPair = 1, padding: IntPair = 1, dilation: IntPair = 1):
    """``(Ho, Wo)`` of the core for an ``Hi x Wi`` input."""
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = (_hw(kernel_size, "kernel_size", 1), _hw(stride, "stride", 1),
                                              _hw(padding, "padding", 0), _hw(dilation, "dilation", 1))
    eh, ew = Hi + 2 * ph - (dh * (kh - 1) + 1), Wi + 2 * pw - (dw * (kw - 1) + 1)
    return (eh // sh + 1 if eh >= 0 else 0), (ew // sw + 1 if ew >= 0 else 0)


def packed_channels(groups: int, taps: int) -> int:
    """``C`` of DCNv4's packed ``offset_mask``: ``groups * 3 * taps`` rounded up to a multiple of 8."""
    return (groups * 3 * taps + 7) // 8 * 8


def _geometry(input, kernel_size, stride, padding, dilation, offset_scale):
    if input.dim() != 5:
        raise ValueError(f"`input` should be [N, Hi, Wi, G, D], but got {tuple(input.shape)}.")
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = (_hw(kernel_size, "kernel_size", 1), _hw(stride, "stride", 1),
                                              _hw(padding, "padding", 0), _hw(dilation, "dilation", 1))
    if not isinstance(offset_scale, (int, float)) or not math.isfinite(offset_scale):
        raise ValueError(f"`offset_scale` should be a finite number, but got {offset_scale!r}.")
    N, Hi, Wi, G, D = input.shape
    Ho, Wo = output_size(Hi, Wi, (kh, kw), (sh, sw), (ph, pw), (dh, dw))
    return (Hi, Wi, Ho, Wo, kh, kw, sh, sw, ph, pw, dh, dw)


def _split_views(input, offset, mask, geom):
    """offset ``[N, Ho, Wo, G, K, 2]`` or ``[N, Ho, Wo, G K 2]``, mask ``[N, Ho, Wo, G, K]`` or ``[N, Ho, Wo, G K]`` -> both in
    their long forms."""
    N, _, _, G, _ = input.shape
    Ho, Wo, K = geom[2], geom[3], geom[4] * geom[5]
    if offset.numel() != N * Ho * Wo * G * K * 2 or tuple(offset.shape[:3]) != (N, Ho, Wo):
        raise ValueError(f"`offset` should be [{N}, {Ho}, {Wo}, {G}, {K}, 2], but got {tuple(offset.shape)}.")
    if mask.numel() != N * Ho * Wo * G * K or tuple(mask.shape[:3]) != (N, Ho, Wo):
        raise ValueError(f"`mask` should be [{N}, {Ho}, {Wo}, {G}, {K}], but got {tuple(mask.shape)}.")
    return offset.reshape(N, Ho, Wo, G, K, 2), mask.reshape(N, Ho, Wo, G, K)


def _packed_views(input, offset_mask, geom):
    """DCNv4's packed tensor -> the (offset, mask) views into it."""
    N, _, _, G, _ = input.shape
    Ho, Wo, K = geom[2], geom[3], geom[4] * geom[5]
    C = packed_channels(G, K)
    if tuple(offset_mask.shape) != (N, Ho, Wo, C):
        raise ValueError(f"`offset_mask` should be [{N}, {Ho}, {Wo}, {C}], but got {tuple(offset_mask.shape)}.")
    per = offset_mask[..., :G * 3 * K].reshape(N, Ho, Wo, G, 3 * K)
    return per[..., :2 * K].reshape(N, Ho, Wo, G, K, 2), per[..., 2 * K:]


def native_deformable_conv_core(input, offset, mask, kernel_size, stride=1, padding=1, dilation=1, offset_scale=1.0,
                                softmax=False):
    """The operator in plain PyTorch, differentiable through autograd: one ``grid_sample`` over all taps.  16-bit tensors
    compute in float32."""
    geom = _geometry(input, kernel_size, stride, padding, dilation, offset_scale)
    offset, mask = _split_views(input, offset, mask, geom)
    Hi, Wi, Ho, Wo, kh, kw, sh, sw, ph, pw, dh, dw = geom
    N, _, _, G, D = input.shape
    K = kh * kw
    dt = torch.promote_types(torch.promote_types(input.dtype, offset.dtype), mask.dtype)
    ct = torch.float32 if dt in (torch.float16, torch.bfloat16) else dt
    if N * Ho * Wo * G * D == 0 or Hi * Wi == 0:
        return (input.sum() * 0 + offset.sum() * 0 + mask.sum() * 0).to(dt) + input.new_zeros((N, Ho, Wo, G, D), dtype=dt)
    dev = input.device
    cx, cy = (dw * (kw - 1)) // 2, (dh * (kh - 1)) // 2
    k = torch.arange(K, device=dev)
    tap_x = ((k // kh) * dw - cx).to(ct)
    tap_y = ((k % kh) * dh - cy).to(ct)
    base_x = (torch.arange(Wo, device=dev) * sw - pw + cx).to(ct).view(1, 1, Wo, 1, 1)
    base_y = (torch.arange(Ho, device=dev) * sh - ph + cy).to(ct).view(1, Ho, 1, 1, 1)
    off = offset.to(ct)
    lx = base_x + offset_scale * (tap_x + off[..., 0])
    ly = base_y + offset_scale * (tap_y + off[..., 1])
    grid = torch.stack([2 * (lx + 0.5) / Wi - 1, 2 * (ly + 0.5) / Hi - 1], -1)  # [N, Ho, Wo, G, K, 2]
    grid = grid.permute(0, 3, 1, 2, 4, 5).reshape(N * G, Ho * Wo, K, 2)
    img = input.to(ct).permute(0, 3, 4, 1, 2).reshape(N * G, D, Hi, Wi)
    sampled = torch.nn.functional.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    m = mask.to(ct)
    m = m.softmax(-1) if softmax else m
    m = m.permute(0, 3, 1, 2, 4).reshape(N * G, 1, Ho * Wo, K)
    out = (sampled * m).sum(-1)  # [N G, D, Ho Wo]
    return out.reshape(N, G, D, Ho, Wo).permute(0, 3, 4, 1, 2).contiguous().to(dt)


# ------------------------------------------------------------------------------------------
# launcher pair over msda_dcn_{fwd,bwd}_<dtype>
# ------------------------------------------------------------------------------------------
def _strided(t: torch.Tensor, long_dims: int):
    """(row stride, group stride) in elements of a view whose last `long_dims` dims are a group's data, which must be
    contiguous, with the pixels [N, Ho, Wo] laid out densely in front."""
    st, sh = t.stride(), t.shape
    inner = 1
    for d in range(t.dim() - 1, t.dim() - 1 - long_dims, -1):
        if sh[d] > 1 and st[d] != inner:
            return None
        inner *= sh[d]
    row = st[2]
    if (sh[1] > 1 and st[1] != row * sh[2]) or (sh[0] > 1 and st[0] != row * sh[2] * sh[1]):
        return None
    return row, st[3]


def _launch_views(offset, mask):
    """offset [N, Ho, Wo, G, K, 2] and mask [N, Ho, Wo, G, K] as the kernels read them: in place when their groups' data
    are contiguous runs under dense pixels (two dense tensors, or views into a packed one), else dense copies."""
    so, sm = _strided(offset, 2), _strided(mask, 1)
    if so is None or sm is None:
        offset, mask = offset.contiguous(), mask.contiguous()
        so, sm = _strided(offset, 2), _strided(mask, 1)
    return offset, mask, so + sm


def dcn_hip_fwd(input, offset, mask, geom, offset_scale, softmax):
    """Enqueue ``msda_dcn_fwd_<dtype>`` on the current stream (no host sync) -> ``out [N, Ho, Wo, G, D]``."""
    _check_devices(input, offset, mask)
    N, _, _, G, D = input.shape
    input = input.contiguous()
    offset, mask, strides = _launch_views(offset, mask)
    out = torch.empty((N, geom[2], geom[3], G, D), dtype=input.dtype, device=input.device)
    symbol = f"msda_dcn_fwd_{_SUFFIX[input.dtype]}"
    args = (input.data_ptr(), offset.data_ptr(), mask.data_ptr(), out.data_ptr(), N, geom[0], geom[1], G, D, *geom[2:],
            float(offset_scale), int(bool(softmax)), *strides)
    if not _fused_run("msda_dcn_fwd", symbol, input.device, getattr(_lib.load(), symbol), args):
        raise ValueError(f"{symbol}: {_lib.load().msda_last_error().decode(errors='replace')}")
    return out


def dcn_hip_bwd(out_grad, input, offset, mask, grad_offset, grad_mask, geom, offset_scale, softmax, need_input=True):
    """``grad_input`` (None when not needed) from ``msda_dcn_bwd_<dtype>``; ``grad_offset`` / ``grad_mask`` are views laid
    out as ``offset`` / ``mask`` that the kernel writes in place (both or neither).  A frozen input allocates no workspace."""
    _check_devices(out_grad, input, offset, mask)
    N, _, _, G, D = input.shape
    K = geom[4] * geom[5]
    input, out_grad = input.contiguous(), out_grad.contiguous()
    offset, mask, strides = _launch_views(offset, mask)
    if grad_offset is not None and _launch_views(grad_offset, grad_mask)[2] != strides:
        raise ValueError("`grad_offset` / `grad_mask` should be laid out as `offset` / `mask`.")
    lib = _lib.load()
    g_in, ws, ws_bytes = None, None, 0
    if need_input:
        g_in = torch.empty_like(input)
        ws_bytes = int(lib.msda_dcn_bwd_workspace_bytes(N, geom[0], geom[1], G, D, geom[2], geom[3], K, input.element_size(), 0))
        ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=input.device)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    symbol = f"msda_dcn_bwd_{_SUFFIX[input.dtype]}"
    args = (out_grad.data_ptr(), input.data_ptr(), offset.data_ptr(), mask.data_ptr(), ptr(g_in), ptr(grad_offset), ptr(grad_mask),
            N, geom[0], geom[1], G, D, *geom[2:], float(offset_scale), int(bool(softmax)), *strides, 0, ptr(ws), ws_bytes)
    if not _fused_run("msda_dcn_bwd", symbol, input.device, getattr(lib, symbol), args):
        raise ValueError(f"{symbol}: {lib.msda_last_error().decode(errors='replace')}")
    return g_in


class _DcnFunction(Function):
    """``second`` None: ``first`` is the packed offset_mask; else (offset, mask) in their long forms."""

    @staticmethod
    @custom_fwd(device_type="cuda")
    def forward(ctx, input, first, second, geom, offset_scale, softmax):
        offset, mask = _packed_views(input, first, geom) if second is None else (first, second)
        ctx.save_for_backward(input, first, second)
        ctx.args = (geom, offset_scale, softmax)
        return dcn_hip_fwd(input, offset, mask, geom, offset_scale, softmax)

    @staticmethod
    @once_differentiable
    @custom_bwd(device_type="cuda")
    def backward(ctx, out_grad):
        input, first, second = ctx.saved_tensors
        geom, offset_scale, softmax = ctx.args
        packed = second is None
        need_input = ctx.needs_input_grad[0]
        need_sample = ctx.needs_input_grad[1] or (not packed and ctx.needs_input_grad[2])
        g_first = g_second = g_off = g_msk = None
        if need_sample and packed:
            g_first = torch.empty_like(first, memory_format=torch.contiguous_format)
            G, K = input.shape[3], geom[4] * geom[5]
            g_first[..., G * 3 * K:] = 0  # the padded tail, which no kernel writes
            g_off, g_msk = _packed_views(input, g_first, geom)
        elif need_sample:
            g_first, g_second = (torch.empty(t.shape, dtype=t.dtype, device=t.device) for t in (first, second))
            g_off, g_msk = g_first, g_second
        offset, mask = _packed_views(input, first.contiguous(), geom) if packed else (first.contiguous(), second.contiguous())
        g_in = None
        if need_input or need_sample:
            g_in = dcn_hip_bwd(out_grad, input, offset, mask, g_off, g_msk, geom, offset_scale, softmax, need_input)
        return g_in, g_first, g_second, None, None, None


def _use_kernels(input, *others) -> bool:
    return (input.device.type == "cuda" and input.dtype in _SUFFIX and all(t.dtype == input.dtype for t in others)
            and not torch.compiler.is_compiling() and input.numel() > 0 and all(t.numel() > 0 for t in others)
            and _lib.has_dcn())


def deformable_conv_core(input: torch.Tensor, offset: torch.Tensor, mask: torch.Tensor, kernel_size: IntPair,
                         stride: IntPair = 1, padding: IntPair = 1, dilation: IntPair = 1, offset_scale: float = 1.0,
                         softmax: bool = False) -> torch.Tensor:
    """Differentiable deformable convolution core (DCNv3 with ``softmax=True``, DCNv4 without).

    Args:
        input: ``[N, Hi, Wi, G, D]`` channels-last.
        offset: ``[N, Ho, Wo, G, K, 2]`` (or flattened ``[N, Ho, Wo, G K 2]``), (x, y) per tap, ``K = kh kw``, tap
            ``k = i kh + j`` with ``i`` the window's column.
        mask: ``[N, Ho, Wo, G, K]`` (or ``[N, Ho, Wo, G K]``): the modulation, softmaxed over K when ``softmax``.
        kernel_size, stride, padding, dilation: an int or an ``(h, w)`` pair each.
        offset_scale: factor on the tap's displacement from the window centre.

    Returns:
        ``[N, Ho, Wo, G, D]``.
    """
    geom = _geometry(input, kernel_size, stride, padding, dilation, offset_scale)
    offset, mask = _split_views(input, offset, mask, geom)
    if _use_kernels(input, offset, mask):
        return _DcnFunction.apply(input, offset, mask, geom, float(offset_scale), bool(softmax))
    return native_deformable_conv_core(input, offset, mask, kernel_size, stride, padding, dilation, offset_scale, softmax)


def deformable_conv_core_packed(input: torch.Tensor, offset_mask: torch.Tensor, kernel_size: IntPair, stride: IntPair = 1,
                                padding: IntPair = 1, dilation: IntPair = 1, offset_scale: float = 1.0,
                                softmax: bool = False) -> torch.Tensor:
    """The core on DCNv4's packed ``offset_mask [N, Ho, Wo, C]`` — per group ``2K`` offsets then ``K`` mask values,
    ``C = packed_channels(G, K)`` — read in place; its gradient comes back in the same layout with the padded tail zero."""
    geom = _geometry(input, kernel_size, stride, padding, dilation, offset_scale)
    offset, mask = _packed_views(input, offset_mask, geom)
    if _use_kernels(input, offset_mask):
        return _DcnFunction.apply(input, offset_mask, None, geom, float(offset_scale), bool(softmax))
    return native_deformable_conv_core(input, offset, mask, kernel_size, stride, padding, dilation, offset_scale, softmax)


def last_launch_info() -> dict:
    """``_lib.last_launch_info()`` and this family's own key: ``dcn_window``, 1 when the last deformable-convolution
    kernel staged its input window in LDS."""
    info = _lib.last_launch_info()
    info["dcn_window"] = int(_lib.load().msda_last_launch_info(b"dcn_window"))
    return info


class DeformableConv(nn.Module):
    """A thin DCNv3 / DCNv4 block on channels-last maps ``[N, H, W, channels]``: ``value_proj``, ONE ``offset_mask`` layer
    that produces the packed layout (zero-initialised: the block starts on the regular grid), the core, ``output_proj``.
    ``softmax=True`` is DCNv3's normalised modulation, False DCNv4's raw one.  The offsets are predicted per input pixel,
    so the geometry must keep the map's size (the depthwise convolution in front of the published blocks is not part of it).
    """

    def __init__(self, channels: int, groups: int, kernel_size: IntPair = 3, stride: IntPair = 1, padding: IntPair = 1,
                 dilation: IntPair = 1, offset_scale: float = 1.0, softmax: bool = False):
        super().__init__()
        if channels % groups != 0:
            raise ValueError(f"Channels ({channels=}) should be divisible by the number of groups ({groups=}).")
        kh, kw = _hw(kernel_size, "kernel_size", 1)
        self.channels, self.groups, self.taps = channels, groups, kh * kw
        self.kernel_size, self.stride, self.padding, self.dilation = kernel_size, stride, padding, dilation
        self.offset_scale, self.softmax = offset_scale, softmax
        self.value_proj = nn.Linear(channels, channels)
        self.offset_mask = nn.Linear(channels, packed_channels(groups, self.taps))
        self.output_proj = nn.Linear(channels, channels)
        self.reset_parameters()

    def reset_parameters(self) -> None:
        nn.init.zeros_(self.offset_mask.weight)
        nn.init.zeros_(self.offset_mask.bias)
        for layer in (self.value_proj, self.output_proj):
            nn.init.xavier_uniform_(layer.weight)
            nn.init.zeros_(layer.bias)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        N, H, W, C = x.shape
        if output_size(H, W, self.kernel_size, self.stride, self.padding, self.dilation) != (H, W):
            raise ValueError("DeformableConv predicts one set of offsets per input pixel: the geometry should keep the map's size.")
        value = projection(self.value_proj, x.reshape(N, H * W, C)).reshape(N, H, W, self.groups, C // self.groups)
        om = projection(self.offset_mask, x.reshape(N, H * W, C)).reshape(N, H, W, -1)
        out = deformable_conv_core_packed(value, om.to(value.dtype), self.kernel_size, self.stride, self.padding, self.dilation,
                                          self.offset_scale, self.softmax)
        return projection(self.output_proj, out.reshape(N, H * W, C)).reshape(N, H, W, C)
