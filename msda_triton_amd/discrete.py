"""Discrete (nearest-pixel) sampling: ``multiscale_deformable_attention(..., sampling_mode="discrete")``.

Every sample reads exactly one pixel, chosen by rounding, and nothing is interpolated::

    ix = clamp(trunc(x * w + 0.5), 0, w - 1)        iy = clamp(trunc(y * h + 0.5), 0, h - 1)
    out[b, q, head, :] += attention_weight * value[b, start_l + iy * w + ix, head, :]

which is transformers' ``multi_scale_deformable_attention_v2(..., method="discrete")`` (D-FINE / DEIMv2 / RT-DETRv2) and
*not* ``grid_sample(mode="nearest")``: the ``+ 0.5`` applies to ``x * w``, there is no pixel-centre shift, out-of-range
samples clamp to the edge pixel.  ``padding_mode`` / ``align_corners`` have no meaning here; the call accepts only
``"border"`` / ``False``.  The sampling points get **no** gradient (autograd returns ``None`` for them, as with
transformers' own core); ``img`` and ``attention_weights`` get theirs.

The per-level-count layout (``[B, Q, H, S, 2]`` / ``[B, Q, H, S]``, level-major) is the native one; the uniform 6-D
layout is the same call with equal counts on a view.  GPU tensors run ``msda_fwd_discrete_<dtype>`` /
``msda_bwd_discrete_<dtype>`` (csrc/msda_discrete.hpp), host tensors the index formulation below.

The pixel index is computed in fp32 (fp64 for fp64 inputs) as a rounded multiply followed by a rounded add, on the GPU
as on the host, so for fp32 inputs both pick the same pixel bit for bit.  For float16 / bfloat16 coordinates the GPU
computes the index in fp32 from the stored 16-bit value; transformers computes it in 16 bits there, which can pick the
neighbouring pixel when ``x * w`` is not representable in 16 bits.
"""
from __future__ import annotations

from typing import Sequence

import torch
from torch.amp import custom_bwd, custom_fwd
from torch.autograd.function import Function, once_differentiable

from . import _ext, _lib
from . import functional as F
from .ragged import _counts_array, _prepare, check_points_per_level

SAMPLING_MODES = ("bilinear", "discrete")


def check_discrete_mode(padding_mode, align_corners) -> None:
    if padding_mode != "border" or bool(align_corners):
        raise ValueError('sampling_mode="discrete" reads one clamped pixel per sample: `padding_mode` and `align_corners` '
                         f'have no meaning and must be "border" / False, but got {padding_mode!r} / {align_corners!r}.')


def native_discrete(img, img_shapes, sampling_points, attention_weights, counts):
    """Host formulation: per level an index gather (differentiable in ``img`` and ``attention_weights``; the index is an
    integer tensor, so ``sampling_points`` gets no gradient)."""
    B, I, H, D = img.shape
    Q = sampling_points.shape[1]
    dt = torch.result_type(img, sampling_points)
    idt = dt if dt in (torch.float32, torch.float64) else torch.float32  # (16-bit: the index in fp32, as the kernels)
    value = img.to(dt).permute(0, 2, 1, 3)                                  # [B, H, I, D]
    pts = sampling_points.detach().to(idt).permute(0, 2, 1, 3, 4)           # [B, H, Q, S, 2]
    weights = attention_weights.to(dt).permute(0, 2, 1, 3)                  # [B, H, Q, S]
    pixel = []
    start = 0
    s0 = 0
    for (h, w), P in zip(img_shapes.tolist(), counts):
        xy = pts[:, :, :, s0:s0 + P]
        ix = torch.clamp(torch.trunc(xy[..., 0] * w + 0.5), 0, w - 1)
        iy = torch.clamp(torch.trunc(xy[..., 1] * h + 0.5), 0, h - 1)
        pixel.append(start + torch.nan_to_num(iy, nan=0.0).to(torch.int64) * w + torch.nan_to_num(ix, nan=0.0).to(torch.int64))
        start += h * w
        s0 += P
    pixel = torch.cat(pixel, dim=-1)                                        # [B, H, Q, S]
    S = pixel.shape[-1]
    rows = torch.gather(value, 2, pixel.reshape(B, H, Q * S, 1).expand(B, H, Q * S, D)).reshape(B, H, Q, S, D)
    out = (rows * weights.unsqueeze(-1)).sum(dim=3)                         # [B, H, Q, D]
    return out.permute(0, 2, 1, 3).contiguous()


_WS_BYTES: dict = {}
_BWD_SUPPORTED: dict = {}


def check_backward_supported(img, sampling_points, counts) -> None:
    B, I, H, D = img.shape
    Q = sampling_points.shape[1]
    key = (B, I, H, D, Q, counts, sampling_points.element_size())
    ok = _BWD_SUPPORTED.get(key)
    if ok is None:
        ok = _BWD_SUPPORTED[key] = bool(_lib.load_discrete().msda_bwd_discrete_supported(
            B, I, H, D, Q, len(counts), _counts_array(counts), sampling_points.element_size()))
    if not ok:
        raise ValueError(f"`img` requires a gradient, but grad_value is not available for this shape (I={I} pixels per "
                         f"plane, D={D}, Q={Q}).  Detach `img` or split the pyramid.")


def discrete_hip_fwd(img, img_shapes, sampling_points, attention_weights, counts):
    lib = _lib.load_discrete()
    suf, img, vrow, pts, att, shapes = _prepare(img, img_shapes, sampling_points, attention_weights)
    B, I, H, D = img.shape
    Q = pts.shape[1]
    out = torch.empty((B, Q, H, D), dtype=pts.dtype, device=img.device)
    fn = getattr(lib, f"msda_fwd_discrete_{suf}")
    with F._OnDevice(img.device):
        rc = fn(img.data_ptr(), shapes.data_ptr(), pts.data_ptr(), att.data_ptr(), out.data_ptr(), B, I, H, D, Q,
                len(counts), _counts_array(counts), vrow, F._stream_ptr(img.device))
    _lib.check(rc, f"msda_fwd_discrete_{suf}")
    return out


def discrete_hip_bwd(out_grad, img, img_shapes, sampling_points, attention_weights, counts, needs=(True, True),
                     level_cells: int = 0, ws_passes: int = 0):
    """(grad_img, grad_attention_weights); ``needs`` says which of the two are wanted (the other is ``None``).
    ``ws_passes``: size the grad_value workspace for that many passes over the batch (0: the library's default)."""
    lib = _lib.load_discrete()
    suf, img, vrow, pts, att, shapes = _prepare(img, img_shapes, sampling_points, attention_weights)
    B, I, H, D = img.shape
    Q, S = pts.shape[1], pts.shape[3]
    cdt = pts.dtype
    out_grad = out_grad.contiguous().to(cdt)
    want_value, want_attn = bool(needs[0]), bool(needs[1])
    g_img = torch.empty((B, I, H, D), dtype=img.dtype, device=img.device) if want_value else None
    g_att = torch.empty((B, Q, H, S), dtype=cdt, device=img.device) if want_attn else None
    if want_value or want_attn:
        arr = _counts_array(counts)
        ws, ws_bytes = None, 0
        if want_value:
            flags = _lib.ws_passes(ws_passes) if ws_passes else 0
            key = (B, I, H, D, Q, counts, cdt, img.dtype, _lib.OPTION_EPOCH, int(level_cells), flags)
            ws_bytes = _WS_BYTES.get(key)
            if ws_bytes is None:
                ws_bytes = _WS_BYTES[key] = int(lib.msda_bwd_discrete_workspace_bytes(
                    B, I, H, D, Q, len(counts), arr, pts.element_size(), img.element_size(), int(level_cells), flags))
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=img.device)
        fn = getattr(lib, f"msda_bwd_discrete_{suf}")
        with F._OnDevice(img.device):
            rc = fn(out_grad.data_ptr(), img.data_ptr(), shapes.data_ptr(), pts.data_ptr(), att.data_ptr(),
                    g_img.data_ptr() if want_value else None, g_att.data_ptr() if want_attn else None, B, I, H, D, Q,
                    len(counts), arr, int(level_cells), vrow, ws.data_ptr() if ws is not None else None, ws_bytes,
                    F._stream_ptr(img.device))
        _lib.check(rc, f"msda_bwd_discrete_{suf}")
    return g_img, g_att


class _HipDiscreteFunction(Function):

    @staticmethod
    @custom_fwd(device_type="cuda", cast_inputs=torch.float32)  # under autocast the op runs in fp32, as the ragged call
    def forward(ctx, img, img_shapes, sampling_points, attention_weights, counts, level_cells=0):
        if ctx.needs_input_grad[0]:
            check_backward_supported(img, sampling_points, counts)
        ctx.save_for_backward(img, img_shapes, sampling_points, attention_weights)
        ctx.counts, ctx.level_cells = counts, level_cells
        return discrete_hip_fwd(img, img_shapes, sampling_points, attention_weights, counts)

    @staticmethod
    @once_differentiable
    @custom_bwd(device_type="cuda")
    def backward(ctx, out_grad):
        img, img_shapes, sampling_points, attention_weights = ctx.saved_tensors
        g_img, g_att = discrete_hip_bwd(out_grad, img, img_shapes, sampling_points, attention_weights, ctx.counts,
                                        (ctx.needs_input_grad[0], ctx.needs_input_grad[3]), ctx.level_cells)
        return g_img, None, None, g_att, None, None  # (the sampling points: no gradient in this mode)


def discrete_multiscale_deformable_attention(img, img_shapes, sampling_points, attention_weights, padding_mode,
                                             align_corners, points_per_level: Sequence[int] = None,
                                             level_shapes=None) -> torch.Tensor:
    """``multiscale_deformable_attention(..., sampling_mode="discrete")``: see the module docstring."""
    check_discrete_mode(padding_mode, align_corners)
    if points_per_level is None:  # the uniform 6-D layout: equal counts on a view
        if sampling_points.dim() != 6 or sampling_points.shape[-1] != 2 or attention_weights.dim() != 5:
            raise ValueError("expected sampling_points [B,N,H,L,P,2] and attention_weights [B,N,H,L,P]; got "
                             f"{tuple(sampling_points.shape)}, {tuple(attention_weights.shape)}")
        if tuple(attention_weights.shape) != tuple(sampling_points.shape[:-1]):
            raise ValueError(f"inconsistent shapes: sampling_points {tuple(sampling_points.shape)}, attention_weights "
                             f"{tuple(attention_weights.shape)}")
        B, Q, H, L, P, _ = sampling_points.shape
        points_per_level = [P] * L
        sampling_points = sampling_points.reshape(B, Q, H, L * P, 2)
        attention_weights = attention_weights.reshape(B, Q, H, L * P)
    counts = check_points_per_level(img, img_shapes, sampling_points, attention_weights, points_per_level)
    if img.device.type != "cuda":
        return native_discrete(img, img_shapes, sampling_points, attention_weights, counts)
    for name, t in (("img", img), ("sampling_points", sampling_points), ("attention_weights", attention_weights)):
        if t.dtype not in F.VALID_DTYPES:
            raise ValueError(f"Dtype of `{name}` should be in {list(F.VALID_DTYPES)}, but got {t.dtype}.")
    if not F._autocast_on() and (sampling_points.dtype != attention_weights.dtype
                                 or not F.dtypes_supported(img.dtype, sampling_points.dtype)):
        raise ValueError(
            "`img`, `sampling_points` and `attention_weights` should share one dtype (or `img` be float16 / bfloat16 "
            f"next to float32 sampling inputs), but got {img.dtype}, {sampling_points.dtype}, {attention_weights.dtype}.")
    level_cells = F.level_cells_of(level_shapes, len(counts), img.shape[1])
    if torch.compiler.is_compiling():  # traced by torch.compile / export: the registered custom ops
        from .compile_op import compiled_discrete_multiscale_deformable_attention
        return compiled_discrete_multiscale_deformable_attention(img, img_shapes, sampling_points, attention_weights,
                                                                 counts, level_cells)
    F._check_devices(img, img_shapes, sampling_points, attention_weights)
    # the C++ autograd node (csrc/msda_torch_ext.cpp), under the conditions the ragged call uses its own: decoder-sized
    # calls spend more host time than device time.  The Python Function serves autocast (fp32 casting), per-kernel
    # timing and a binding built without the node.
    ext = _ext.load()
    if ext is not None and hasattr(ext, "msda_discrete") and F.KernelTimer.active is None and not F._autocast_on():
        _lib.load_discrete()
        if img.requires_grad and torch.is_grad_enabled():
            check_backward_supported(img, sampling_points, counts)
        return ext.msda_discrete(img, F._shapes_i64(img_shapes), sampling_points, attention_weights, level_cells,
                                 list(counts))
    if F._autocast_on() and img.dtype in (torch.bfloat16, torch.float16) and sampling_points.dtype == torch.float32 \
            and attention_weights.dtype == torch.float32:
        # the mixed storage under autocast: served in place (the Function's fp32 casting would copy the pyramid)
        with torch.autocast("cuda", enabled=False):
            return _HipDiscreteFunction.apply(img, img_shapes, sampling_points, attention_weights, counts, level_cells)
    return _HipDiscreteFunction.apply(img, img_shapes, sampling_points, attention_weights, counts, level_cells)
