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
FUSED_BOX_MAX_LEVELS = 8  # msda_*_fused_hfbox_discrete_<dtype>: the level scales ride in the kernel arguments


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


# ------------------------------------------------------------------------------------------
# Hugging Face's box rule in front of discrete sampling (D-FINE / DEIMv2 / RT-DETRv2, decoder_method="discrete"):
# functional.fused_hf_box_core(..., sampling_mode="discrete") on msda_*_fused_hfbox_discrete_<suffix>
# ------------------------------------------------------------------------------------------
def hf_box_discrete_hip_fwd_fused(img, img_shapes, proj, reference_points, counts, offset_scale: float = 0.5):
    """Forward with the softmax, transformers' box rule and the pixel choice done in the kernel
    (``msda_fwd_fused_hfbox_discrete_<suffix>``; ``reference_points`` ``[B, Q, 4]``).  None when the library declines (more
    than 8 levels) or predates these entry points: the caller then composes the prologue around the discrete operator."""
    from .ragged import _scale_array
    if not _lib.has_fused_hfbox_discrete() or len(counts) > FUSED_BOX_MAX_LEVELS:  # (declined without a call)
        return None
    B, I, H, D = img.shape
    B2, Q, H2, S, _ = proj.shape
    if (B2, H2) != (B, H) or tuple(reference_points.shape) != (B, Q, 4):
        raise ValueError(f"inconsistent shapes: img {tuple(img.shape)}, proj {tuple(proj.shape)}, "
                         f"reference_points {tuple(reference_points.shape)}")
    suf, _, img, vrow, shapes, proj, reference_points, _ = F._fused_prepare(img, img_shapes, proj, reference_points)
    fn = getattr(_lib.load(), f"msda_fwd_fused_hfbox_discrete_{suf}")
    out = torch.empty((B, Q, H, D), dtype=proj.dtype, device=img.device)
    ok = F._fused_run("msda_fwd_fused_hfbox_discrete", f"msda_fwd_fused_hfbox_discrete_{suf}", img.device, fn,
                      (img.data_ptr(), shapes.data_ptr(), proj.data_ptr(), reference_points.data_ptr(), out.data_ptr(),
                       B, I, H, D, Q, len(counts), _counts_array(counts), _scale_array(counts), float(offset_scale), vrow))
    return out if ok else None


def hf_box_discrete_hip_bwd_fused(out_grad, img, img_shapes, proj, reference_points, counts, offset_scale: float = 0.5,
                                  need_img: bool = True, level_cells: int = 0, parked_points: bool = False):
    """Backward of the discrete box core (``msda_bwd_fused_hfbox_discrete_<suffix>``): ``(img_grad | None, proj_grad)`` —
    the offset slots of ``proj_grad`` are stored zeros and the boxes have no gradient —, or None when the library declines
    (nothing was launched).  ``parked_points`` (with ``need_img``): two more elements, the sampling points
    ``[B, Q, H, S, 2]`` and the softmaxed weights ``[B, Q, H, S]`` the kernel left at the head of its workspace for the
    grad_value passes, in the arithmetic dtype (float32 for the 16-bit operators)."""
    from .ragged import _scale_array
    if not _lib.has_fused_hfbox_discrete() or len(counts) > FUSED_BOX_MAX_LEVELS:  # (declined without a call)
        return None
    B, I, H, D = img.shape
    _, Q, _, S, _ = proj.shape
    suf, _, img, vrow, shapes, proj, reference_points, out_grad = F._fused_prepare(img, img_shapes, proj, reference_points,
                                                                                   out_grad=out_grad)
    lib = _lib.load()
    fn = getattr(lib, f"msda_bwd_fused_hfbox_discrete_{suf}")
    g_img = torch.empty((B, I, H, D), dtype=img.dtype, device=img.device) if need_img else None
    g_proj = torch.empty((B, Q, H, S, 3), dtype=proj.dtype, device=img.device)
    arr, scale = _counts_array(counts), _scale_array(counts)
    level_cells = int(level_cells)
    ws, ws_bytes = F._fused_workspace(need_img, lib.msda_bwd_fused_hfbox_discrete_workspace_bytes,
                                      (B, I, H, D, Q, len(counts), arr), suf, proj, img, level_cells)
    if not F._fused_run("msda_bwd_fused_hfbox_discrete", f"msda_bwd_fused_hfbox_discrete_{suf}", img.device, fn,
                        (out_grad.data_ptr(), img.data_ptr(), shapes.data_ptr(), proj.data_ptr(), reference_points.data_ptr(),
                         g_img.data_ptr() if need_img else None, g_proj.data_ptr(), B, I, H, D, Q, len(counts), arr, scale,
                         float(offset_scale), level_cells, vrow, ws.data_ptr() if need_img else None, ws_bytes)):
        return None
    res = (g_img, g_proj)
    if parked_points and ws is not None:
        res += F._parked(ws, reference_points, B, Q, H, S, weights=True)
    return res


def _hf_box_discrete_composition(img, img_shapes, proj, reference_points, counts, offset_scale, level_shapes):
    """transformers' box prologue as PyTorch ops around the discrete operator (host tensors, traced calls, whatever the
    fused kernels do not take).  16-bit value / projection next to fp32 boxes: the prologue in fp32, the mixed-storage
    operator, the result back in the projection's dtype."""
    if img.device.type == "cuda" and F.fused_storage_dtypes(img.dtype, proj.dtype, reference_points.dtype):
        pts, att = F.hf_box_sampling_inputs(proj.to(reference_points.dtype), reference_points, counts, offset_scale)
        return discrete_multiscale_deformable_attention(img, img_shapes, pts, att, "border", False, counts,
                                                        level_shapes).to(proj.dtype)
    pts, att = F.hf_box_sampling_inputs(proj, reference_points, counts, offset_scale)
    return discrete_multiscale_deformable_attention(img, img_shapes, pts, att, "border", False, counts, level_shapes)


class _HipFusedHfBoxDiscreteFunction(Function):
    """The discrete box core on ``msda_*_fused_hfbox_discrete_<dtype>`` (autocast: in fp32; the storage suffixes).  When
    the library declines, the prologue runs in PyTorch around the discrete operator's kernels."""

    @staticmethod
    @custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, img, img_shapes, proj, reference_points, counts, offset_scale, level_cells=0):
        ctx.level_cells, ctx.counts, ctx.offset_scale = int(level_cells), counts, float(offset_scale)
        out = hf_box_discrete_hip_fwd_fused(img, img_shapes, proj, reference_points, counts, offset_scale)
        ctx.fused = out is not None  # the backward has the same limits: do not ask twice
        if out is None:
            pts, att = F.hf_box_sampling_inputs(proj.to(reference_points.dtype), reference_points, counts, offset_scale)
            out = discrete_hip_fwd(img, img_shapes, pts, att, counts).to(proj.dtype)
        ctx.save_for_backward(img, img_shapes, proj, reference_points)
        return out

    @staticmethod
    @once_differentiable
    @custom_bwd(device_type="cuda")
    def backward(ctx, out_grad):
        img, img_shapes, proj, reference_points = ctx.saved_tensors
        need_img, _, need_proj = ctx.needs_input_grad[:3]
        counts = ctx.counts
        if ctx.fused and need_proj:
            res = hf_box_discrete_hip_bwd_fused(out_grad, img, img_shapes, proj, reference_points, counts, ctx.offset_scale,
                                                need_img, level_cells=ctx.level_cells)
            if res is not None:
                return res[0], None, res[1], None, None, None, None
        g_img, g_proj, _ = F._composed_backward(
            lambda proj_, ref_: F.hf_box_sampling_inputs(proj_, ref_, counts, ctx.offset_scale),
            lambda g, pts, att, want_img, want_attn: discrete_hip_bwd(g, img, img_shapes, pts, att, counts,
                                                                      (want_img, want_attn), ctx.level_cells),
            out_grad, proj, reference_points, need_img, need_proj, False)
        return g_img, None, g_proj, None, None, None, None


def fused_hf_box_discrete_core(img, img_shapes, proj, reference_points, points_per_level, offset_scale=0.5,
                               level_shapes=None) -> torch.Tensor:
    """:func:`msda_triton_amd.functional.fused_hf_box_core` with ``sampling_mode="discrete"``.  Routing mirrors the
    bilinear core's: host tensors -> the composition; GPU -> the fused kernels (the C++ node, else the Python
    ``Function``); traced -> the composition over the registered discrete custom ops."""
    from .ragged import _box_ref, check_hf_box_args
    counts = check_hf_box_args(img_shapes, proj, reference_points, points_per_level)
    offset_scale = float(offset_scale)
    B, Q, H, S, _ = proj.shape
    on_gpu = img.device.type == "cuda"
    if on_gpu and img_shapes.device != img.device:
        img_shapes = img_shapes.to(img.device)  # (a handful of integers: follow `img`, as the other cores do)
    floating = img.is_floating_point() and proj.is_floating_point() and reference_points.is_floating_point()
    if on_gpu and floating and not torch.compiler.is_compiling() and _lib.has_fused_hfbox_discrete() \
            and len(counts) <= FUSED_BOX_MAX_LEVELS:
        F._check_devices(img, proj, reference_points)
        same = F.dtypes_supported(img.dtype, proj.dtype) and reference_points.dtype == proj.dtype
        if F._autocast_on() or F.fused_storage_dtypes(img.dtype, proj.dtype, reference_points.dtype) or same:
            level_cells = F.level_cells_of(level_shapes, len(counts), img.shape[1])
            ref = _box_ref(reference_points)
            if img.requires_grad and torch.is_grad_enabled():
                check_backward_supported(img, proj, counts)
            node = getattr(getattr(_ext.load(), "box_discrete", None), "msda_fused_hfbox_discrete", None)
            if same and node is not None and F.KernelTimer.active is None \
                    and not F._autocast_on() and img.dim() == 4 and (img.shape[0], img.shape[2]) == (B, H):
                # the C++ autograd node: decoder-sized calls spend more host time than device time
                return node(img, F._shapes_i64(img_shapes), proj, ref, level_cells, list(counts),
                            list(F.hf_box_level_scale(counts)), offset_scale)
            return _HipFusedHfBoxDiscreteFunction.apply(img, img_shapes, proj, ref, counts, offset_scale, level_cells)
    # host tensors, tracing (the discrete operator's registered custom ops) and everything the checks above did not take
    return _hf_box_discrete_composition(img, img_shapes, proj, reference_points, counts, offset_scale, level_shapes)


# ------------------------------------------------------------------------------------------
# the reference module's own rule in front of discrete sampling (MultiscaleDeformableAttention(sampling_mode="discrete")):
# functional.fused_module_core(..., sampling_mode="discrete") on msda_*_fused_discrete_<suffix>
# ------------------------------------------------------------------------------------------
def module_discrete_hip_fwd_fused(img, img_shapes, proj, reference_points, counts):
    """Forward with the softmax, the module's point rule (:func:`msda_triton_amd.ragged.ragged_module_sampling_inputs`) and
    the pixel choice done in the kernel (``msda_fwd_fused_discrete_<suffix>``; ``proj`` ``[B, Q, H, S, 3]``,
    ``reference_points`` ``[B, Q, 2 | 4]``).  None when the library declines (more than 8 levels) or predates these entry
    points: the caller then composes the prologue around the discrete operator."""
    if not _lib.has_module_discrete() or len(counts) > FUSED_BOX_MAX_LEVELS:  # (declined without a call)
        return None
    B, I, H, D = img.shape
    B2, Q, H2, S, _ = proj.shape
    ref_dim = reference_points.shape[-1]
    if (B2, H2) != (B, H) or tuple(reference_points.shape) != (B, Q, ref_dim) or ref_dim not in (2, 4):
        raise ValueError(f"inconsistent shapes: img {tuple(img.shape)}, proj {tuple(proj.shape)}, "
                         f"reference_points {tuple(reference_points.shape)}")
    suf, _, img, vrow, shapes, proj, reference_points, _ = F._fused_prepare(img, img_shapes, proj, reference_points)
    fn = getattr(_lib.load(), f"msda_fwd_fused_discrete_{suf}")
    out = torch.empty((B, Q, H, D), dtype=proj.dtype, device=img.device)
    ok = F._fused_run("msda_fwd_fused_discrete", f"msda_fwd_fused_discrete_{suf}", img.device, fn,
                      (img.data_ptr(), shapes.data_ptr(), proj.data_ptr(), reference_points.data_ptr(), out.data_ptr(),
                       B, I, H, D, Q, len(counts), _counts_array(counts), ref_dim, vrow))
    return out if ok else None


def module_discrete_hip_bwd_fused(out_grad, img, img_shapes, proj, reference_points, counts, need_img: bool = True,
                                  level_cells: int = 0, parked_points: bool = False):
    """Backward of the discrete module core (``msda_bwd_fused_discrete_<suffix>``): ``(img_grad | None, proj_grad)`` — the
    offset slots of ``proj_grad`` are stored zeros and the reference points have no gradient —, or None when the library
    declines (nothing was launched).  ``parked_points``: as :func:`hf_box_discrete_hip_bwd_fused`."""
    if not _lib.has_module_discrete() or len(counts) > FUSED_BOX_MAX_LEVELS:  # (declined without a call)
        return None
    B, I, H, D = img.shape
    _, Q, _, S, _ = proj.shape
    ref_dim = reference_points.shape[-1]
    suf, _, img, vrow, shapes, proj, reference_points, out_grad = F._fused_prepare(img, img_shapes, proj, reference_points,
                                                                                   out_grad=out_grad)
    lib = _lib.load()
    fn = getattr(lib, f"msda_bwd_fused_discrete_{suf}")
    g_img = torch.empty((B, I, H, D), dtype=img.dtype, device=img.device) if need_img else None
    g_proj = torch.empty((B, Q, H, S, 3), dtype=proj.dtype, device=img.device)
    arr = _counts_array(counts)
    level_cells = int(level_cells)
    ws, ws_bytes = F._fused_workspace(need_img, lib.msda_bwd_fused_discrete_workspace_bytes,
                                      (B, I, H, D, Q, len(counts), arr), suf, proj, img, level_cells)
    if not F._fused_run("msda_bwd_fused_discrete", f"msda_bwd_fused_discrete_{suf}", img.device, fn,
                        (out_grad.data_ptr(), img.data_ptr(), shapes.data_ptr(), proj.data_ptr(), reference_points.data_ptr(),
                         g_img.data_ptr() if need_img else None, g_proj.data_ptr(), B, I, H, D, Q, len(counts), arr, ref_dim,
                         level_cells, vrow, ws.data_ptr() if need_img else None, ws_bytes)):
        return None
    res = (g_img, g_proj)
    if parked_points and ws is not None:
        res += F._parked(ws, reference_points, B, Q, H, S, weights=True)
    return res


def _module_discrete_composition(img, img_shapes, proj, reference_points, counts, level_shapes):
    """The module's prologue as PyTorch ops around the discrete operator (host tensors, traced calls, ``fuse_discrete=False``,
    whatever the fused kernels do not take).  16-bit value / projection next to fp32 reference points: the prologue in fp32,
    the mixed-storage operator, the result back in the projection's dtype."""
    from .ragged import ragged_module_sampling_inputs
    if img.device.type == "cuda" and F.fused_storage_dtypes(img.dtype, proj.dtype, reference_points.dtype):
        pts, att = ragged_module_sampling_inputs(proj.to(reference_points.dtype), img_shapes, reference_points, counts)
        return discrete_multiscale_deformable_attention(img, img_shapes, pts, att, "border", False, counts,
                                                        level_shapes).to(proj.dtype)
    pts, att = ragged_module_sampling_inputs(proj, img_shapes, reference_points, counts)
    return discrete_multiscale_deformable_attention(img, img_shapes, pts, att, "border", False, counts, level_shapes)


class _HipFusedModuleDiscreteFunction(Function):
    """The discrete module core on ``msda_*_fused_discrete_<dtype>`` (autocast: in fp32; the storage suffixes).  When the
    library declines, the prologue runs in PyTorch around the discrete operator's kernels."""

    @staticmethod
    @custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, img, img_shapes, proj, reference_points, counts, level_cells=0):
        from .ragged import ragged_module_sampling_inputs
        ctx.level_cells, ctx.counts = int(level_cells), counts
        out = module_discrete_hip_fwd_fused(img, img_shapes, proj, reference_points, counts)
        ctx.fused = out is not None  # the backward has the same limits: do not ask twice
        if out is None:
            pts, att = ragged_module_sampling_inputs(proj.to(reference_points.dtype), img_shapes, reference_points, counts)
            out = discrete_hip_fwd(img, img_shapes, pts, att, counts).to(proj.dtype)
        ctx.save_for_backward(img, img_shapes, proj, reference_points)
        return out

    @staticmethod
    @once_differentiable
    @custom_bwd(device_type="cuda")
    def backward(ctx, out_grad):
        from .ragged import ragged_module_sampling_inputs
        img, img_shapes, proj, reference_points = ctx.saved_tensors
        need_img, _, need_proj = ctx.needs_input_grad[:3]
        counts = ctx.counts
        if ctx.fused and need_proj:
            res = module_discrete_hip_bwd_fused(out_grad, img, img_shapes, proj, reference_points, counts, need_img,
                                                level_cells=ctx.level_cells)
            if res is not None:
                return res[0], None, res[1], None, None, None
        g_img, g_proj, _ = F._composed_backward(
            lambda proj_, ref_: ragged_module_sampling_inputs(proj_, img_shapes, ref_, counts),
            lambda g, pts, att, want_img, want_attn: discrete_hip_bwd(g, img, img_shapes, pts, att, counts,
                                                                      (want_img, want_attn), ctx.level_cells),
            out_grad, proj, reference_points, need_img, need_proj, False)
        return g_img, None, g_proj, None, None, None  # (the reference points: no gradient in this mode)


def fuse_discrete_default(img: torch.Tensor) -> bool:
    """``fuse_discrete=None``: the kernels for the storage dtypes where they were measured faster than the composition in
    every repeat (``msda_triton_amd.module.DISCRETE_IN_KERNELS_DTYPES``), the composition elsewhere."""
    from . import module
    return bool(module.DISCRETE_IN_KERNELS) and img.dtype in module.DISCRETE_IN_KERNELS_DTYPES


def fused_module_discrete_core(img, img_shapes, proj, reference_points, points_per_level=None, level_shapes=None,
                               fuse_discrete=None) -> torch.Tensor:
    """:func:`msda_triton_amd.functional.fused_module_core` with ``sampling_mode="discrete"`` (masks already composed by
    the caller).  ``proj`` is ``[B, Q, H, L, P, 3]``, or ``[B, Q, H, S, 3]`` with ``points_per_level`` — the kernels take the
    per-level-count layout, a uniform count is the same call with equal counts.  Host tensors, traced calls,
    ``fuse_discrete=False`` (``None``: :func:`fuse_discrete_default`), a library without the symbols, more than 8 levels and
    unsupported dtype combinations compose the prologue around the discrete operator."""
    from .ragged import check_proj_points_per_level
    if points_per_level is None:
        if proj.dim() != 6 or proj.shape[-1] != 3:
            raise ValueError(f"expected proj [B,N,H,L,P,3] = (x offset, y offset, logit) per sample; got {tuple(proj.shape)}")
        B, Q, H, L, P, _ = proj.shape
        points_per_level = [P] * L
        proj = proj.reshape(B, Q, H, L * P, 3)
    counts = check_proj_points_per_level(img_shapes, proj, reference_points, points_per_level)
    on_gpu = img.device.type == "cuda"
    if on_gpu and img_shapes.device != img.device:
        img_shapes = img_shapes.to(img.device)  # (a handful of integers: follow `img`, as the other cores do)
    floating = img.is_floating_point() and proj.is_floating_point() and reference_points.is_floating_point()
    if fuse_discrete is None:
        fuse_discrete = fuse_discrete_default(img)
    if fuse_discrete and on_gpu and floating and not torch.compiler.is_compiling() and _lib.has_module_discrete() \
            and len(counts) <= FUSED_BOX_MAX_LEVELS:
        F._check_devices(img, proj, reference_points)
        same = F.dtypes_supported(img.dtype, proj.dtype) and reference_points.dtype == proj.dtype
        if F._autocast_on() or F.fused_storage_dtypes(img.dtype, proj.dtype, reference_points.dtype) or same:
            level_cells = F.level_cells_of(level_shapes, len(counts), img.shape[1])
            if img.requires_grad and torch.is_grad_enabled():
                check_backward_supported(img, proj, counts)
            return _HipFusedModuleDiscreteFunction.apply(img, img_shapes, proj, reference_points, counts, level_cells)
    return _module_discrete_composition(img, img_shapes, proj, reference_points, counts, level_shapes)


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
