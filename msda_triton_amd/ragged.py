"""Per-level sampling-point counts (``points_per_level``): the D-FINE / DEIMv2 decoders' layout.

Sampling points are ``[B, Q, H, S, 2]`` and attention weights ``[B, Q, H, S]`` with ``S = sum(points_per_level)``; the
sample axis is level-major, samples ``[start_l, start_l + P_l)`` belong to level ``l`` (transformers'
``multi_scale_deformable_attention_v2``).  A list of equal counts is the uniform 6-D call on a view; unequal counts run
``msda_fwd_ragged_<dtype>`` / ``msda_bwd_ragged_<dtype>`` on the GPU (no padding to ``max(P_l)``) and per-level
``grid_sample`` over the level's slice of the sample axis on the host.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence, Tuple

import torch
from torch.amp import custom_bwd, custom_fwd
from torch.autograd.function import Function, once_differentiable

from . import _ext, _lib
from . import functional as F


def check_points_per_level(img, img_shapes, sampling_points, attention_weights, points_per_level) -> Tuple[int, ...]:
    """Validate the ragged layout; returns the counts as a tuple of ints.  Raises ``ValueError`` with the reason."""
    counts = tuple(int(p) for p in points_per_level)
    L = int(img_shapes.shape[0]) if img_shapes.dim() >= 1 else -1
    if img_shapes.dim() != 2 or img_shapes.shape[1] != 2:
        raise ValueError(f"`img_shapes` should be [L, 2], but got {tuple(img_shapes.shape)}.")
    if len(counts) != L:
        raise ValueError(f"`points_per_level` has {len(counts)} entries, but `img_shapes` describes {L} levels.")
    if any(p < 1 for p in counts):
        raise ValueError(f"every entry of `points_per_level` should be at least 1, but got {list(counts)}.")
    if img.dim() != 4 or sampling_points.dim() != 5 or sampling_points.shape[-1] != 2:
        raise ValueError("with `points_per_level`, expected img [B,I,H,C] and sampling_points [B,N,H,S,2]; got "
                         f"{tuple(img.shape)}, {tuple(sampling_points.shape)}")
    B, _, H, _ = img.shape
    B2, Q, H2, S, _ = sampling_points.shape
    if sum(counts) != S:
        raise ValueError(f"`points_per_level` sums to {sum(counts)}, but `sampling_points` has S = {S} samples per head.")
    if (B2, H2) != (B, H):
        raise ValueError(f"inconsistent shapes: img {tuple(img.shape)}, sampling_points {tuple(sampling_points.shape)}")
    if tuple(attention_weights.shape) != (B, Q, H, S):
        raise ValueError(f"`attention_weights` should be {(B, Q, H, S)} with `points_per_level`, but got "
                         f"{tuple(attention_weights.shape)}.")
    return counts


def native_ragged(img, img_shapes, sampling_points, attention_weights, padding_mode, align_corners, counts):
    """Host formulation: per level, ``grid_sample`` over the level's slice of the sample axis (differentiable)."""
    F._padding_code(padding_mode)
    B, I, H, D = img.shape
    Q = sampling_points.shape[1]
    dt = torch.result_type(img, sampling_points)
    planes = img.to(dt).permute(0, 2, 3, 1).reshape(B * H, D, I)          # [B*H, D, I]
    grid = (2 * sampling_points.to(dt) - 1).permute(0, 2, 1, 3, 4)         # [B, H, Q, S, 2]
    weights = attention_weights.to(dt).permute(0, 2, 1, 3)                 # [B, H, Q, S]
    out = planes.new_zeros((B * H, Q, D))
    start, s0 = 0, 0
    for (h, w), P in zip(img_shapes.tolist(), counts):
        level = planes[:, :, start:start + h * w].reshape(B * H, D, h, w)
        g = grid[:, :, :, s0:s0 + P].reshape(B * H, Q, P, 2)
        sampled = torch.nn.functional.grid_sample(level, g, mode="bilinear", padding_mode=padding_mode,
                                                  align_corners=align_corners)  # [B*H, D, Q, P]
        out = out + torch.einsum("ndqp,nqp->nqd", sampled, weights[:, :, :, s0:s0 + P].reshape(B * H, Q, P))
        start += h * w
        s0 += P
    return out.reshape(B, H, Q, D).permute(0, 2, 1, 3).contiguous()


def _counts_array(counts) -> ctypes.Array:
    return (ctypes.c_int32 * len(counts))(*counts)


_WS_BYTES: dict = {}
_BWD_SUPPORTED: dict = {}


def check_backward_supported(img, sampling_points, counts) -> None:
    B, I, H, D = img.shape
    Q = sampling_points.shape[1]
    key = (B, I, H, D, Q, counts, sampling_points.element_size())
    ok = _BWD_SUPPORTED.get(key)
    if ok is None:
        ok = _BWD_SUPPORTED[key] = bool(_lib.load().msda_bwd_ragged_supported(
            B, I, H, D, Q, len(counts), _counts_array(counts), sampling_points.element_size()))
    if not ok:
        raise ValueError(f"`img` requires a gradient, but grad_value is not available for this shape (I={I} pixels per "
                         f"plane, D={D}, Q={Q}).  Detach `img` or split the pyramid.")


def _prepare(img, img_shapes, sampling_points, attention_weights):
    F._check_devices(img, img_shapes, sampling_points, attention_weights)
    cdt = sampling_points.dtype
    if attention_weights.dtype != cdt:
        raise ValueError(f"`sampling_points` and `attention_weights` should share one dtype, but got {cdt} and "
                         f"{attention_weights.dtype}.")
    suf = F._suffix_for(img.dtype, cdt)
    (img, vrow) = F._value_rows(img)
    return suf, img, vrow, sampling_points.contiguous(), attention_weights.contiguous(), F._shapes_i64(img_shapes)


def ragged_hip_fwd(img, img_shapes, sampling_points, attention_weights, padding_mode, align_corners, counts):
    pad = F._padding_code(padding_mode)
    suf, img, vrow, pts, att, shapes = _prepare(img, img_shapes, sampling_points, attention_weights)
    B, I, H, D = img.shape
    Q = pts.shape[1]
    out = torch.empty((B, Q, H, D), dtype=pts.dtype, device=img.device)
    fn = getattr(_lib.load(), f"msda_fwd_ragged_{suf}")
    with F._OnDevice(img.device):
        rc = fn(img.data_ptr(), shapes.data_ptr(), pts.data_ptr(), att.data_ptr(), out.data_ptr(), B, I, H, D, Q,
                len(counts), _counts_array(counts), pad, int(bool(align_corners)), vrow, F._stream_ptr(img.device))
    _lib.check(rc, f"msda_fwd_ragged_{suf}")
    return out


def ragged_hip_bwd(out_grad, img, img_shapes, sampling_points, attention_weights, padding_mode, align_corners, counts,
                   needs=(True, True, True), level_cells: int = 0):
    pad = F._padding_code(padding_mode)
    suf, img, vrow, pts, att, shapes = _prepare(img, img_shapes, sampling_points, attention_weights)
    B, I, H, D = img.shape
    Q, S = pts.shape[1], pts.shape[3]
    cdt = pts.dtype
    out_grad = out_grad.contiguous().to(cdt)
    want_value, want_sample = bool(needs[0]), bool(needs[1] or needs[2])
    g_img = torch.empty((B, I, H, D), dtype=img.dtype, device=img.device) if want_value else None
    g_pts = torch.empty((B, Q, H, S, 2), dtype=cdt, device=img.device) if want_sample else None
    g_att = torch.empty((B, Q, H, S), dtype=cdt, device=img.device) if want_sample else None
    if want_value or want_sample:
        lib = _lib.load()
        arr = _counts_array(counts)
        ws, ws_bytes = None, 0
        if want_value:
            flags = _lib.WS_RECORDS_IN_GRADS if (want_sample and g_pts.data_ptr() % 16 == 0 and g_att.data_ptr() % 16 == 0
                                                 and g_img.data_ptr() % 16 == 0
                                                 and _lib.get_option("overlap") != 1) else 0
            key = (B, I, H, D, Q, counts, cdt, img.dtype, _lib.OPTION_EPOCH, int(level_cells), flags)
            ws_bytes = _WS_BYTES.get(key)
            if ws_bytes is None:
                ws_bytes = _WS_BYTES[key] = int(lib.msda_bwd_ragged_workspace_bytes(
                    B, I, H, D, Q, len(counts), arr, pts.element_size(), img.element_size(), int(level_cells), flags))
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=img.device)
        fn = getattr(lib, f"msda_bwd_ragged_{suf}")
        with F._OnDevice(img.device):
            rc = fn(out_grad.data_ptr(), img.data_ptr(), shapes.data_ptr(), pts.data_ptr(), att.data_ptr(),
                    g_img.data_ptr() if want_value else None, g_pts.data_ptr() if want_sample else None,
                    g_att.data_ptr() if want_sample else None, B, I, H, D, Q, len(counts), arr, pad,
                    int(bool(align_corners)), int(level_cells), vrow, ws.data_ptr() if ws is not None else None,
                    ws_bytes, F._stream_ptr(img.device))
        _lib.check(rc, f"msda_bwd_ragged_{suf}")
    return g_img, (g_pts if needs[1] else None), (g_att if needs[2] else None)


class _HipRaggedFunction(Function):

    @staticmethod
    @custom_fwd(device_type="cuda", cast_inputs=torch.float32)  # under autocast the op runs in fp32, as the 6-D call
    def forward(ctx, img, img_shapes, sampling_points, attention_weights, padding_mode, align_corners, counts,
                level_cells=0):
        if ctx.needs_input_grad[0]:
            check_backward_supported(img, sampling_points, counts)
        ctx.save_for_backward(img, img_shapes, sampling_points, attention_weights)
        ctx.padding_mode, ctx.align_corners, ctx.counts, ctx.level_cells = padding_mode, align_corners, counts, level_cells
        return ragged_hip_fwd(img, img_shapes, sampling_points, attention_weights, padding_mode, align_corners, counts)

    @staticmethod
    @once_differentiable
    @custom_bwd(device_type="cuda")
    def backward(ctx, out_grad):
        img, img_shapes, sampling_points, attention_weights = ctx.saved_tensors
        needs = (ctx.needs_input_grad[0], ctx.needs_input_grad[2], ctx.needs_input_grad[3])
        g_img, g_pts, g_att = ragged_hip_bwd(out_grad, img, img_shapes, sampling_points, attention_weights,
                                             ctx.padding_mode, ctx.align_corners, ctx.counts, needs, ctx.level_cells)
        return g_img, None, g_pts, g_att, None, None, None, None


def ragged_multiscale_deformable_attention(img, img_shapes, sampling_points, attention_weights, padding_mode,
                                           align_corners, points_per_level: Sequence[int],
                                           level_shapes=None) -> torch.Tensor:
    """``multiscale_deformable_attention(..., points_per_level=...)``: see the module docstring."""
    counts = check_points_per_level(img, img_shapes, sampling_points, attention_weights, points_per_level)
    B, Q, H, S, _ = sampling_points.shape
    L = len(counts)
    if all(p == counts[0] for p in counts):  # equal counts: the uniform call on a view
        P = counts[0]
        return F.multiscale_deformable_attention(img, img_shapes, sampling_points.reshape(B, Q, H, L, P, 2),
                                                 attention_weights.reshape(B, Q, H, L, P), padding_mode, align_corners,
                                                 level_shapes)
    if img.device.type != "cuda":
        return native_ragged(img, img_shapes, sampling_points, attention_weights, padding_mode, align_corners, counts)
    for name, t in (("img", img), ("sampling_points", sampling_points), ("attention_weights", attention_weights)):
        if t.dtype not in F.VALID_DTYPES:
            raise ValueError(f"Dtype of `{name}` should be in {list(F.VALID_DTYPES)}, but got {t.dtype}.")
    if not F._autocast_on() and (sampling_points.dtype != attention_weights.dtype
                                 or not F.dtypes_supported(img.dtype, sampling_points.dtype)):
        raise ValueError(
            "`img`, `sampling_points` and `attention_weights` should share one dtype (or `img` be float16 / bfloat16 "
            f"next to float32 sampling inputs), but got {img.dtype}, {sampling_points.dtype}, {attention_weights.dtype}.")
    F._padding_code(padding_mode)
    level_cells = F.level_cells_of(level_shapes, L, img.shape[1])
    if torch.compiler.is_compiling():  # traced by torch.compile / export: the registered custom ops
        from .compile_op import compiled_ragged_multiscale_deformable_attention
        return compiled_ragged_multiscale_deformable_attention(img, img_shapes, sampling_points, attention_weights,
                                                               padding_mode, align_corners, counts, level_cells)
    # the C++ autograd node (csrc/msda_torch_ext.cpp): decoder-sized calls spend more host time than device time.  The
    # Python Function serves autocast (fp32 casting), per-kernel timing and a binding built without the node.
    ext = _ext.load()
    if ext is not None and hasattr(ext, "msda_ragged") and F.KernelTimer.active is None and not F._autocast_on():
        F._check_devices(img, img_shapes, sampling_points, attention_weights)
        if img.requires_grad and torch.is_grad_enabled():
            check_backward_supported(img, sampling_points, counts)
        return ext.msda_ragged(img, F._shapes_i64(img_shapes), sampling_points, attention_weights,
                               F._padding_code(padding_mode), bool(align_corners), level_cells, list(counts))
    return _HipRaggedFunction.apply(img, img_shapes, sampling_points, attention_weights, padding_mode,
                                    bool(align_corners), counts, level_cells)
