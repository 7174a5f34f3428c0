"""Key-aware deformable attention: the weights of a query's samples are a softmax over what was sampled.

    K_s = bilinear(key_h, p_s)               V_s = bilinear(value_h, p_s)
    z_s = scale * <query[b, q, h, :], K_s>   a = softmax_s(z)               out[b, q, h, :] = sum_s a_s * V_s

(Lite-DETR's key-aware deformable attention, the sampled-key attention of the DAT family.)  ``key`` is a second pyramid
of ``value``'s shape, sampled at the same points; the softmax runs over a (b, q, head) unit's ``L * P`` scores.

  key_aware_deformable_attention   the function: gfx950 kernels for GPU tensors of one supported dtype, else PyTorch
  keyaware_hip_fwd / keyaware_hip_bwd   the launcher pair over ``msda_keyaware_{fwd,bwd}_<dtype>`` (include/msda_hip.h)
  KeyAwareDeformableAttention      the module: value / key / query / output projections and a sampling-offset layer

The kernels never materialise the sampled keys ``[B, Q, H, L * P, D]``, and both pyramid gradients come from the
scatter-free grad_value pipeline.  Padding masks compose: zero-fill both pyramids
(``functional.apply_value_mask``).
"""
from __future__ import annotations

import math
from typing import Literal, Optional, Tuple

import torch
from torch import nn
from torch.amp import custom_bwd, custom_fwd
from torch.autograd.function import Function, once_differentiable

from . import _lib
from ._linear import projection
from .functional import (_SUFFIX, _check_devices, _fused_run, _padding_code, _shapes_i64, _value_rows, level_cells_of)


def _dims(query, key, value, img_shapes, sampling_points):
    if query.dim() != 4 or key.dim() != 4 or value.dim() != 4 or sampling_points.dim() != 6:
        raise ValueError(
            "expected query [B,N,H,C], key and value [B,I,H,C], sampling_points [B,N,H,L,P,2]; got "
            f"{tuple(query.shape)}, {tuple(key.shape)}, {tuple(value.shape)}, {tuple(sampling_points.shape)}")
    B, Q, H, D = query.shape
    I = value.shape[1]  # noqa: E741
    L, P = sampling_points.shape[3:5]
    if tuple(key.shape) != tuple(value.shape) or tuple(value.shape) != (B, I, H, D) or \
            tuple(sampling_points.shape) != (B, Q, H, L, P, 2):
        raise ValueError(
            f"inconsistent shapes: query {tuple(query.shape)}, key {tuple(key.shape)}, value {tuple(value.shape)}, "
            f"sampling_points {tuple(sampling_points.shape)}")
    if tuple(img_shapes.shape) != (L, 2):
        raise ValueError(f"`img_shapes` should be [{L}, 2], but got {tuple(img_shapes.shape)}.")
    return B, I, H, D, Q, L, P


def native_key_aware_deformable_attention(query, key, value, img_shapes, sampling_points, padding_mode, align_corners,
                                          scale, level_shapes=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The operator in plain PyTorch, differentiable through autograd -> ``(out, attn)``: per level one ``grid_sample`` on
    each pyramid, the scores as a dot product with the query's head row, one softmax over all ``L * P`` of them, and the
    contraction with the sampled values.  16-bit tensors compute in float32.  Reads ``img_shapes`` on the host unless
    ``level_shapes`` (the same pairs as host numbers) is given."""
    _padding_code(padding_mode)
    B, I, H, D, Q, L, P = _dims(query, key, value, img_shapes, sampling_points)  # noqa: E741
    dt = torch.promote_types(torch.promote_types(query.dtype, key.dtype), torch.promote_types(value.dtype, sampling_points.dtype))
    ct = torch.float32 if dt in (torch.float16, torch.bfloat16) else dt
    kp = key.to(ct).permute(0, 2, 3, 1).reshape(B * H, D, I)
    vp = value.to(ct).permute(0, 2, 3, 1).reshape(B * H, D, I)
    qh = query.to(ct).permute(0, 2, 1, 3).reshape(B * H, Q, D)
    grid = (2 * sampling_points.to(ct) - 1).permute(0, 2, 3, 1, 4, 5)  # [B, H, L, Q, P, 2] in grid_sample's [-1, 1]
    if L * P == 0:
        return query.new_zeros((B, Q, H, D), dtype=dt), query.new_zeros((B, Q, H, L, P), dtype=dt)
    scores, sampled = [], []
    start = 0
    for lvl, (h, w) in enumerate(img_shapes.tolist() if level_shapes is None else level_shapes):
        h, w = int(h), int(w)
        g = grid[:, :, lvl].reshape(B * H, Q, P, 2)
        ks, vs = (torch.nn.functional.grid_sample(t[:, :, start:start + h * w].reshape(B * H, D, h, w), g, mode="bilinear",
                                                  padding_mode=padding_mode, align_corners=align_corners) for t in (kp, vp))
        scores.append(torch.einsum("nqd,ndqp->nqp", qh, ks))
        sampled.append(vs)  # [B*H, D, Q, P]
        start += h * w
    attn = (torch.cat(scores, dim=-1) * scale).softmax(dim=-1)  # [B*H, Q, L*P]
    out = torch.einsum("nqs,ndqs->nqd", attn, torch.cat(sampled, dim=-1))
    return (out.reshape(B, H, Q, D).permute(0, 2, 1, 3).contiguous().to(dt),
            attn.reshape(B, H, Q, L, P).permute(0, 2, 1, 3, 4).contiguous().to(dt))


# ------------------------------------------------------------------------------------------
# launcher pair over msda_keyaware_{fwd,bwd}_<dtype>
# ------------------------------------------------------------------------------------------
def _prepare(query, key, value, img_shapes, sampling_points, padding_mode, *more):
    """Device and dtype checks, and every tensor as the kernels take it -> (suffix, padding code, query, key, value,
    value_row_stride, shapes, sampling_points, *more contiguous in the common dtype).  Both pyramids share ONE row stride:
    padded rows (``functional.padded_value_rows``) are read in place when both have them, else both are copied dense."""
    _check_devices(query, key, value, img_shapes, sampling_points, *more)
    pad = _padding_code(padding_mode)
    dt = query.dtype
    if dt not in _SUFFIX or any(t.dtype != dt for t in (key, value, sampling_points)):
        raise ValueError("`query`, `key`, `value` and `sampling_points` should share one of float32, float64, bfloat16, "
                         f"float16, but got {[t.dtype for t in (query, key, value, sampling_points)]}.")
    (value_, vrow), (key_, krow) = _value_rows(value), _value_rows(key)
    if vrow != krow:
        value_, key_, vrow = value.contiguous(), key.contiguous(), 0
    more = tuple(t.contiguous() if t.dtype == dt else t.contiguous().to(dt) for t in more)
    return (_SUFFIX[dt], pad, query.contiguous(), key_, value_, vrow, _shapes_i64(img_shapes), sampling_points.contiguous()) + more


def keyaware_hip_fwd(query, key, value, img_shapes, sampling_points, padding_mode, align_corners, scale):
    """Enqueue ``msda_keyaware_fwd_<dtype>`` on the current stream (no host sync) -> ``(out [B,Q,H,D], attn [B,Q,H,L,P])``."""
    B, I, H, D, Q, L, P = _dims(query, key, value, img_shapes, sampling_points)  # noqa: E741
    suf, pad, query, key, value, vrow, shapes, pts = _prepare(query, key, value, img_shapes, sampling_points, padding_mode)
    out = torch.empty((B, Q, H, D), dtype=query.dtype, device=query.device)
    attn = torch.empty((B, Q, H, L, P), dtype=query.dtype, device=query.device)
    symbol = f"msda_keyaware_fwd_{suf}"
    args = (query.data_ptr(), key.data_ptr(), value.data_ptr(), shapes.data_ptr(), pts.data_ptr(), out.data_ptr(), attn.data_ptr(),
            B, I, H, D, L, P, Q, pad, int(bool(align_corners)), float(scale), vrow)
    if not _fused_run("msda_keyaware_fwd", symbol, query.device, getattr(_lib.load(), symbol), args):
        raise ValueError(f"{symbol}: {_lib.load().msda_last_error().decode(errors='replace')}")
    return out, attn


def keyaware_hip_bwd(out_grad, query, key, value, img_shapes, sampling_points, attn, padding_mode, align_corners, scale,
                     needs=(True, True, True, True), level_cells: int = 0):
    """``(grad_query, grad_key, grad_value, grad_sampling_points)`` from ``msda_keyaware_bwd_<dtype>``; entries not in
    ``needs`` are None.  Gradients are fully written by the kernels and not pre-zeroed; a frozen pyramid skips its pass,
    and with both frozen no workspace is allocated."""
    B, I, H, D, Q, L, P = _dims(query, key, value, img_shapes, sampling_points)  # noqa: E741
    suf, pad, query, key, value, vrow, shapes, pts, out_grad, attn = _prepare(
        query, key, value, img_shapes, sampling_points, padding_mode, out_grad, attn)
    need_q, need_k, need_v, need_p = (bool(n) for n in needs)
    want_sample = need_q or need_p
    dev, dt = query.device, query.dtype
    g_q = torch.empty((B, Q, H, D), dtype=dt, device=dev) if want_sample else None
    g_p = torch.empty((B, Q, H, L, P, 2), dtype=dt, device=dev) if want_sample else None
    g_k = torch.empty((B, I, H, D), dtype=dt, device=dev) if need_k else None
    g_v = torch.empty((B, I, H, D), dtype=dt, device=dev) if need_v else None
    if not (want_sample or need_k or need_v):
        return None, None, None, None
    lib = _lib.load()
    ws, ws_bytes = None, 0
    if need_k or need_v:
        ws_bytes = int(lib.msda_keyaware_bwd_workspace_bytes(B, I, H, D, L, P, Q, query.element_size(), 0))
        ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    symbol = f"msda_keyaware_bwd_{suf}"
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    args = (out_grad.data_ptr(), query.data_ptr(), key.data_ptr(), value.data_ptr(), shapes.data_ptr(), pts.data_ptr(),
            attn.data_ptr(), ptr(g_q), ptr(g_k), ptr(g_v), ptr(g_p), B, I, H, D, L, P, Q, pad, int(bool(align_corners)),
            float(scale), int(level_cells), vrow, ptr(ws), ws_bytes)
    if not _fused_run("msda_keyaware_bwd", symbol, dev, getattr(lib, symbol), args):
        raise ValueError(f"{symbol}: {lib.msda_last_error().decode(errors='replace')}")
    return (g_q if need_q else None), g_k, g_v, (g_p if need_p else None)


class _KeyAwareFunction(Function):

    @staticmethod
    @custom_fwd(device_type="cuda")
    def forward(ctx, query, key, value, img_shapes, sampling_points, padding_mode, align_corners, scale, level_cells):
        out, attn = keyaware_hip_fwd(query, key, value, img_shapes, sampling_points, padding_mode, align_corners, scale)
        ctx.save_for_backward(query, key, value, img_shapes, sampling_points, attn)
        ctx.args = (padding_mode, align_corners, scale, int(level_cells))
        ctx.mark_non_differentiable(attn)
        return out, attn

    @staticmethod
    @once_differentiable
    @custom_bwd(device_type="cuda")
    def backward(ctx, out_grad, _attn_grad):
        query, key, value, img_shapes, sampling_points, attn = ctx.saved_tensors
        padding_mode, align_corners, scale, level_cells = ctx.args
        needs = (ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2], ctx.needs_input_grad[4])
        g_q, g_k, g_v, g_p = keyaware_hip_bwd(out_grad, query, key, value, img_shapes, sampling_points, attn, padding_mode,
                                              align_corners, scale, needs, level_cells)
        return g_q, g_k, g_v, None, g_p, None, None, None, None


def key_aware_deformable_attention(
    query: torch.Tensor,
    key: torch.Tensor,
    value: torch.Tensor,
    img_shapes: torch.Tensor,
    sampling_points: torch.Tensor,
    padding_mode: Literal["border", "zeros"] = "border",
    align_corners: bool = False,
    scale: Optional[float] = None,
    level_shapes=None,
    return_attention: bool = False,
):
    """Differentiable key-aware deformable attention.

    Args:
        query: ``[batch, num_queries, num_heads, num_channels]``.
        key, value: flattened pyramids ``[batch, num_image, num_heads, num_channels]`` of one shape.
        img_shapes: ``[num_levels, 2]`` integer tensor of (height, width).
        sampling_points: ``[batch, num_queries, num_heads, num_levels, num_points, 2]`` in (x, y) order, normalised to
            [0, 1]; both pyramids are sampled there.
        padding_mode, align_corners: as in ``multiscale_deformable_attention``.
        scale: factor on the scores; default ``num_channels ** -0.5``.
        level_shapes: optional — the same (height, width) pairs as host numbers (``functional.level_cells_of``).
        return_attention: also return the softmaxed weights ``[batch, num_queries, num_heads, num_levels, num_points]``
            (detached: they carry no gradient).

    Returns:
        ``[batch, num_queries, num_heads, num_channels]``, or ``(out, attention)``.

    GPU tensors of one dtype among float32, float64, bfloat16, float16 run the gfx950 kernels and never fall back; host
    tensors, traced calls, mixed dtypes and a library without the kernels run the PyTorch formulation.
    """
    _padding_code(padding_mode)
    B, I, H, D, Q, L, P = _dims(query, key, value, img_shapes, sampling_points)  # noqa: E741
    if scale is None:
        scale = D ** -0.5 if D > 0 else 1.0
    if not isinstance(scale, (int, float)) or not math.isfinite(scale):
        raise ValueError(f"`scale` should be a finite number, but got {scale!r}.")
    one_dtype = query.dtype in _SUFFIX and all(t.dtype == query.dtype for t in (key, value, sampling_points))
    if query.device.type == "cuda" and one_dtype and not torch.compiler.is_compiling() and query.numel() > 0 and \
            L * P > 0 and I > 0 and _lib.has_keyaware():
        level_cells = level_cells_of(level_shapes, L, I)
        out, attn = _KeyAwareFunction.apply(query, key, value, img_shapes, sampling_points, padding_mode,
                                            bool(align_corners), float(scale), level_cells)
    else:
        out, attn = native_key_aware_deformable_attention(query, key, value, img_shapes, sampling_points, padding_mode,
                                                          align_corners, scale, level_shapes)
        attn = attn.detach()
    return (out, attn) if return_attention else out


class KeyAwareDeformableAttention(nn.Module):
    """Key-aware deformable attention with its projections: value, key and query projections, a sampling-offset layer and
    an output projection — and NO attention-weight layer: the weights are the softmax of the query's dot products with
    the keys sampled at its points.

    Args:
        embed_dim: feature dimension of the pyramid and the queries; divisible by ``num_heads``.
        num_heads, num_levels, num_points: heads, pyramid levels, sampling points per level.
        padding_mode, align_corners: of the bilinear sampler.
        scale: factor on the scores; default ``(embed_dim / num_heads) ** -0.5``.

    The sampling offsets start on Deformable-DETR's grid: zero weight, and a bias that points head ``h`` in direction
    ``2 pi h / num_heads`` with point ``p`` of every level ``p + 1`` steps out.
    """

    def __init__(self, embed_dim: int, num_heads: int, num_levels: int, num_points: int,
                 padding_mode: Literal["border", "zeros"] = "border", align_corners: bool = False,
                 scale: Optional[float] = None):
        super().__init__()
        if embed_dim % num_heads != 0:
            raise ValueError(f"Embedding dimension ({embed_dim=}) should be divisible by number of heads ({num_heads=}).")
        _padding_code(padding_mode)
        self.embed_dim, self.num_heads, self.num_levels, self.num_points = embed_dim, num_heads, num_levels, num_points
        self.padding_mode, self.align_corners, self.scale = padding_mode, align_corners, scale
        self.value_proj = nn.Linear(embed_dim, embed_dim)
        self.key_proj = nn.Linear(embed_dim, embed_dim)
        self.query_proj = nn.Linear(embed_dim, embed_dim)
        self.sampling_offsets = nn.Linear(embed_dim, num_heads * num_levels * num_points * 2)
        self.output_proj = nn.Linear(embed_dim, embed_dim)
        self.reset_parameters()

    def reset_parameters(self) -> None:
        H, L, P = self.num_heads, self.num_levels, self.num_points
        nn.init.zeros_(self.sampling_offsets.weight)
        thetas = torch.arange(H, dtype=torch.float32) * (2.0 * math.pi / H)
        grid = torch.stack([thetas.cos(), thetas.sin()], -1)
        grid = (grid / grid.abs().max(-1, keepdim=True)[0]).view(H, 1, 1, 2).repeat(1, L, P, 1)
        grid = grid * torch.arange(1, P + 1, dtype=torch.float32).view(1, 1, P, 1)
        with torch.no_grad():
            self.sampling_offsets.bias.copy_(grid.reshape(-1))
        for layer in (self.value_proj, self.key_proj, self.query_proj, self.output_proj):
            nn.init.xavier_uniform_(layer.weight)
            nn.init.zeros_(layer.bias)

    def forward(self, img: torch.Tensor, img_shapes: torch.Tensor, queries: torch.Tensor, reference_points: torch.Tensor,
                level_shapes=None, return_attention: bool = False):
        """``img`` ``[batch, num_image, embed_dim]`` (the flattened pyramid keys and values are projected from),
        ``img_shapes`` ``[num_levels, 2]``, ``queries`` ``[batch, num_queries, embed_dim]``, ``reference_points``
        ``[batch, num_queries, 2]`` (x, y) in [0, 1]: a sample sits at ``ref + offset / (h_l, w_l)`` (the module's rule for
        points, in ``img_shapes``' stored order).  Returns ``[batch, num_queries, embed_dim]`` (and the attention weights)."""
        B, I, _ = img.shape  # noqa: E741
        N = queries.shape[1]
        H, L, P = self.num_heads, self.num_levels, self.num_points
        if reference_points.shape[-1] != 2:
            raise ValueError(f"`reference_points` should have the last dim 2, but got {reference_points.shape[-1]}.")
        D = self.embed_dim // H
        value = projection(self.value_proj, img).reshape(B, I, H, D)
        key = projection(self.key_proj, img).reshape(B, I, H, D)
        query = projection(self.query_proj, queries).reshape(B, N, H, D)
        offsets = projection(self.sampling_offsets, queries).reshape(B, N, H, L, P, 2)
        points = reference_points[:, :, None, None, None, :] + offsets / img_shapes[:, None, :]
        res = key_aware_deformable_attention(query, key, value, img_shapes, points.to(query.dtype), self.padding_mode,
                                             self.align_corners, self.scale, level_shapes, return_attention)
        out, attn = res if return_attention else (res, None)
        out = projection(self.output_proj, out.reshape(B, N, self.embed_dim))
        return (out, attn) if return_attention else out
