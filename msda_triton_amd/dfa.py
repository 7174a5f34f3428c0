"""Deformable feature aggregation (Sparse4D v2 / v3, SparseDrive): multi-camera, multi-level sampling of anchor key points.

    out[b, a, g, :] = sum_{p, c, l} valid(b, a, p, c) * weights[b, a, p, c, l, g]
                                     * bilinear(feature_maps[b, map(c, l), g, :], x * w_cl - 0.5, y * h_cl - 0.5)
    valid = 0 < x < 1 and 0 < y < 1     (strict: a dropped pair contributes nothing on any level)

``feature_maps [B, I, G, D]`` is channels-last with the ``cams * levels`` maps packed camera-major, level-minor
(``I = sum h_cl w_cl``), ``spatial_shapes [cams, levels, 2]`` their ``(h, w)``, ``sampling_locations [B, A, P, cams, 2]``
``(x, y)`` normalised to the camera's image, ``weights [B, A, P, cams, levels, G]``; zeros outside a map, pixel centres at
half-integers (``align_corners=False``).

  deformable_aggregation          the public function
  native_deformable_aggregation   the operator in plain PyTorch: host tensors, traced calls, unsupported dtypes, > 32 maps
  dfa_hip_fwd / dfa_hip_bwd       the launcher pair over ``msda_dfa_{fwd,bwd}_<dtype>`` (include/msda_hip.h)

GPU tensors of one dtype among float32, float64, bfloat16, float16 run the gfx950 kernels: an anchor with all
its channels is a unit, out-of-view pairs are compacted away before any row is requested, and grad_feature_maps comes from
the scatter-free grad_value pipeline.
"""
from __future__ import annotations

import torch
from torch.amp import custom_bwd, custom_fwd
from torch.autograd.function import Function, once_differentiable

from . import _lib
from .functional import _SUFFIX, _check_devices, _fused_run

MAX_MAPS = 32  # MSDA_MAX_LEVELS: cams * levels the kernels' level table holds


def _dims(feature_maps, spatial_shapes, sampling_locations, weights):
    """-> (B, I, G, D, A, P, cams, levels) and whether ``feature_maps`` came flat ``[B, I, C]``."""
    if weights.dim() != 6:
        raise ValueError(f"`weights` should be [B, A, P, cams, levels, G], but got {tuple(weights.shape)}.")
    B, A, P, cams, levels, G = weights.shape
    if tuple(spatial_shapes.shape) != (cams, levels, 2) or spatial_shapes.dtype.is_floating_point:
        raise ValueError(f"`spatial_shapes` should be an integer tensor [{cams}, {levels}, 2], but got "
                         f"{spatial_shapes.dtype} {tuple(spatial_shapes.shape)}.")
    if tuple(sampling_locations.shape) != (B, A, P, cams, 2):
        raise ValueError(f"`sampling_locations` should be [{B}, {A}, {P}, {cams}, 2], but got {tuple(sampling_locations.shape)}.")
    flat = feature_maps.dim() == 3
    if feature_maps.dim() not in (3, 4) or feature_maps.shape[0] != B or (not flat and feature_maps.shape[2] != G):
        raise ValueError(f"`feature_maps` should be [{B}, I, {G}, D] or [{B}, I, C], but got {tuple(feature_maps.shape)}.")
    if flat and (G == 0 or feature_maps.shape[2] % G != 0):
        raise ValueError(f"Channels ({feature_maps.shape[2]}) should be divisible by the number of groups ({G}).")
    I = feature_maps.shape[1]  # noqa: E741
    D = feature_maps.shape[2] // G if flat else feature_maps.shape[3]
    if not (feature_maps.dtype == sampling_locations.dtype == weights.dtype) or not feature_maps.dtype.is_floating_point:
        raise ValueError("`feature_maps`, `sampling_locations` and `weights` should share one floating dtype, but got "
                         f"{feature_maps.dtype}, {sampling_locations.dtype} and {weights.dtype}.")
    return (B, I, G, D, A, P, cams, levels), flat


def native_deformable_aggregation(feature_maps, spatial_shapes, sampling_locations, weights):
    """The operator in plain PyTorch, differentiable through autograd: one ``grid_sample`` per map with the validity mask
    multiplied into the weights.  Reads ``spatial_shapes`` on the host; 16-bit tensors compute in float32."""
    (B, I, G, D, A, P, cams, levels), flat = _dims(feature_maps, spatial_shapes, sampling_locations, weights)
    dt = feature_maps.dtype
    ct = torch.float32 if dt in (torch.float16, torch.bfloat16) else dt
    shapes = spatial_shapes.reshape(cams * levels, 2).tolist()
    if sum(h * w for h, w in shapes) != I:
        raise ValueError(f"`feature_maps` has {I} pixels, but `spatial_shapes` describes {sum(h * w for h, w in shapes)}.")
    loc = sampling_locations.to(ct)
    valid = ((loc > 0) & (loc < 1)).all(-1)                                      # [B, A, P, cams]
    wts = weights.to(ct) * valid[..., None, None].to(ct)
    planes = feature_maps.to(ct).reshape(B, I, G * D).permute(0, 2, 1)           # [B, C, I]
    # (a dropped pair is sampled at the far outside: its own location may be NaN, which 0 * does not silence)
    grid = torch.where(valid[..., None], 2 * loc - 1, torch.full_like(loc, -3.0))
    out = feature_maps.new_zeros((B, A, G, D), dtype=ct) + (planes.sum() + wts.sum()) * 0
    start = 0
    for m, (h, w) in enumerate(shapes):
        cam, lvl = divmod(m, levels)
        if h * w:
            img = planes[:, :, start:start + h * w].reshape(B, G * D, h, w)
            sampled = torch.nn.functional.grid_sample(img, grid[:, :, :, cam], mode="bilinear", padding_mode="zeros",
                                                      align_corners=False)                    # [B, C, A, P]
            out = out + torch.einsum("bgdap,bapg->bagd", sampled.reshape(B, G, D, A, P), wts[:, :, :, cam, lvl])
        start += h * w
    out = out.to(dt)
    return out.reshape(B, A, G * D) if flat else out


# ------------------------------------------------------------------------------------------
# launcher pair over msda_dfa_{fwd,bwd}_<dtype>
# ------------------------------------------------------------------------------------------
def _sizes(feature_maps, sampling_locations, weights):
    B, A, P, cams, levels, G = weights.shape
    return (B, feature_maps.shape[1], G, feature_maps.shape[3], A, P, cams, levels)


def dfa_hip_fwd(feature_maps, spatial_shapes, sampling_locations, weights):
    """Enqueue ``msda_dfa_fwd_<dtype>`` on the current stream (no host sync) -> ``out [B, A, G, D]``, or None where the
    library declines the call (nothing was launched)."""
    _check_devices(feature_maps, spatial_shapes, sampling_locations, weights)
    sizes = _sizes(feature_maps, sampling_locations, weights)
    feature_maps, loc, wts = feature_maps.contiguous(), sampling_locations.contiguous(), weights.contiguous()
    shapes = spatial_shapes.to(torch.int64).contiguous()
    out = torch.empty((sizes[0], sizes[4], sizes[2], sizes[3]), dtype=feature_maps.dtype, device=feature_maps.device)
    symbol = f"msda_dfa_fwd_{_SUFFIX[feature_maps.dtype]}"
    args = (feature_maps.data_ptr(), shapes.data_ptr(), loc.data_ptr(), wts.data_ptr(), out.data_ptr(), *sizes, 0)
    return out if _fused_run("msda_dfa_fwd", symbol, feature_maps.device, getattr(_lib.load(), symbol), args) else None


def dfa_hip_bwd(out_grad, feature_maps, spatial_shapes, sampling_locations, weights, need_maps=True, need_sample=True):
    """``(grad_feature_maps, grad_sampling_locations, grad_weights)`` from ``msda_dfa_bwd_<dtype>``, None where not asked
    for (the last two come together); None instead of the triple where the library declines the call.  Frozen
    ``feature_maps`` allocate no workspace."""
    _check_devices(out_grad, feature_maps, spatial_shapes, sampling_locations, weights)
    sizes = _sizes(feature_maps, sampling_locations, weights)
    feature_maps, loc, wts = feature_maps.contiguous(), sampling_locations.contiguous(), weights.contiguous()
    shapes = spatial_shapes.to(torch.int64).contiguous()
    out_grad = out_grad.contiguous()
    lib = _lib.load()
    g_maps = g_loc = g_wts = ws = None
    ws_bytes = 0
    if need_maps:
        g_maps = torch.empty_like(feature_maps)
        ws_bytes = int(lib.msda_dfa_bwd_workspace_bytes(*sizes, feature_maps.element_size(), 0))
        ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=feature_maps.device)
    if need_sample:
        g_loc, g_wts = torch.empty_like(loc), torch.empty_like(wts)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    symbol = f"msda_dfa_bwd_{_SUFFIX[feature_maps.dtype]}"
    args = (out_grad.data_ptr(), feature_maps.data_ptr(), shapes.data_ptr(), loc.data_ptr(), wts.data_ptr(), ptr(g_maps),
            ptr(g_loc), ptr(g_wts), *sizes, 0, 0, ptr(ws), ws_bytes)
    if not _fused_run("msda_dfa_bwd", symbol, feature_maps.device, getattr(lib, symbol), args):
        return None
    return g_maps, g_loc, g_wts


class _DfaFunction(Function):
    @staticmethod
    @custom_fwd(device_type="cuda")
    def forward(ctx, feature_maps, spatial_shapes, sampling_locations, weights):
        out = dfa_hip_fwd(feature_maps, spatial_shapes, sampling_locations, weights)
        if out is None:
            raise ValueError(f"msda_dfa_fwd: {_lib.load().msda_last_error().decode(errors='replace')}")
        ctx.save_for_backward(feature_maps, spatial_shapes, sampling_locations, weights)
        return out

    @staticmethod
    @once_differentiable
    @custom_bwd(device_type="cuda")
    def backward(ctx, out_grad):
        feature_maps, spatial_shapes, sampling_locations, weights = ctx.saved_tensors
        need_maps = ctx.needs_input_grad[0]
        need_sample = ctx.needs_input_grad[2] or ctx.needs_input_grad[3]
        if not (need_maps or need_sample):
            return None, None, None, None
        grads = dfa_hip_bwd(out_grad, feature_maps, spatial_shapes, sampling_locations, weights, need_maps, need_sample)
        if grads is None:
            raise ValueError(f"msda_dfa_bwd: {_lib.load().msda_last_error().decode(errors='replace')}")
        return grads[0], None, grads[1], grads[2]


def deformable_aggregation(feature_maps: torch.Tensor, spatial_shapes: torch.Tensor, sampling_locations: torch.Tensor,
                           weights: torch.Tensor) -> torch.Tensor:
    """Differentiable deformable feature aggregation.

    Args:
        feature_maps: ``[B, I, G, D]`` (or flat ``[B, I, C]``, ``C = G D``), channels-last, the ``cams * levels`` maps packed
            camera-major, level-minor.
        spatial_shapes: ``[cams, levels, 2]`` integer ``(h, w)``; cameras may differ in size.
        sampling_locations: ``[B, A, P, cams, 2]``, ``(x, y)`` normalised to the camera's image.  A pair outside the open
            unit square is dropped on every level.
        weights: ``[B, A, P, cams, levels, G]``.

    Returns:
        ``[B, A, G, D]`` (``[B, A, C]`` for flat ``feature_maps``).
    """
    (B, I, G, D, A, P, cams, levels), flat = _dims(feature_maps, spatial_shapes, sampling_locations, weights)
    tensors = (feature_maps, sampling_locations, weights)
    if (feature_maps.device.type == "cuda" and feature_maps.dtype in _SUFFIX and not torch.compiler.is_compiling()
            and cams * levels <= MAX_MAPS and all(t.numel() > 0 for t in tensors) and _lib.has_dfa()):
        out = _DfaFunction.apply(feature_maps.reshape(B, I, G, D), spatial_shapes, sampling_locations, weights)
        return out.reshape(B, A, G * D) if flat else out
    return native_deformable_aggregation(feature_maps, spatial_shapes, sampling_locations, weights)
