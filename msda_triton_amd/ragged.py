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


# ------------------------------------------------------------------------------------------
# module core with per-level point counts: raw projection [B, Q, H, S, 3] -> attended values
# ------------------------------------------------------------------------------------------
def check_proj_points_per_level(img_shapes, proj, reference_points, points_per_level) -> Tuple[int, ...]:
    """Validate the module core's ragged layout; returns the counts as a tuple of ints.  Raises ``ValueError``."""
    counts = tuple(int(p) for p in points_per_level)
    if img_shapes.dim() != 2 or img_shapes.shape[1] != 2:
        raise ValueError(f"`img_shapes` should be [L, 2], but got {tuple(img_shapes.shape)}.")
    L = int(img_shapes.shape[0])
    if len(counts) != L:
        raise ValueError(f"`points_per_level` has {len(counts)} entries, but `img_shapes` describes {L} levels.")
    if any(p < 1 for p in counts):
        raise ValueError(f"every entry of `points_per_level` should be at least 1, but got {list(counts)}.")
    if proj.dim() != 5 or proj.shape[-1] != 3:
        raise ValueError("with `points_per_level`, expected proj [B,N,H,S,3] = (x offset, y offset, logit) per sample; "
                         f"got {tuple(proj.shape)}")
    if sum(counts) != proj.shape[3]:
        raise ValueError(f"`points_per_level` sums to {sum(counts)}, but `proj` has S = {proj.shape[3]} samples per head.")
    if reference_points.dim() != 3 or reference_points.shape[-1] not in (2, 4):
        raise ValueError("`reference_points` should be [B,N,2] or [B,N,4] (last dim either 2 or 4), but got "
                         f"{tuple(reference_points.shape)}.")
    if tuple(reference_points.shape[:2]) != tuple(proj.shape[:2]):
        raise ValueError(f"inconsistent shapes: proj {tuple(proj.shape)}, reference_points {tuple(reference_points.shape)}")
    return counts


def ragged_module_sampling_inputs(proj: torch.Tensor, img_shapes: torch.Tensor, reference_points: torch.Tensor, counts):
    """The module's prologue for per-level point counts in plain PyTorch (differentiable): raw projection
    ``[B, N, H, S, 3]`` = (x offset, y offset, attention logit) per sample, ``S = sum(counts)``, level-major ->
    ``(sampling_points [B, N, H, S, 2], attention_weights [B, N, H, S])``.

    * weights: softmax of the logits over all ``S`` samples of a ``(b, n, h)`` unit;
    * 2-d reference points: ``ref + (ox / img_shapes[l][0], oy / img_shapes[l][1])`` — the stored (h, w) order, exactly
      as :func:`msda_triton_amd.functional.module_sampling_inputs` keeps it;
    * 4-d: ``ref_xy + (ox, oy) * ref_wh / (2 * P_l)`` with the count of the sample's own level (D-FINE's
      ``offset * num_points_scale * ref_wh * offset_scale``, ``num_points_scale = 1 / P_l``, ``offset_scale = 0.5``).

    Equal counts are the uniform prologue on a view."""
    counts = check_proj_points_per_level(img_shapes, proj, reference_points, counts)
    B, N, H, S, _ = proj.shape
    L = len(counts)
    if all(p == counts[0] for p in counts):
        pts, att = F.module_sampling_inputs(proj.reshape(B, N, H, L, counts[0], 3), img_shapes, reference_points)
        return pts.reshape(B, N, H, S, 2), att.reshape(B, N, H, S)
    offsets, logits = proj[..., :2], proj[..., 2]
    attention_weights = logits.softmax(dim=-1)
    level = torch.tensor([l for l, p in enumerate(counts) for _ in range(p)], dtype=torch.long, device=img_shapes.device)
    ref = reference_points[:, :, None, None, :]
    if reference_points.shape[-1] == 2:
        sampling_points = ref + offsets / img_shapes[level].to(proj.device)
    else:
        two_p = torch.tensor([2 * p for p in counts for _ in range(p)], dtype=proj.dtype, device=proj.device)
        sampling_points = ref[..., :2] + offsets * ref[..., 2:] / two_p[:, None]
    return sampling_points, attention_weights


def fused_ragged_limits_ok(D: int, elem_size: int, counts) -> bool:
    """Do the fused kernels take these counts (all S samples of a unit in one LDS pass, at most 8 levels)?"""
    key = (D, elem_size)
    limit = F._FUSED_LP_LIMIT.get(key)
    if limit is None:
        limit = F._FUSED_LP_LIMIT[key] = int(_lib.load().msda_fused_lp_limit(*key))
    return sum(counts) <= limit and len(counts) <= 8


def ragged_hip_fwd_fused(img, img_shapes, proj, reference_points, padding_mode, align_corners, counts,
                         value_mask=None, query_mask=None, masks_checked: bool = False) -> Optional[torch.Tensor]:
    """Forward with the softmax and the sampling-point arithmetic done in the kernel prologue
    (``msda_fwd_fused_ragged_<suffix>``).  None when the library declines (S too large for one pass, more than 8 levels)
    or predates these entry points: the caller then takes the unfused route.  ``value_mask`` / ``query_mask``: the masked
    pair ``msda_fwd_fused_ragged_masked_<suffix>`` (:func:`msda_triton_amd.functional._module_mask_args`)."""
    if not _lib.has_fused_ragged():
        return None
    B, I, H, D = img.shape
    B2, Q, H2, S, _ = proj.shape
    if (B2, H2) != (B, H) or reference_points.shape[0] != B:
        raise ValueError(f"inconsistent shapes: img {tuple(img.shape)}, proj {tuple(proj.shape)}, "
                         f"reference_points {tuple(reference_points.shape)}")
    suf, pad, img, vrow, shapes, proj, reference_points, _ = F._fused_prepare(img, img_shapes, proj, reference_points,
                                                                              padding_mode)
    sym, mask_arg, _masks = F._module_mask_args("msda_fwd_fused_ragged", value_mask, query_mask, img, proj, masks_checked)
    fn = getattr(_lib.load(), f"{sym}_{suf}", None)
    if fn is None:
        return None
    out = torch.empty((B, Q, H, D), dtype=proj.dtype, device=img.device)
    ok = F._fused_run("msda_fwd_fused_ragged", f"{sym}_{suf}", img.device, fn,
                      (img.data_ptr(), *mask_arg, shapes.data_ptr(), proj.data_ptr(), reference_points.data_ptr(),
                       out.data_ptr(), B, I, H, D, Q, len(counts), _counts_array(counts), reference_points.shape[-1], pad,
                       int(bool(align_corners)), vrow))
    return out if ok else None


def ragged_hip_bwd_fused(out_grad, img, img_shapes, proj, reference_points, padding_mode, align_corners, counts,
                         need_img: bool = True, level_cells: int = 0, need_ref: bool = True, value_mask=None,
                         query_mask=None, masks_checked: bool = False):
    """Backward of the module core with the prologue's chain rule done in the kernel
    (``msda_bwd_fused_ragged_<suffix>``): ``(img_grad | None, proj_grad, reference_points_grad | None)``, or None when
    the library declines (nothing was launched)."""
    if not _lib.has_fused_ragged():
        return None
    B, I, H, D = img.shape
    _, Q, _, S, _ = proj.shape
    ref_dim = reference_points.shape[-1]
    suf, pad, img, vrow, shapes, proj, reference_points, out_grad = F._fused_prepare(
        img, img_shapes, proj, reference_points, padding_mode, out_grad)
    lib = _lib.load()
    # (the masked pair msda_bwd_fused_ragged_masked_<suffix>; the workspace is the twin's)
    sym, mask_arg, _masks = F._module_mask_args("msda_bwd_fused_ragged", value_mask, query_mask, img, proj, masks_checked)
    fn = getattr(lib, f"{sym}_{suf}", None)
    if fn is None:
        return None
    g_img = torch.empty((B, I, H, D), dtype=img.dtype, device=img.device) if need_img else None
    g_proj = torch.empty((B, Q, H, S, 3), dtype=proj.dtype, device=img.device)
    g_ref_part = torch.empty((B, Q, H, ref_dim), dtype=reference_points.dtype, device=img.device)
    arr = _counts_array(counts)
    level_cells = int(level_cells)
    ws, ws_bytes = F._fused_workspace(need_img, lib.msda_bwd_fused_ragged_workspace_bytes,
                                      (B, I, H, D, Q, len(counts), arr), suf, proj, img, level_cells)
    if not F._fused_run("msda_bwd_fused_ragged", f"{sym}_{suf}", img.device, fn,
                        (out_grad.data_ptr(), img.data_ptr(), *mask_arg, shapes.data_ptr(), proj.data_ptr(),
                         reference_points.data_ptr(), g_img.data_ptr() if need_img else None, g_proj.data_ptr(),
                         g_ref_part.data_ptr(), B, I, H, D, Q, len(counts), arr, ref_dim, pad, int(bool(align_corners)),
                         level_cells, vrow, ws.data_ptr() if need_img else None, ws_bytes)):
        return None
    return g_img, g_proj, (g_ref_part.sum(dim=2) if need_ref else None)


class _HipFusedRaggedModuleCoreFunction(Function):
    """value, raw projection [B, Q, H, S, 3], reference points -> attended values, the prologue and its chain rule inside
    the HIP kernels.  When the library declines (or lacks the entry points) the prologue runs in PyTorch around the ragged
    operator's kernels."""

    @staticmethod
    @custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, img, img_shapes, proj, reference_points, padding_mode, align_corners, counts, level_cells=0,
                value_mask=None, query_mask=None):
        ctx.level_cells, ctx.counts = int(level_cells), counts
        # (value_mask, query_mask: uint8 [B, I] / [B, Q] as check_*_mask returns them, or None:
        # msda_*_fused_ragged_masked_<dtype>; no gradient.  A masked call the library declines is handed back to
        # fused_ragged_module_core, which composes it — the ragged operator has no masked kernels to do that here)
        out = ragged_hip_fwd_fused(img, img_shapes, proj, reference_points, padding_mode, align_corners, counts,
                                   value_mask, query_mask, masks_checked=True)
        ctx.fused = out is not None  # the backward has the same limits: do not ask twice
        if out is None and (value_mask is not None or query_mask is not None):
            raise F.MaskedCallDeclined()
        if out is None:
            pts, att = ragged_module_sampling_inputs(proj.to(reference_points.dtype), img_shapes, reference_points, counts)
            out = ragged_hip_fwd(img, img_shapes, pts, att, padding_mode, align_corners, counts).to(proj.dtype)
        ctx.save_for_backward(img, img_shapes, proj, reference_points, value_mask, query_mask)
        ctx.padding_mode, ctx.align_corners = padding_mode, align_corners
        return out

    @staticmethod
    @once_differentiable
    @custom_bwd(device_type="cuda")
    def backward(ctx, out_grad):
        img, img_shapes, proj, reference_points, value_mask, query_mask = ctx.saved_tensors
        need_img, _, need_proj, need_ref = ctx.needs_input_grad[:4]
        counts = ctx.counts
        # (a masked call stays on the fused backward even when only the pyramid wants a gradient — its grad_proj is then
        # discarded: there is no masked ragged operator to compose from)
        masked = value_mask is not None or query_mask is not None
        if ctx.fused and (need_proj or need_ref or masked):
            res = ragged_hip_bwd_fused(out_grad, img, img_shapes, proj, reference_points, ctx.padding_mode,
                                       ctx.align_corners, counts, need_img, level_cells=ctx.level_cells, need_ref=need_ref,
                                       value_mask=value_mask, query_mask=query_mask, masks_checked=True)
            if res is not None:
                g_img, g_proj, g_ref = res
                return (g_img, None, (g_proj if need_proj else None), (g_ref if need_ref else None), None, None, None, None,
                        None, None)
        if masked:  # (the forward ran masked; only the grad_value pipeline can decline here, and the message says why)
            raise _lib.MSDALibraryError("the masked fused ragged backward was declined after its forward ran: "
                                        + _lib.load().msda_last_error().decode(errors="replace"))
        g_img, g_proj, g_ref = F._composed_backward(
            lambda proj_, ref_: ragged_module_sampling_inputs(proj_, img_shapes, ref_, counts),
            lambda g, pts, att, want_img, want_sample: ragged_hip_bwd(
                g, img, img_shapes, pts, att, ctx.padding_mode, ctx.align_corners, counts,
                (want_img, want_sample, want_sample), ctx.level_cells),
            out_grad, proj, reference_points, need_img, need_proj, need_ref)
        return g_img, None, g_proj, g_ref, None, None, None, None, None, None


def fused_ragged_module_core(img, img_shapes, proj, reference_points, padding_mode, align_corners, points_per_level,
                             level_shapes=None, value_mask=None, query_mask=None, mask_in_kernels: bool = True) -> torch.Tensor:
    """``fused_module_core(..., points_per_level=...)``: ``proj`` is ``[B, Q, H, S, 3]``.  Routing mirrors the uniform
    function: equal counts -> the uniform call on a view; host tensors -> the composition; GPU -> the fused kernels.
    ``value_mask`` / ``query_mask`` / ``mask_in_kernels``: as :func:`msda_triton_amd.functional.fused_module_core` — on GPU
    tensors the masks go into ``msda_*_fused_ragged_masked_<dtype>`` through the Python ``Function``; every other route
    composes ``apply_value_mask`` / ``apply_query_mask``."""
    counts = check_proj_points_per_level(img_shapes, proj, reference_points, points_per_level)
    B, Q, H, S, _ = proj.shape
    L = len(counts)
    if all(p == counts[0] for p in counts):
        return F.fused_module_core(img, img_shapes, proj.reshape(B, Q, H, L, counts[0], 3), reference_points, padding_mode,
                                   align_corners, level_shapes, None, value_mask, query_mask, mask_in_kernels)
    if value_mask is not None or query_mask is not None:
        if value_mask is not None:
            F._validate_value_mask(value_mask, img)
        if query_mask is not None:
            F._validate_query_mask(query_mask, proj)
        if mask_in_kernels and F.module_masks_in_kernels(img, proj, reference_points, S, L):
            if img_shapes.device != img.device:
                img_shapes = img_shapes.to(img.device)
            F._check_devices(img, proj, reference_points)
            F._padding_code(padding_mode)
            try:  # (the masks were validated above: converted once, here)
                return _HipFusedRaggedModuleCoreFunction.apply(
                    img, img_shapes, proj, reference_points, padding_mode, bool(align_corners), counts,
                    F.level_cells_of(level_shapes, L, img.shape[1]),
                    F._mask_bytes(value_mask) if value_mask is not None else F._ones_value_mask(img),
                    None if query_mask is None else F._mask_bytes(query_mask))
            except F.MaskedCallDeclined:
                pass  # nothing was launched: the composition below
        # the composition, as the uniform function states it
        if query_mask is not None:
            out = fused_ragged_module_core(img, img_shapes, F.apply_query_mask(proj, query_mask, 0.0),
                                           F.apply_query_mask(reference_points, query_mask, 0.5), padding_mode,
                                           align_corners, counts, level_shapes, value_mask, None, mask_in_kernels)
            return F.apply_query_mask(out, query_mask, 0.0)
        img = F.apply_value_mask(img, value_mask)
    level_cells = F.level_cells_of(level_shapes, L, img.shape[1])
    on_gpu = img.device.type == "cuda"
    if on_gpu and img_shapes.device != img.device:
        img_shapes = img_shapes.to(img.device)  # (a handful of integers: follow `img`, as the uniform function does)
    if on_gpu:
        F._check_devices(img, proj, reference_points)
    floating = img.is_floating_point() and proj.is_floating_point() and reference_points.is_floating_point()
    if on_gpu and floating and not torch.compiler.is_compiling():
        same = F.dtypes_supported(img.dtype, proj.dtype) and reference_points.dtype == proj.dtype
        if F._autocast_on() or F.fused_storage_dtypes(img.dtype, proj.dtype, reference_points.dtype) or same:
            pad = F._padding_code(padding_mode)
            ext = _ext.load()
            if same and ext is not None and hasattr(ext, "msda_fused_ragged") and F.KernelTimer.active is None and \
                    not F._autocast_on() and _lib.has_fused_ragged() and img.dim() == 4 and \
                    (img.shape[0], img.shape[2]) == (B, H) and fused_ragged_limits_ok(img.shape[3], proj.element_size(), counts):
                # the C++ autograd node: decoder-sized calls spend more host time than device time
                return ext.msda_fused_ragged(img, F._shapes_i64(img_shapes), proj, reference_points, pad,
                                             bool(align_corners), level_cells, list(counts))
            return _HipFusedRaggedModuleCoreFunction.apply(img, img_shapes, proj, reference_points, padding_mode,
                                                           bool(align_corners), counts, level_cells)
    # host tensors, tracing (the ragged operator's registered custom ops) and everything the checks above did not take
    pts, att = ragged_module_sampling_inputs(proj, img_shapes, reference_points, counts)
    return F.multiscale_deformable_attention(img, img_shapes, pts, att, padding_mode, align_corners,
                                             level_shapes=level_shapes, points_per_level=counts)


# ------------------------------------------------------------------------------------------
# the same core for Hugging Face's box rule (D-FINE, DEIMv2, RT-DETRv2): functional.hf_box_sampling_inputs states it
# ------------------------------------------------------------------------------------------
def _scale_array(counts) -> ctypes.Array:
    return (ctypes.c_float * len(counts))(*F.hf_box_level_scale(counts))


def _box_ref(reference_points):
    """``[B, Q, 1, 4]`` -> ``[B, Q, 4]`` (a view; the kernels take one box per query)."""
    return reference_points[:, :, 0, :] if reference_points.dim() == 4 and reference_points.shape[2] == 1 else reference_points


def check_hf_box_args(img_shapes, proj, reference_points, points_per_level) -> Tuple[int, ...]:
    """Validate the box core's layout; returns the counts as a tuple of ints.  Raises ``ValueError``."""
    ref = _box_ref(reference_points)
    if ref.dim() != 3 or ref.shape[-1] != 4:
        raise ValueError("`reference_points` should be [B,N,4] or [B,N,1,4] (one box per query), but got "
                         f"{tuple(reference_points.shape)}.")
    return check_proj_points_per_level(img_shapes, proj, ref, points_per_level)


def hf_box_hip_fwd_fused(img, img_shapes, proj, reference_points, padding_mode, align_corners, counts,
                         offset_scale: float = 0.5) -> Optional[torch.Tensor]:
    """Forward with the softmax and transformers' box rule done in the kernel prologue
    (``msda_fwd_fused_hfbox_<suffix>``; ``reference_points`` ``[B, Q, 4]``).  None when the library declines (S too large
    for one pass, more than 8 levels) or predates these entry points: the caller then takes the unfused route."""
    if not _lib.has_fused_hfbox():
        return None
    B, I, H, D = img.shape
    B2, Q, H2, S, _ = proj.shape
    if (B2, H2) != (B, H) or tuple(reference_points.shape) != (B, Q, 4):
        raise ValueError(f"inconsistent shapes: img {tuple(img.shape)}, proj {tuple(proj.shape)}, "
                         f"reference_points {tuple(reference_points.shape)}")
    suf, pad, img, vrow, shapes, proj, reference_points, _ = F._fused_prepare(img, img_shapes, proj, reference_points,
                                                                              padding_mode)
    fn = getattr(_lib.load(), f"msda_fwd_fused_hfbox_{suf}")
    out = torch.empty((B, Q, H, D), dtype=proj.dtype, device=img.device)
    ok = F._fused_run("msda_fwd_fused_hfbox", f"msda_fwd_fused_hfbox_{suf}", img.device, fn,
                      (img.data_ptr(), shapes.data_ptr(), proj.data_ptr(), reference_points.data_ptr(), out.data_ptr(),
                       B, I, H, D, Q, len(counts), _counts_array(counts), _scale_array(counts), float(offset_scale), 4, pad,
                       int(bool(align_corners)), vrow))
    return out if ok else None


def hf_box_hip_bwd_fused(out_grad, img, img_shapes, proj, reference_points, padding_mode, align_corners, counts,
                         offset_scale: float = 0.5, need_img: bool = True, level_cells: int = 0, need_ref: bool = True,
                         parked_points: bool = False):
    """Backward of the box core with the prologue's chain rule done in the kernel (``msda_bwd_fused_hfbox_<suffix>``):
    ``(img_grad | None, proj_grad, reference_points_grad | None)``, or None when the library declines (nothing was
    launched).  ``parked_points`` (with ``need_img``): a fourth element, the sampling points ``[B, Q, H, S, 2]`` the kernel
    left at the head of its workspace for the grad_value passes — the points the forward sampled, in the arithmetic
    dtype."""
    if not _lib.has_fused_hfbox():
        return None
    B, I, H, D = img.shape
    _, Q, _, S, _ = proj.shape
    suf, pad, img, vrow, shapes, proj, reference_points, out_grad = F._fused_prepare(
        img, img_shapes, proj, reference_points, padding_mode, out_grad)
    lib = _lib.load()
    fn = getattr(lib, f"msda_bwd_fused_hfbox_{suf}")
    g_img = torch.empty((B, I, H, D), dtype=img.dtype, device=img.device) if need_img else None
    g_proj = torch.empty((B, Q, H, S, 3), dtype=proj.dtype, device=img.device)
    g_ref_part = torch.empty((B, Q, H, 4), dtype=reference_points.dtype, device=img.device)
    arr, scale = _counts_array(counts), _scale_array(counts)
    level_cells = int(level_cells)
    # (the fused per-level-count pair's query answers)
    ws, ws_bytes = F._fused_workspace(need_img, lib.msda_bwd_fused_ragged_workspace_bytes,
                                      (B, I, H, D, Q, len(counts), arr), suf, proj, img, level_cells)
    if not F._fused_run("msda_bwd_fused_hfbox", f"msda_bwd_fused_hfbox_{suf}", img.device, fn,
                        (out_grad.data_ptr(), img.data_ptr(), shapes.data_ptr(), proj.data_ptr(), reference_points.data_ptr(),
                         g_img.data_ptr() if need_img else None, g_proj.data_ptr(), g_ref_part.data_ptr(),
                         B, I, H, D, Q, len(counts), arr, scale, float(offset_scale), 4, pad, int(bool(align_corners)),
                         level_cells, vrow, ws.data_ptr() if need_img else None, ws_bytes)):
        return None
    res = (g_img, g_proj, (g_ref_part.sum(dim=2) if need_ref else None))
    if parked_points and ws is not None:
        res += F._parked(ws, reference_points, B, Q, H, S, weights=False)
    return res


def _hf_box_composition(img, img_shapes, proj, reference_points, counts, offset_scale, padding_mode, align_corners,
                        level_shapes):
    """transformers' box prologue as PyTorch ops around the ragged operator (host tensors, traced calls, whatever the fused
    kernels do not take).  16-bit value / projection next to fp32 boxes: the prologue in fp32, the mixed-storage operator,
    the result back in the projection's dtype."""
    if img.device.type == "cuda" and F.fused_storage_dtypes(img.dtype, proj.dtype, reference_points.dtype):
        pts, att = F.hf_box_sampling_inputs(proj.to(reference_points.dtype), reference_points, counts, offset_scale)
        return F.multiscale_deformable_attention(img, img_shapes, pts, att, padding_mode, align_corners,
                                                 level_shapes=level_shapes, points_per_level=counts).to(proj.dtype)
    pts, att = F.hf_box_sampling_inputs(proj, reference_points, counts, offset_scale)
    return F.multiscale_deformable_attention(img, img_shapes, pts, att, padding_mode, align_corners,
                                             level_shapes=level_shapes, points_per_level=counts)


class _HipFusedHfBoxCoreFunction(Function):
    """:class:`_HipFusedRaggedModuleCoreFunction` for transformers' box rule (``msda_*_fused_hfbox_<dtype>``).  When the
    library declines (or lacks the entry points) the prologue runs in PyTorch around the ragged operator's kernels."""

    @staticmethod
    @custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, img, img_shapes, proj, reference_points, padding_mode, align_corners, counts, offset_scale,
                level_cells=0):
        ctx.level_cells, ctx.counts, ctx.offset_scale = int(level_cells), counts, float(offset_scale)
        out = hf_box_hip_fwd_fused(img, img_shapes, proj, reference_points, padding_mode, align_corners, counts, offset_scale)
        ctx.fused = out is not None  # the backward has the same limits: do not ask twice
        if out is None:
            pts, att = F.hf_box_sampling_inputs(proj.to(reference_points.dtype), reference_points, counts, offset_scale)
            out = ragged_hip_fwd(img, img_shapes, pts, att, padding_mode, align_corners, counts).to(proj.dtype)
        ctx.save_for_backward(img, img_shapes, proj, reference_points)
        ctx.padding_mode, ctx.align_corners = padding_mode, align_corners
        return out

    @staticmethod
    @once_differentiable
    @custom_bwd(device_type="cuda")
    def backward(ctx, out_grad):
        img, img_shapes, proj, reference_points = ctx.saved_tensors
        need_img, _, need_proj, need_ref = ctx.needs_input_grad[:4]
        counts = ctx.counts
        if ctx.fused and (need_proj or need_ref):
            res = hf_box_hip_bwd_fused(out_grad, img, img_shapes, proj, reference_points, ctx.padding_mode,
                                       ctx.align_corners, counts, ctx.offset_scale, need_img, level_cells=ctx.level_cells,
                                       need_ref=need_ref)
            if res is not None:
                g_img, g_proj, g_ref = res
                return g_img, None, (g_proj if need_proj else None), (g_ref if need_ref else None), None, None, None, None, None
        g_img, g_proj, g_ref = F._composed_backward(
            lambda proj_, ref_: F.hf_box_sampling_inputs(proj_, ref_, counts, ctx.offset_scale),
            lambda g, pts, att, want_img, want_sample: ragged_hip_bwd(
                g, img, img_shapes, pts, att, ctx.padding_mode, ctx.align_corners, counts,
                (want_img, want_sample, want_sample), ctx.level_cells),
            out_grad, proj, reference_points, need_img, need_proj, need_ref)
        return g_img, None, g_proj, g_ref, None, None, None, None, None


def fused_hf_box_module_core(img, img_shapes, proj, reference_points, points_per_level, offset_scale=0.5,
                             padding_mode="zeros", align_corners=False, level_shapes=None) -> torch.Tensor:
    """:func:`msda_triton_amd.functional.fused_hf_box_core`.  Routing mirrors ``fused_hf_module_core``: host tensors -> the
    composition; GPU -> the fused kernels (the C++ node, else the Python ``Function``); traced -> the composition over the
    registered ragged custom ops.  Equal counts stay on these kernels: the uniform fused kernels implement other rules."""
    counts = check_hf_box_args(img_shapes, proj, reference_points, points_per_level)
    offset_scale = float(offset_scale)
    B, Q, H, S, _ = proj.shape
    L = len(counts)
    on_gpu = img.device.type == "cuda"
    if on_gpu and img_shapes.device != img.device:
        img_shapes = img_shapes.to(img.device)  # (a handful of integers: follow `img`, as the other cores do)
    floating = img.is_floating_point() and proj.is_floating_point() and reference_points.is_floating_point()
    if on_gpu and floating and not torch.compiler.is_compiling():
        F._check_devices(img, proj, reference_points)
        same = F.dtypes_supported(img.dtype, proj.dtype) and reference_points.dtype == proj.dtype
        if F._autocast_on() or F.fused_storage_dtypes(img.dtype, proj.dtype, reference_points.dtype) or same:
            pad = F._padding_code(padding_mode)
            level_cells = F.level_cells_of(level_shapes, L, img.shape[1])
            ref = _box_ref(reference_points)
            ext = _ext.load()
            if same and ext is not None and hasattr(ext, "msda_fused_hfbox") and F.KernelTimer.active is None and \
                    not F._autocast_on() and _lib.has_fused_hfbox() and img.dim() == 4 and \
                    (img.shape[0], img.shape[2]) == (B, H) and fused_ragged_limits_ok(img.shape[3], proj.element_size(), counts):
                # the C++ autograd node: decoder-sized calls spend more host time than device time
                return ext.msda_fused_hfbox(img, F._shapes_i64(img_shapes), proj, ref, pad, bool(align_corners),
                                            level_cells, list(counts), list(F.hf_box_level_scale(counts)), offset_scale)
            return _HipFusedHfBoxCoreFunction.apply(img, img_shapes, proj, ref, padding_mode, bool(align_corners), counts,
                                                    offset_scale, level_cells)
    # host tensors, tracing (the ragged operator's registered custom ops) and everything the checks above did not take
    return _hf_box_composition(img, img_shapes, proj, reference_points, counts, offset_scale, padding_mode, align_corners,
                               level_shapes)
