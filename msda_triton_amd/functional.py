"""Functional API: the reference's operator interface over the MI355X HIP kernels.

Mirrors /root/reference/src/msda_triton/frontend.py (same names, argument meaning and errors):

  multiscale_deformable_attention          frontend.py:145-172   public entry
  hip_multiscale_deformable_attention      frontend.py:71-105    GPU path (there: triton_multiscale_…)
  native_multiscale_deformable_attention   frontend.py:15-68     host-tensor path
  msda_hip_fwd / msda_hip_bwd              kernels.py:351-379 / 556-592   launcher pair (the native seam)

Deliberate differences from the reference:
  * GPU tensors never fall back to a CPU/eager path.  The reference wraps its GPU path in
    ``try/except Exception`` (frontend.py:167-172); here a missing extension or a failed launch
    raises.  Host (CPU) tensors use the native formulation, as the reference documents
    (README.md:127 "cpu uses fallback native torch version").
  * bfloat16 runs natively on the GPU (the reference rejects it, frontend.py:84).
  * an unknown ``padding_mode`` raises ``ValueError`` instead of reaching ``grid_sample``.
"""
from __future__ import annotations

import os
from typing import Literal, Optional, Tuple

import numpy as np
import torch
from torch.amp import custom_bwd, custom_fwd
from torch.autograd.function import Function, once_differentiable

from . import _ext, _lib

_SUFFIX = {
    torch.float32: "f32",
    torch.float16: "f16",
    torch.bfloat16: "bf16",
    torch.float64: "f64",
}
VALID_DTYPES = tuple(_SUFFIX)
# mixed storage: `img` (and its gradient) in 16 bits next to fp32 sampling points / attention weights / output
_MIXED_SUFFIX = {torch.bfloat16: "f32_vbf16", torch.float16: "f32_vf16"}


def dtypes_supported(img_dtype: torch.dtype, compute_dtype: torch.dtype) -> bool:
    """One dtype for every tensor, or a 16-bit `img` with fp32 everything else (the result is then fp32)."""
    if img_dtype == compute_dtype:
        return img_dtype in _SUFFIX
    return compute_dtype == torch.float32 and img_dtype in _MIXED_SUFFIX


# (img, sampling_points, attention_weights) dtypes the kernels take, for the fast path's single lookup
_DTYPE_TRIPLES = frozenset([(t, t, t) for t in _SUFFIX] + [(t, torch.float32, torch.float32) for t in _MIXED_SUFFIX])
_SHAPE_DTYPES = frozenset((torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8))


def _suffix_for(img_dtype: torch.dtype, compute_dtype: torch.dtype) -> str:
    if not dtypes_supported(img_dtype, compute_dtype):
        raise ValueError(
            "`img`, `sampling_points` and `attention_weights` should share one dtype (or `img` be float16 / bfloat16 "
            f"next to float32 sampling inputs), but got {img_dtype} and {compute_dtype}.")
    return _SUFFIX[img_dtype] if img_dtype == compute_dtype else _MIXED_SUFFIX[img_dtype]


# the module's 16-bit storage (fused entry points only): value and projection in one 16-bit dtype, reference points fp32
_FUSED_STORAGE_SUFFIX = {torch.bfloat16: "f32_sbf16", torch.float16: "f32_sf16"}


def fused_storage_dtypes(img_dtype, proj_dtype, ref_dtype) -> bool:
    """16-bit value pyramid and projection next to fp32 reference points: what autocast's GEMMs hand the module core.
    The kernels compute in fp32 and return / differentiate in the 16-bit dtype (``msda_*_fused_f32_sbf16`` / ``_sf16``)."""
    return img_dtype == proj_dtype and proj_dtype in _FUSED_STORAGE_SUFFIX and ref_dtype == torch.float32


def _fused_suffix_for(img_dtype, proj_dtype, ref_dtype) -> str:
    if fused_storage_dtypes(img_dtype, proj_dtype, ref_dtype):
        return _FUSED_STORAGE_SUFFIX[proj_dtype]
    if ref_dtype != proj_dtype:
        raise ValueError(f"`proj` and `reference_points` should share one dtype (or `img` and `proj` be float16 / bfloat16 "
                         f"next to float32 `reference_points`), but got {proj_dtype} and {ref_dtype}.")
    return _suffix_for(img_dtype, proj_dtype)


def _padding_code(padding_mode: str) -> int:
    try:
        return _lib.PADDING_MODES[padding_mode]
    except KeyError:
        raise ValueError(f"`padding_mode` should be 'border' or 'zeros', but got {padding_mode!r}.") from None


def _dims(img: torch.Tensor, sampling_points: torch.Tensor, attention_weights: torch.Tensor, img_shapes: torch.Tensor):
    if img.dim() != 4 or sampling_points.dim() != 6 or attention_weights.dim() != 5:
        raise ValueError(
            "expected img [B,I,H,C], sampling_points [B,N,H,L,P,2], attention_weights [B,N,H,L,P]; got "
            f"{tuple(img.shape)}, {tuple(sampling_points.shape)}, {tuple(attention_weights.shape)}")
    B, I, H, D = img.shape
    B2, Q, H2, L, P, two = sampling_points.shape
    if (B2, H2, two) != (B, H, 2) or tuple(attention_weights.shape) != (B, Q, H, L, P):
        raise ValueError(
            f"inconsistent shapes: img {tuple(img.shape)}, sampling_points {tuple(sampling_points.shape)}, "
            f"attention_weights {tuple(attention_weights.shape)}")
    if tuple(img_shapes.shape) != (L, 2):
        raise ValueError(f"`img_shapes` should be [{L}, 2], but got {tuple(img_shapes.shape)}.")
    return B, I, H, D, Q, L, P


def _shapes_i64(img_shapes: torch.Tensor) -> torch.Tensor:
    if img_shapes.dtype not in (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8):
        raise ValueError(f"`img_shapes` should be an integer tensor, but got {img_shapes.dtype}.")
    if img_shapes.dtype == torch.int64 and img_shapes.is_contiguous():
        return img_shapes
    return img_shapes.to(torch.int64).contiguous()  # stays on the device: no host sync


_BWD_SUPPORTED: dict = {}  # (B, I, H, D, Q, L, P, element size) -> msda_bwd_supported


def check_backward_supported(img, sampling_points, num_queries: Optional[int] = None) -> None:
    """Raise at FORWARD time when the value pyramid needs a gradient the library cannot produce for these sizes (a plane
    of 2^22 pixels or more, or a head dimension beyond the sorted pipeline's 32-bit slot offsets, on a problem too
    large for the single-launch kernel) — not from the backward in the middle of a training step.
    ``num_queries``: ``sampling_points`` is a flat run of rows ``[rows, H, L, P, 2]`` of batch elements with that many
    queries each (the row-sharded operator)."""
    B, I, H, D = img.shape
    if num_queries is None:
        _, Q, _, L, P = sampling_points.shape[:5]
    else:
        Q, (_, _, L, P) = int(num_queries), sampling_points.shape[:4]
    key = (B, I, H, D, Q, L, P, sampling_points.element_size())
    ok = _BWD_SUPPORTED.get(key)
    if ok is None:
        ok = _BWD_SUPPORTED[key] = bool(_lib.load().msda_bwd_supported(*key))
    if not ok:
        raise ValueError(
            f"`img` requires a gradient, but grad_value is not available for this shape (I={I} pixels per plane, D={D}, "
            f"Q={Q}): the sorted pipeline addresses planes below 2^22 pixels with 4*I*D*sizeof(acc) < 2^31 bytes of "
            "partial rows.  Detach `img` or split the pyramid.")


def _check_devices(*tensors: torch.Tensor) -> torch.device:
    """All tensors must live on ONE gpu (reference: frontend.py:93-95).  Raised before any ``data_ptr()`` is handed
    to the library: a host or foreign-device pointer would otherwise fault inside the kernel."""
    devices = [t.device for t in tensors]
    if any(d.type != "cuda" for d in devices) or any(d != devices[0] for d in devices):
        raise ValueError(f"Expected all inputs to be on one gpu, but got {devices}.")
    return devices[0]


def padded_value_rows(B: int, I: int, H: int, D: int, dtype: torch.dtype, device, pad_bytes: Optional[int] = None):  # noqa: E741
    """A ``[B, I, H, D]`` tensor whose pixels' rows sit ``H * D * size + pad`` bytes apart (uninitialised): the view
    ``buf[:, :, :H * D].view(B, I, H, D)`` of a ``[B, I, H * D + pad / size]`` buffer.  The kernels read such a tensor
    in place (``value_row_stride`` of the C ABI, include/msda_hip.h).  ``pad_bytes=None``: :func:`value_row_pad`'s
    choice — one 128-byte line when the dense stride is a multiple of 256 bytes, else none."""
    es = torch.empty((), dtype=dtype).element_size()
    pad = value_row_pad(H * D * es) if pad_bytes is None else int(pad_bytes)
    if pad % es:
        raise ValueError(f"pad_bytes={pad} is not a multiple of the element size {es}")
    buf = torch.empty((B, I, H * D + pad // es), dtype=dtype, device=device)
    return buf[:, :, :H * D].view(B, I, H, D)


def value_row_pad(dense_row_bytes: int) -> int:
    """Bytes to put behind every pixel's rows of a value pyramid this package allocates itself.  The gather kernels are
    bound by the vector L1, which picks one of four tag RAMs from the low bits of a row's 128-byte line index: with the
    pixels' rows an EVEN number of lines apart (1 024 bytes: 8 heads x 32 channels x fp32; 512: the same in 16 bits) the
    rows of one head keep hitting the same tag RAMs, and that head's plane gathers up to 20 % slower (HISTORY.md 4 item 5).  One
    extra line makes the distance odd: every head cycles through all eight residues.  Measured (round 6,
    profiles/r06_row_stride_ab.txt): forward -4 ... -8 %, sample gradients -9 ... -10 % at 900 ... 5 000 queries per batch
    element; c3's bf16 forward -7.5 %; nothing at 10 000 queries, where two-plane workgroups already level it."""
    env = os.environ.get("MSDA_VALUE_ROW_PAD")  # (A/B runs and an escape hatch: bytes, 0 = never pad)
    if env is not None and env.strip().lstrip("-").isdigit():
        return max(0, int(env))
    return 128 if dense_row_bytes % 256 == 0 else 0


def _value_rows(img: torch.Tensor):
    """-> (tensor the kernels can address, its value_row_stride in bytes; 0: dense).  A ``[B, I, H, D]`` view whose
    pixels are a constant number of bytes apart with the H * D channels of a pixel contiguous (:func:`padded_value_rows`)
    is read in place; any other layout is copied dense, as the reference does (kernels.py:367-370)."""
    if img.is_contiguous():
        return img, 0
    B, I, H, D = img.shape  # noqa: E741
    st = img.stride()
    if D > 0 and H > 0 and I > 0 and st[3] == 1 and st[2] == D and st[1] >= H * D and (B == 1 or st[0] == I * st[1]) and \
            (st[1] * img.element_size()) % 16 == 0 and I * st[1] * img.element_size() < 2 ** 31:
        return img, st[1] * img.element_size()
    return img.contiguous(), 0


def _validate_value_mask(value_mask: torch.Tensor, img: torch.Tensor) -> None:
    if not torch.is_tensor(value_mask) or value_mask.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"`value_mask` should be a bool or uint8 tensor, but got "
                         f"{value_mask.dtype if torch.is_tensor(value_mask) else type(value_mask).__name__}.")
    if value_mask.dim() != 2 or img.dim() != 4 or tuple(value_mask.shape) != tuple(img.shape[:2]):
        raise ValueError(f"`value_mask` should be [{img.shape[0] if img.dim() else '?'}, {img.shape[1] if img.dim() > 1 else '?'}] "
                         f"(a flag per pixel of `img`), but got {tuple(value_mask.shape)}.")
    if value_mask.device != img.device:
        raise ValueError(f"`value_mask` should be on `img`'s device {img.device}, but got {value_mask.device}.")


def check_value_mask(value_mask: torch.Tensor, img: torch.Tensor) -> torch.Tensor:
    """``value_mask``: ``[B, I]``, bool or uint8, on ``img``'s device — non-zero = the pixel is real (transformers'
    ``attention_mask`` polarity; mmcv's ``key_padding_mask`` is the inverse).  Returns it as the kernels take it:
    contiguous uint8 (a bool mask as its uint8 view, without a copy)."""
    _validate_value_mask(value_mask, img)
    value_mask = value_mask.contiguous()
    return value_mask.view(torch.uint8) if value_mask.dtype == torch.bool else value_mask


def apply_value_mask(img: torch.Tensor, value_mask: Optional[torch.Tensor]) -> torch.Tensor:
    """``where(value_mask, img, 0)`` over heads and channels — the composition every route without masked kernels uses
    (autograd gives ``grad_img`` its zeros); ``img`` itself without a mask."""
    if value_mask is None:
        return img
    _validate_value_mask(value_mask, img)
    padding = ~value_mask if value_mask.dtype == torch.bool else value_mask == 0
    return img.masked_fill(padding[:, :, None, None], 0)


def _validate_query_mask(query_mask: torch.Tensor, per_query: torch.Tensor) -> None:
    """``per_query``: any tensor whose two leading dims are (batch, num_queries) — the sampling points, the projection."""
    if not torch.is_tensor(query_mask) or query_mask.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"`query_mask` should be a bool or uint8 tensor, but got "
                         f"{query_mask.dtype if torch.is_tensor(query_mask) else type(query_mask).__name__}.")
    if query_mask.dim() != 2 or per_query.dim() < 2 or tuple(query_mask.shape) != tuple(per_query.shape[:2]):
        raise ValueError(f"`query_mask` should be [{per_query.shape[0] if per_query.dim() else '?'}, "
                         f"{per_query.shape[1] if per_query.dim() > 1 else '?'}] (a flag per query), but got "
                         f"{tuple(query_mask.shape)}.")
    if query_mask.device != per_query.device:
        raise ValueError(f"`query_mask` should be on the queries' device {per_query.device}, but got {query_mask.device}.")


def check_query_mask(query_mask: torch.Tensor, per_query: torch.Tensor) -> torch.Tensor:
    """``query_mask``: ``[B, Q]``, bool or uint8, on the device of ``per_query`` (a ``[B, Q, ...]`` tensor) — non-zero = the
    query is real, the polarity and dtype handling of :func:`check_value_mask`.  Returns it as the kernels take it:
    contiguous uint8 (a bool mask as its uint8 view, without a copy)."""
    _validate_query_mask(query_mask, per_query)
    query_mask = query_mask.contiguous()
    return query_mask.view(torch.uint8) if query_mask.dtype == torch.bool else query_mask


def apply_query_mask(per_query: torch.Tensor, query_mask: Optional[torch.Tensor], fill: float = 0.0) -> torch.Tensor:
    """``where(query_mask, per_query, fill)`` over everything behind the two leading (batch, query) dims — the
    composition every route without query-mask kernels uses, and the definition of ``query_mask`` on host tensors:

    * the masked queries' INPUTS are sanitised: sampling points (or reference points) to ``fill=0.5``, attention weights,
      logits and offsets to 0 — whatever bits they held (NaN, Inf) are gone before anything is computed;
    * the masked rows of ``out`` are zeroed (``fill=0``).

    ``where`` routes gradients by selection, never by multiplication, so autograd gives the masked queries' inputs zero
    gradients and keeps a non-finite ``grad_out`` row of theirs out of ``grad_value``.  ``per_query`` itself without a
    mask."""
    if query_mask is None:
        return per_query
    _validate_query_mask(query_mask, per_query)
    real = query_mask if query_mask.dtype == torch.bool else query_mask != 0
    real = real.reshape(real.shape + (1,) * (per_query.dim() - 2))
    return torch.where(real, per_query, torch.full((), fill, dtype=per_query.dtype, device=per_query.device))


_ONES_MASKS: dict = {}  # (B, I, device) -> all-ones uint8 [B, I]: the value mask of a call that has a query mask only


def _ones_value_mask(img: torch.Tensor) -> torch.Tensor:
    key = (img.shape[0], img.shape[1], img.device)
    ones = _ONES_MASKS.get(key)
    if ones is None:
        ones = _ONES_MASKS[key] = torch.ones(key[:2], dtype=torch.uint8, device=img.device)
    return ones


def _mask_args(name: str, value_mask, query_mask, img, per_query):
    """Entry-point family and leading mask pointers of a launcher call: ``name`` itself without a mask, its ``_masked``
    twin with a value mask, ``_qmasked`` with a query mask (both masks required there: all ones for a missing value mask).
    The tensors are returned too — the caller keeps them alive across the launch."""
    if query_mask is not None:
        value_mask = check_value_mask(value_mask, img) if value_mask is not None else _ones_value_mask(img)
        query_mask = check_query_mask(query_mask, per_query)
        return name + "_qmasked", (value_mask.data_ptr(), query_mask.data_ptr()), (value_mask, query_mask)
    if value_mask is not None:
        value_mask = check_value_mask(value_mask, img)
        return name + "_masked", (value_mask.data_ptr(),), (value_mask,)
    return name, (), ()


class MaskedCallDeclined(Exception):
    """Raised by the forward of a masked module ``Function`` when the library declines the call (``MSDA_ERR_UNSUPPORTED``;
    nothing was launched): :func:`fused_module_core` / ``fused_ragged_module_core`` catch it and compose the masks."""


def _mask_bytes(mask: torch.Tensor) -> torch.Tensor:
    """a validated mask as the kernels take it: contiguous uint8 (bool is viewed, not copied)"""
    mask = mask.contiguous()
    return mask.view(torch.uint8) if mask.dtype == torch.bool else mask


def _module_mask_args(name: str, value_mask, query_mask, img, per_query, checked: bool = False):
    """:func:`_mask_args` for the module's own fused pairs (``msda_*_fused_masked_<suffix>``,
    ``msda_*_fused_ragged_masked_<suffix>``): one ``_masked`` family takes both pointers behind ``value``; a call with a
    query mask only passes the cached all-ones value mask, a call with a value mask only a NULL query mask ("every query is
    real": it keeps what a query mask costs the kernels).  ``checked``: the masks are what :func:`check_value_mask` /
    :func:`check_query_mask` return already (the ``Function``s: the cores validated and converted them once)."""
    if value_mask is None and query_mask is None:
        return name, (), ()
    if value_mask is None:
        value_mask = _ones_value_mask(img)
    elif not checked:
        value_mask = check_value_mask(value_mask, img)
    if query_mask is not None and not checked:
        query_mask = check_query_mask(query_mask, per_query)
    return (name + "_masked", (value_mask.data_ptr(), None if query_mask is None else query_mask.data_ptr()),
            (value_mask, query_mask))


def fused_lp_limit(D: int, elem_size: int) -> int:
    """``msda_fused_lp_limit``: the most samples per (b, q, h) unit the fused kernels take at this head dimension and
    arithmetic element size (cached)."""
    key = (int(D), int(elem_size))
    limit = _FUSED_LP_LIMIT.get(key)
    if limit is None:
        limit = _FUSED_LP_LIMIT[key] = int(_lib.load().msda_fused_lp_limit(*key))
    return limit


def module_masks_in_kernels(img, proj, reference_points, samples: int, levels: Optional[int] = None) -> bool:
    """Do the module's masked fused kernels take this call — GPU tensors of the dtypes the fused kernels serve, outside a
    trace, a library that has the symbols, and a shape the kernels do not decline (all ``samples`` of a unit in one LDS
    pass; ``levels``, given for per-level counts, at most 8)?  Everything else composes :func:`apply_value_mask` /
    :func:`apply_query_mask` with the unmasked route."""
    if img.device.type != "cuda" or torch.compiler.is_compiling() or img.dim() != 4:
        return False
    if not (img.is_floating_point() and proj.is_floating_point() and reference_points.is_floating_point()):
        return False
    autocast = _autocast_on()
    storage = fused_storage_dtypes(img.dtype, proj.dtype, reference_points.dtype)
    same = dtypes_supported(img.dtype, proj.dtype) and reference_points.dtype == proj.dtype
    if not (autocast or storage or same) or not _lib.has_module_masks():
        return False
    if levels is not None and levels > 8:
        return False
    return samples <= fused_lp_limit(img.shape[3], 4 if (autocast or storage) else proj.element_size())


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_FUSED_LP_LIMIT: dict = {}  # (D, element size) -> msda_fused_lp_limit
_WS_BYTES: dict = {}  # (B, I, H, D, Q, L, P, elem, option epoch) -> msda_bwd_workspace_bytes


def _stream_ptr(device: torch.device) -> int:
    """hipStream_t of PyTorch's current stream on ``device`` (the raw getter is ~10x cheaper than building a
    torch.cuda.Stream object; same value)."""
    if _raw_stream is not None and device.index is not None:
        return _raw_stream(device.index)
    return torch.cuda.current_stream(device).cuda_stream


def _autocast_on() -> bool:
    try:
        return torch.is_autocast_enabled("cuda")
    except TypeError:  # older signature
        return torch.is_autocast_enabled()


class _OnDevice:
    """``with torch.cuda.device(d)`` only when ``d`` is not already the current device (the context manager costs
    several microseconds per call, which matters for Grounding-DINO-sized problems)."""

    __slots__ = ("ctx",)

    def __init__(self, device: torch.device):
        self.ctx = None if (device.index is None or device.index == torch.cuda.current_device()) \
            else torch.cuda.device(device)

    def __enter__(self):
        if self.ctx is not None:
            self.ctx.__enter__()

    def __exit__(self, *exc):
        if self.ctx is not None:
            return self.ctx.__exit__(*exc)
        return False


class KernelTimer:
    """Per-kernel HIP-event timing for measurements (``bench.py``).

    While active (``with KernelTimer() as kt:``) every launcher brackets each kernel launch with
    events recorded on the stream the kernel is launched on, and the backward is issued as two C-ABI
    calls so its two kernels are timed separately.  ``kt.summary()`` (after a device sync) gives
    ``{kernel: (launches, mean_ms)}``.  Off by default: zero cost on the normal path.
    """

    active: Optional["KernelTimer"] = None

    def __init__(self):
        self.records = []  # (name, start_event, end_event)

    def __enter__(self):
        KernelTimer.active = self
        return self

    def __exit__(self, *exc):
        KernelTimer.active = None
        return False

    def launch(self, name: str, device: torch.device, call):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        stream = torch.cuda.current_stream(device)
        start.record(stream)
        rc = call()
        end.record(stream)
        self.records.append((name, start, end))
        return rc

    def summary(self):
        acc = {}
        for name, start, end in self.records:
            n, total = acc.get(name, (0, 0.0))
            acc[name] = (n + 1, total + start.elapsed_time(end))
        return {k: (n, total / n) for k, (n, total) in acc.items()}


# ------------------------------------------------------------------------------------------
# the steps every fused launcher shares (here, in .ragged and in .discrete): a launcher keeps its own shape check, its
# output shapes and its argument tuple
# ------------------------------------------------------------------------------------------
def _fused_prepare(img, img_shapes, proj, reference_points, padding_mode=None, out_grad=None, logits=None):
    """Device check, suffix, and every tensor as the kernels take it -> ``(suffix, padding code | None, img,
    value_row_stride, shapes, proj, reference_points, out_grad | None)``, and ``logits`` behind those for the split pair.
    ``out_grad`` (a backward): contiguous, in the projection's dtype — one rule for every family."""
    _check_devices(*[t for t in (img, img_shapes, proj, logits, reference_points, out_grad) if t is not None])
    pad = None if padding_mode is None else _padding_code(padding_mode)
    cdt = proj.dtype
    suf = _fused_suffix_for(img.dtype, cdt, reference_points.dtype)
    (img, vrow), proj, reference_points = _value_rows(img), proj.contiguous(), reference_points.contiguous()
    if out_grad is not None:
        out_grad = out_grad.contiguous()
        if out_grad.dtype != cdt:
            out_grad = out_grad.to(cdt)
    res = (suf, pad, img, vrow, _shapes_i64(img_shapes), proj, reference_points, out_grad)
    return res if logits is None else res + (logits.contiguous(),)


def _fused_workspace(need_img: bool, query, dims, suf: str, proj, img, level_cells: int):
    """-> (workspace, its bytes) of a fused backward: ``query`` is the family's size query, ``dims`` its leading arguments
    (B, I, H, D, Q, L and P or the counts array).  (None, 0) for a frozen value pyramid, which needs none at all (ADVICE
    r04).  The arithmetic element size is 4 under a storage suffix (fp32 arithmetic on 16-bit tensors), else ``proj``'s."""
    if not need_img:
        return None, 0
    ws_bytes = int(query(*dims, 4 if suf in _lib.FUSED_STORAGE_SUFFIXES else proj.element_size(), img.element_size(),
                         level_cells, 0))
    return torch.empty(ws_bytes, dtype=torch.uint8, device=img.device), ws_bytes


def _fused_run(group: str, symbol: str, device: torch.device, fn, args) -> bool:
    """Issue ``fn(*args, stream)`` on ``device``'s current stream, under the per-kernel timer's ``group`` when one is
    active.  False when the library declines the call (nothing was launched); any other failure raises."""
    with _OnDevice(device):
        timer = KernelTimer.active
        if timer is None:
            rc = fn(*args, _stream_ptr(device))
        else:
            rc = timer.launch(group, device, lambda: fn(*args, _stream_ptr(device)))
    if rc == -5:  # MSDA_ERR_UNSUPPORTED
        return False
    _lib.check(rc, symbol)
    return True


def _parked(ws, reference_points, B, Q, H, S, weights: bool):
    """Copies of what a fused backward left at the head of its workspace for the grad_value passes: the sampling points
    ``[B, Q, H, S, 2]`` and, behind them (``weights``: the discrete pairs), the softmaxed weights ``[B, Q, H, S]`` — in the
    arithmetic dtype, float32 for the 16-bit operators (msda_common.hpp, ParkType)."""
    pdt = torch.float32 if reference_points.element_size() == 2 else reference_points.dtype
    n = B * Q * H * S * pdt.itemsize
    points = ws[:2 * n].view(pdt).view(B, Q, H, S, 2).clone()
    return (points, ws[2 * n:3 * n].view(pdt).view(B, Q, H, S).clone()) if weights else (points,)


def _composed_backward(prologue, op_bwd, out_grad, proj, reference_points, need_img, need_proj, need_ref):
    """The backward of a fused core the library declined: the prologue in PyTorch around the unfused operator's backward
    -> ``(g_img, g_proj, g_ref)``.  ``prologue(proj, reference_points) -> (points, weights)`` in the reference points'
    dtype; ``op_bwd(out_grad, points, weights, need_img, need_sample)`` the operator's backward — ``(g_img, g_points,
    g_weights)``, or ``(g_img, g_weights)`` from the discrete operator, whose points take no gradient."""
    with torch.enable_grad():
        proj_ = proj.detach().to(reference_points.dtype).requires_grad_(need_proj)
        ref_ = reference_points.detach().requires_grad_(need_ref)
        pts, att = prologue(proj_, ref_)
    need_sample = need_proj or need_ref
    g_img, *g_sample = op_bwd(out_grad.to(pts.dtype), pts.detach(), att.detach(), need_img, need_sample)
    g_proj = g_ref = None
    if need_sample:
        wrt = [t for t, n in ((proj_, need_proj), (ref_, need_ref)) if n]
        grads = list(torch.autograd.grad([pts, att][-len(g_sample):], wrt, g_sample, allow_unused=True))
        if need_proj:
            g_proj = grads.pop(0).to(proj.dtype)
        if need_ref:
            g_ref = grads.pop(0)
    return g_img, g_proj, g_ref


# ------------------------------------------------------------------------------------------
# launcher pair — the native seam (reference: kernels.py:351-379, 556-592)
# ------------------------------------------------------------------------------------------
def msda_hip_fwd(img, img_shapes, sampling_points, attention_weights, padding_mode, align_corners,
                 out: Optional[torch.Tensor] = None, value_mask: Optional[torch.Tensor] = None,
                 query_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Allocate ``out`` (or write into the caller's contiguous ``[B, Q, H, D]`` buffer, e.g. a slice of a gather
    buffer) and enqueue the forward kernel on the current stream (no host sync).  ``value_mask``: the value-mask twin
    (``msda_fwd_masked_<dtype>``; :func:`check_value_mask`).  ``query_mask``: ``msda_fwd_qmasked_<dtype>``
    (:func:`check_query_mask`; without a value mask the call passes all ones)."""
    B, I, H, D, Q, L, P = _dims(img, sampling_points, attention_weights, img_shapes)
    _check_devices(img, img_shapes, sampling_points, attention_weights)
    pad = _padding_code(padding_mode)
    cdt = sampling_points.dtype  # dtype of everything but `img` (the same, or fp32 next to a 16-bit `img`)
    if attention_weights.dtype != cdt:
        raise ValueError(f"`sampling_points` and `attention_weights` should share one dtype, but got {cdt} and "
                         f"{attention_weights.dtype}.")
    suf = _suffix_for(img.dtype, cdt)
    (img, vrow), sampling_points, attention_weights = _value_rows(img), sampling_points.contiguous(), attention_weights.contiguous()
    shapes = _shapes_i64(img_shapes)
    if out is None:
        out = torch.empty((B, Q, H, D), dtype=cdt, device=img.device)
    elif tuple(out.shape) != (B, Q, H, D) or out.dtype != cdt or out.device != img.device or not out.is_contiguous():
        raise ValueError(f"`out` should be a contiguous {(B, Q, H, D)} {cdt} tensor on {img.device}, but got "
                         f"{tuple(out.shape)} {out.dtype} on {out.device} (contiguous: {out.is_contiguous()}).")
    lib = _lib.load()
    name, mask_arg, _masks = _mask_args("msda_fwd", value_mask, query_mask, img, sampling_points)
    fn = getattr(lib, f"{name}_{suf}")

    def call():
        return fn(img.data_ptr(), *mask_arg, shapes.data_ptr(), sampling_points.data_ptr(), attention_weights.data_ptr(),
                  out.data_ptr(), B, I, H, D, Q, L, P, pad, int(bool(align_corners)), vrow, _stream_ptr(img.device))

    with _OnDevice(img.device):
        timer = KernelTimer.active
        rc = timer.launch(name, img.device, call) if timer else call()
    _lib.check(rc, f"{name}_{suf}")
    return out


def level_cells_of(level_shapes, num_levels: Optional[int] = None, num_pixels: Optional[int] = None) -> int:
    """``level_shapes``: the pyramid's (height, width) pairs AS HOST NUMBERS (e.g. Hugging Face's
    ``spatial_shapes_list``), or None.  Returns the bound ``msda_bwd_<dtype>`` takes as ``max_level_cells`` — the bilinear cells of the
    largest level, (h + 1) * (w + 1) — or 0 for "unknown".  With it the backward can use its single-launch grad_value
    kernel on decoder-sized calls over real-image pyramids (include/msda_hip.h); it must describe the same pyramid as
    the ``img_shapes`` tensor (a level larger than promised gets NaN gradients)."""
    if level_shapes is None:
        return 0
    if isinstance(level_shapes, torch.Tensor):
        if level_shapes.device.type != "cpu":
            raise ValueError("`level_shapes` should be host numbers (a device tensor would need a synchronisation); "
                             "pass e.g. `spatial_shapes_list`")
        level_shapes = level_shapes.tolist()
    # (plain loops: torch.compile traces this function with the list as a constant)
    levels, pixels, cells = 0, 0, 0
    for h, w in level_shapes:
        h, w = int(h), int(w)
        levels += 1
        pixels += h * w
        cells = max(cells, (h + 1) * (w + 1))
    # what can be checked without reading `img_shapes` back from the device: the level count and the pixel total of
    # the call it is supposed to describe (a list describing another pyramid would give NaN grad_value rows)
    if num_levels is not None and levels != num_levels:
        raise ValueError(f"`level_shapes` has {levels} levels, `img_shapes` {num_levels}")
    if num_pixels is not None and pixels != num_pixels:
        raise ValueError(f"`level_shapes` describes {pixels} pixels, `img` has {num_pixels}")
    return cells


def msda_hip_bwd(out_grad, img, img_shapes, sampling_points, attention_weights, padding_mode, align_corners,
                 needs: Tuple[bool, bool, bool] = (True, True, True),
                 out: Optional[Tuple[Optional[torch.Tensor], Optional[torch.Tensor], Optional[torch.Tensor]]] = None,
                 level_cells: int = 0, value_mask: Optional[torch.Tensor] = None,
                 query_mask: Optional[torch.Tensor] = None,
                 ) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor], Optional[torch.Tensor]]:
    """Returns ``(img_grad, sampling_points_grad, attention_weights_grad)``; entries not in ``needs`` are None.
    ``level_cells``: see :func:`level_cells_of` (0: unknown).  ``value_mask``: the value-mask twin
    (``msda_bwd_masked_<dtype>``): padding pixels count as zeros and their ``img_grad`` rows are zeros.  ``query_mask``:
    ``msda_bwd_qmasked_<dtype>`` — the masked queries' gradient rows are zeros and nothing of theirs reaches ``img_grad``.

    Gradients are allocated contiguous (the reference's ``zeros_like(...).contiguous()`` would write
    into a temporary for permuted inputs, kernels.py:570-578) and are fully written by the kernels,
    so they are not pre-zeroed.  ``out``: contiguous buffers of the gradients' shapes to write into instead (e.g.
    slices of a shard's gradient tensors); an entry that is None is allocated here.
    """
    B, I, H, D, Q, L, P = _dims(img, sampling_points, attention_weights, img_shapes)
    _check_devices(img, img_shapes, sampling_points, attention_weights, out_grad)
    bwd_name, mask_arg, _masks = _mask_args("msda_bwd", value_mask, query_mask, img, sampling_points)
    pad = _padding_code(padding_mode)
    cdt = sampling_points.dtype
    if attention_weights.dtype != cdt:
        raise ValueError(f"`sampling_points` and `attention_weights` should share one dtype, but got {cdt} and "
                         f"{attention_weights.dtype}.")
    suf = _suffix_for(img.dtype, cdt)
    (img, vrow), sampling_points, attention_weights = _value_rows(img), sampling_points.contiguous(), attention_weights.contiguous()
    out_grad = out_grad.contiguous()
    if out_grad.dtype != cdt:
        out_grad = out_grad.to(cdt)
    shapes = _shapes_i64(img_shapes)
    want_value = bool(needs[0])
    want_sample = bool(needs[1] or needs[2])

    def buf(i, shape, wanted, dtype):
        if not wanted:
            return None
        t = out[i] if out is not None else None
        if t is None:
            return torch.empty(shape, dtype=dtype, device=img.device)
        if tuple(t.shape) != tuple(shape) or t.dtype != dtype or t.device != img.device or not t.is_contiguous():
            raise ValueError(f"`out[{i}]` should be a contiguous {tuple(shape)} {dtype} tensor on {img.device}")
        return t

    g_img = buf(0, (B, I, H, D), want_value, img.dtype)
    g_pts = buf(1, (B, Q, H, L, P, 2), want_sample, cdt)
    g_att = buf(2, (B, Q, H, L, P), want_sample, cdt)
    if want_value or want_sample:
        lib = _lib.load()
        fn = getattr(lib, f"{bwd_name}_{suf}")  # (the level-size bound travels as an argument: include/msda_hip.h)
        ws, ws_bytes = None, 0
        level_cells = int(level_cells)
        if want_value:  # scratch: the inverted index of grad_value (grad_loc / grad_attn never need any)
            # all three gradients in ONE call: the sorted records may use the gradient buffers themselves (smaller
            # workspace); the per-kernel timer issues the halves as two calls and needs the full size
            # (the library's own conditions: 16-byte aligned gradient buffers, no forced side-stream fork)
            flags = _lib.WS_RECORDS_IN_GRADS if (want_sample and KernelTimer.active is None
                                                 and g_pts.data_ptr() % 16 == 0 and g_att.data_ptr() % 16 == 0
                                                 and g_img.data_ptr() % 16 == 0
                                                 and _lib.get_option("overlap") != 1) else 0
            key = (B, I, H, D, Q, L, P, sampling_points.element_size(), img.element_size(), _lib.OPTION_EPOCH, level_cells,
                   flags)
            ws_bytes = _WS_BYTES.get(key)
            if ws_bytes is None:
                ws_bytes = _WS_BYTES[key] = int(lib.msda_bwd_workspace_bytes(*key[:9], level_cells, flags))
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=img.device)

        def call(value_part: bool, sample_part: bool):
            return fn(out_grad.data_ptr(), img.data_ptr(), *mask_arg, shapes.data_ptr(), sampling_points.data_ptr(),
                      attention_weights.data_ptr(),
                      g_img.data_ptr() if value_part else None,
                      g_pts.data_ptr() if sample_part else None,
                      g_att.data_ptr() if sample_part else None,
                      B, I, H, D, Q, L, P, pad, int(bool(align_corners)), level_cells, vrow,
                      ws.data_ptr() if ws is not None else None, ws_bytes,
                      _stream_ptr(img.device))

        with _OnDevice(img.device):
            timer = KernelTimer.active
            if timer is None:
                rc = call(want_value, want_sample)
            else:  # one C-ABI call per kernel so each gets its own event pair
                rc = 0
                if want_sample:
                    rc = timer.launch(f"{bwd_name}_sample", img.device, lambda: call(False, True))
                if rc == 0 and want_value:
                    rc = timer.launch(f"{bwd_name}_value", img.device, lambda: call(True, False))
        _lib.check(rc, f"{bwd_name}_{suf}")
    return g_img, (g_pts if needs[1] else None), (g_att if needs[2] else None)


# ------------------------------------------------------------------------------------------
# autograd boundary (reference: _TritonMultiscaleDeformableAttentionFunction, frontend.py:108-142)
# ------------------------------------------------------------------------------------------
class _HipMultiscaleDeformableAttentionFunction(Function):

    @staticmethod
    @custom_fwd(device_type="cuda", cast_inputs=torch.float32)  # under autocast the op runs in fp32 (frontend.py:111)
    def forward(ctx, img, img_shapes, sampling_points, attention_weights, padding_mode, align_corners, level_cells=0,
                value_mask=None, query_mask=None):
        if ctx.needs_input_grad[0]:
            check_backward_supported(img, sampling_points)
        ctx.save_for_backward(img, img_shapes, sampling_points, attention_weights)
        ctx.padding_mode = padding_mode
        ctx.align_corners = align_corners
        ctx.level_cells = int(level_cells)
        ctx.value_mask = value_mask  # (uint8 [B, I] or None; takes no gradient)
        ctx.query_mask = query_mask  # (uint8 [B, Q] or None; likewise)
        return msda_hip_fwd(img, img_shapes, sampling_points, attention_weights, padding_mode, align_corners,
                            value_mask=value_mask, query_mask=query_mask)

    @staticmethod
    @once_differentiable
    @custom_bwd(device_type="cuda")
    def backward(ctx, out_grad):
        img, img_shapes, sampling_points, attention_weights = ctx.saved_tensors
        needs = (ctx.needs_input_grad[0], ctx.needs_input_grad[2], ctx.needs_input_grad[3])
        g_img, g_pts, g_att = msda_hip_bwd(
            out_grad, img, img_shapes, sampling_points, attention_weights,
            ctx.padding_mode, ctx.align_corners, needs, level_cells=ctx.level_cells, value_mask=ctx.value_mask,
            query_mask=ctx.query_mask)
        return g_img, None, g_pts, g_att, None, None, None, None, None


def hip_multiscale_deformable_attention(
    img: torch.Tensor,
    img_shapes: torch.Tensor,
    sampling_points: torch.Tensor,
    attention_weights: torch.Tensor,
    padding_mode: Literal["border", "zeros"],
    align_corners: bool,
    level_shapes=None,
    points_per_level=None,
    value_mask=None,
    query_mask=None,
) -> torch.Tensor:
    """GPU path.  Same contract as the reference's ``triton_multiscale_deformable_attention``
    (frontend.py:71-105): ``ValueError`` on unsupported dtype or non-GPU inputs.  ``level_shapes`` (an addition): the
    pyramid's (h, w) pairs as host numbers, see :func:`level_cells_of`.  ``points_per_level``, ``value_mask``,
    ``query_mask``: see :func:`multiscale_deformable_attention`."""
    if query_mask is not None:
        if img.device.type != "cuda":
            raise ValueError(f"hip_multiscale_deformable_attention needs GPU tensors, but `img` is on {img.device}.")
        _validate_query_mask(query_mask, sampling_points)
        # the query-mask entry points serve the uniform call outside a trace; everything else composes apply_query_mask
        # with its route
        if points_per_level is not None or torch.compiler.is_compiling() or not _lib.has_query_mask():
            out = hip_multiscale_deformable_attention(
                img, img_shapes, apply_query_mask(sampling_points, query_mask, 0.5),
                apply_query_mask(attention_weights, query_mask, 0.0), padding_mode, align_corners, level_shapes,
                points_per_level, value_mask)
            return apply_query_mask(out, query_mask, 0.0)
        if value_mask is None:  # (both masks travel to the kernels: a cached all-ones byte per pixel)
            value_mask = _ones_value_mask(img)
    if value_mask is not None:
        if img.device.type != "cuda":
            raise ValueError(f"hip_multiscale_deformable_attention needs GPU tensors, but `img` is on {img.device}.")
        _validate_value_mask(value_mask, img)
        # the value-mask kernels serve the uniform call outside a trace; everything else composes masked_fill with its route
        if points_per_level is not None or torch.compiler.is_compiling() or not _lib.has_value_mask():
            return hip_multiscale_deformable_attention(apply_value_mask(img, value_mask), img_shapes, sampling_points,
                                                       attention_weights, padding_mode, align_corners, level_shapes,
                                                       points_per_level)
        for name, t in (("img", img), ("sampling_points", sampling_points), ("attention_weights", attention_weights)):
            if t.dtype not in VALID_DTYPES:
                raise ValueError(f"Dtype of `{name}` should be in {list(VALID_DTYPES)}, but got {t.dtype}.")
        if sampling_points.dtype != attention_weights.dtype or not dtypes_supported(img.dtype, sampling_points.dtype):
            raise ValueError(
                "`img`, `sampling_points` and `attention_weights` should share one dtype (or `img` be float16 / bfloat16 "
                f"next to float32 sampling inputs), but got {img.dtype}, {sampling_points.dtype}, {attention_weights.dtype}.")
        _check_devices(img, img_shapes, sampling_points, attention_weights)
        _padding_code(padding_mode)
        # (the Python Function: the C++ autograd node takes no mask)
        return _HipMultiscaleDeformableAttentionFunction.apply(
            img, img_shapes, sampling_points, attention_weights, padding_mode, bool(align_corners),
            level_cells_of(level_shapes, img_shapes.shape[0], img.shape[1]), check_value_mask(value_mask, img),
            None if query_mask is None else check_query_mask(query_mask, sampling_points))
    if points_per_level is not None:
        if img.device.type != "cuda":
            raise ValueError(f"hip_multiscale_deformable_attention needs GPU tensors, but `img` is on {img.device}.")
        from .ragged import ragged_multiscale_deformable_attention
        return ragged_multiscale_deformable_attention(img, img_shapes, sampling_points, attention_weights, padding_mode,
                                                      align_corners, points_per_level, level_shapes)
    # Fast path (the small decoder / README shapes spend more host time than device time per call): every check below
    # as one conjunction; whatever fails it — or needs the Python Function — takes the checks that carry the messages.
    dev, dt, shp, ish = img.device, sampling_points.dtype, sampling_points.shape, img.shape
    if dev.type == "cuda" and not torch.compiler.is_compiling() and (ext := _ext.load()) is not None and \
            KernelTimer.active is None and \
            (img.dtype, dt, attention_weights.dtype) in _DTYPE_TRIPLES and padding_mode in _lib.PADDING_MODES and \
            img_shapes.device == dev and sampling_points.device == dev and attention_weights.device == dev and \
            len(ish) == 4 and len(shp) == 6 and shp[0] == ish[0] and shp[2] == ish[2] and shp[5] == 2 and \
            attention_weights.shape == shp[:5] and img_shapes.shape == (shp[3], 2) and \
            img_shapes.dtype in _SHAPE_DTYPES and not _autocast_on():
        if img.requires_grad and torch.is_grad_enabled():
            check_backward_supported(img, sampling_points)
        return ext.msda(img, img_shapes, sampling_points, attention_weights, _lib.PADDING_MODES[padding_mode],
                        bool(align_corners), level_cells_of(level_shapes, shp[3], ish[1]) if level_shapes is not None else 0)
    for name, t in (("img", img), ("sampling_points", sampling_points), ("attention_weights", attention_weights)):
        if t.dtype not in VALID_DTYPES:
            raise ValueError(f"Dtype of `{name}` should be in {list(VALID_DTYPES)}, but got {t.dtype}.")
    if sampling_points.dtype != attention_weights.dtype or not dtypes_supported(img.dtype, sampling_points.dtype):
        raise ValueError(
            "`img`, `sampling_points` and `attention_weights` should share one dtype (or `img` be float16 / bfloat16 "
            f"next to float32 sampling inputs), but got {img.dtype}, {sampling_points.dtype}, {attention_weights.dtype}.")
    _check_devices(img, img_shapes, sampling_points, attention_weights)
    _padding_code(padding_mode)
    if torch.compiler.is_compiling():  # traced by torch.compile / export: use the registered custom ops
        from .compile_op import compiled_multiscale_deformable_attention
        return compiled_multiscale_deformable_attention(
            img, img_shapes, sampling_points, attention_weights, padding_mode, align_corners,
            level_cells_of(level_shapes, img_shapes.shape[0], img.shape[1]))
    # Optional C++ autograd glue over the same C ABI (csrc/msda_torch_ext.cpp): same kernels, a fraction of the host
    # time per call.  The Python Function below serves autocast (fp32 casting), per-kernel timing and every
    # installation where the binding was not built.
    ext = _ext.load()
    if ext is not None and KernelTimer.active is None and not _autocast_on():
        _dims(img, sampling_points, attention_weights, img_shapes)
        _shapes_i64(img_shapes)
        if img.requires_grad and torch.is_grad_enabled():
            check_backward_supported(img, sampling_points)
        return ext.msda(img, img_shapes, sampling_points, attention_weights, _padding_code(padding_mode),
                        bool(align_corners), level_cells_of(level_shapes, img_shapes.shape[0], img.shape[1]))
    return _HipMultiscaleDeformableAttentionFunction.apply(
        img, img_shapes, sampling_points, attention_weights, padding_mode, bool(align_corners),
        level_cells_of(level_shapes, img_shapes.shape[0], img.shape[1]))


# ------------------------------------------------------------------------------------------
# module core with the prologue fused into the kernel (reference frontend.py:253-289)
# ------------------------------------------------------------------------------------------
def module_sampling_inputs(proj: torch.Tensor, img_shapes: torch.Tensor, reference_points: torch.Tensor):
    """The reference module's prologue in plain PyTorch: raw projection [B,N,H,L,P,3] ->
    (sampling_points [B,N,H,L,P,2], attention_weights [B,N,H,L,P])  (frontend.py:253-284)."""
    B, N, H, L, P, _ = proj.shape
    offsets, logits = proj[..., :2], proj[..., 2]
    attention_weights = logits.reshape(B, N, H, L * P).softmax(dim=-1).reshape(B, N, H, L, P)
    ref = reference_points[:, :, None, None, None, :]
    coords = reference_points.shape[-1]
    if coords == 2:
        # NB: the reference divides the (x, y) offsets by img_shapes in its stored (h, w) order
        # (frontend.py:275); reproduced for parity — it only matters for non-square levels.
        sampling_points = ref + offsets / img_shapes[:, None, :]
    elif coords == 4:
        sampling_points = ref[..., :2] + offsets * ref[..., 2:] / (2 * P)
    else:
        raise ValueError(f"`reference_points` should have the last dim either 2 or 4, but got {coords}.")
    return sampling_points, attention_weights


def msda_hip_fwd_fused(img, img_shapes, proj, reference_points, padding_mode, align_corners,
                       levelref: bool = False, value_mask: Optional[torch.Tensor] = None,
                       query_mask: Optional[torch.Tensor] = None, masks_checked: bool = False) -> Optional[torch.Tensor]:
    """Forward with softmax + sampling-point math done in the kernel prologue.  Returns None when the
    library declines (L*P too large for one pass): the caller then takes the unfused route.  ``levelref``: the
    reference points are per level, ``[B, Q, L, ref_dim]``, and the points follow transformers' rule
    (:func:`hf_module_sampling_inputs`; ``msda_fwd_fused_levelref_<dtype>``).  ``value_mask`` / ``query_mask``: with
    ``levelref`` the twins ``msda_fwd_fused_levelref_masked_<dtype>`` / ``..._qmasked_<dtype>``; without it the module's own
    masked pair ``msda_fwd_fused_masked_<dtype>``, which takes both pointers (:func:`_module_mask_args`)."""
    B, I, H, D = img.shape
    B2, Q, H2, L, P, three = proj.shape
    if (B2, H2, three) != (B, H, 3) or tuple(reference_points.shape[:2]) != (B, Q) or \
            reference_points.dim() != (4 if levelref else 3) or (levelref and reference_points.shape[2] != L):
        raise ValueError(f"inconsistent shapes: img {tuple(img.shape)}, proj {tuple(proj.shape)}, "
                         f"reference_points {tuple(reference_points.shape)}")
    ref_dim = reference_points.shape[-1]
    if ref_dim not in (2, 4):
        raise ValueError(f"`reference_points` should have the last dim either 2 or 4, but got {ref_dim}.")
    if tuple(img_shapes.shape) != (L, 2):
        raise ValueError(f"`img_shapes` should be [{L}, 2], but got {tuple(img_shapes.shape)}.")
    suf, pad, img, vrow, shapes, proj, reference_points, _ = _fused_prepare(img, img_shapes, proj, reference_points,
                                                                            padding_mode)
    name = "msda_fwd_fused_levelref" if levelref else "msda_fwd_fused"
    sym, mask_arg, _masks = _mask_args(name, value_mask, query_mask, img, proj) if levelref else \
        _module_mask_args(name, value_mask, query_mask, img, proj, masks_checked)
    fn = getattr(_lib.load(), f"{sym}_{suf}", None)
    if fn is None:  # (a library built before the per-level entry points: the caller composes)
        return None
    out = torch.empty((B, Q, H, D), dtype=proj.dtype, device=img.device)
    # (the timer's group stays the pair's — "msda_fwd_fused_levelref" — with or without a mask: it names the launcher)
    ok = _fused_run(name, f"{sym}_{suf}", img.device, fn,
                    (img.data_ptr(), *mask_arg, shapes.data_ptr(), proj.data_ptr(), reference_points.data_ptr(),
                     out.data_ptr(), B, I, H, D, Q, L, P, ref_dim, pad, int(bool(align_corners)), vrow))
    return out if ok else None


def msda_hip_bwd_fused(out_grad, img, img_shapes, proj, reference_points, padding_mode, align_corners,
                       need_img: bool = True, level_cells: int = 0, need_ref: bool = True, levelref: bool = False,
                       value_mask: Optional[torch.Tensor] = None, query_mask: Optional[torch.Tensor] = None,
                       masks_checked: bool = False):
    """Backward of the module core with the prologue's chain rule done in the kernel: returns
    ``(img_grad | None, proj_grad, reference_points_grad)``, or None when the library declines (L*P too large
    for one pass; nothing was launched).  ``levelref``: as in :func:`msda_hip_fwd_fused`; the kernel's partials are
    then ``[B, Q, H, L, ref_dim]`` and the gradient ``[B, Q, L, ref_dim]``."""
    B, I, H, D = img.shape
    _, Q, _, L, P, _ = proj.shape
    ref_dim = reference_points.shape[-1]
    suf, pad, img, vrow, shapes, proj, reference_points, out_grad = _fused_prepare(img, img_shapes, proj, reference_points,
                                                                                   padding_mode, out_grad)
    lib = _lib.load()
    name = "msda_bwd_fused_levelref" if levelref else "msda_bwd_fused"
    # (the masked entry points; the workspace is the twin's)
    sym, mask_arg, _masks = _mask_args(name, value_mask, query_mask, img, proj) if levelref else \
        _module_mask_args(name, value_mask, query_mask, img, proj, masks_checked)
    fn = getattr(lib, f"{sym}_{suf}", None)  # (the timer's group stays the pair's, as in the forward)
    if fn is None:
        return None
    g_img = torch.empty((B, I, H, D), dtype=img.dtype, device=img.device) if need_img else None
    g_proj = torch.empty((B, Q, H, L, P, 3), dtype=proj.dtype, device=img.device)
    g_ref_part = torch.empty((B, Q, H, L, ref_dim) if levelref else (B, Q, H, ref_dim), dtype=reference_points.dtype,
                             device=img.device)
    level_cells = int(level_cells)  # the level-size bound (level_cells_of), an argument of the size query and the launch
    ws, ws_bytes = _fused_workspace(need_img, lib.msda_bwd_fused_workspace_bytes, (B, I, H, D, Q, L, P), suf, proj, img,
                                    level_cells)
    if not _fused_run(name, f"{sym}_{suf}", img.device, fn,
                      (out_grad.data_ptr(), img.data_ptr(), *mask_arg, shapes.data_ptr(), proj.data_ptr(),
                       reference_points.data_ptr(), g_img.data_ptr() if need_img else None, g_proj.data_ptr(),
                       g_ref_part.data_ptr(), B, I, H, D, Q, L, P, ref_dim, pad, int(bool(align_corners)), level_cells, vrow,
                       ws.data_ptr() if need_img else None, ws_bytes)):
        return None
    # (the kernel leaves per-head partials of grad_reference_points; their sum is a launch of its own — 16 us at the c2
    # shape — and reference points rarely require a gradient)
    return g_img, g_proj, (g_ref_part.sum(dim=2) if need_ref else None)


class _HipFusedModuleCoreFunction(Function):
    """value, raw projection, reference points -> attended values.  Forward and backward are one fused kernel
    (pipeline) each: the softmax / sampling-point prologue and its chain rule run inside the HIP kernels.  When the
    library declines (L*P too large for one LDS pass) the prologue is done in PyTorch around the plain operator."""

    @staticmethod
    @custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, img, img_shapes, proj, reference_points, padding_mode, align_corners, level_cells=0, value_mask=None,
                query_mask=None):
        ctx.level_cells = int(level_cells)
        # (value_mask, query_mask: uint8 [B, I] / [B, Q] as check_*_mask returns them, or None: msda_*_fused_masked_<dtype>;
        # no gradient.  A masked call the library declines is handed back to fused_module_core, which composes it)
        out = msda_hip_fwd_fused(img, img_shapes, proj, reference_points, padding_mode, align_corners,
                                 value_mask=value_mask, query_mask=query_mask, masks_checked=True)
        ctx.fused = out is not None  # the backward has the same L*P limit: do not ask twice
        if out is None and (value_mask is not None or query_mask is not None):
            raise MaskedCallDeclined()
        if out is None:
            # (16-bit storage next to fp32 reference points: the prologue in fp32, the mixed-storage operator)
            pts, att = module_sampling_inputs(proj.to(reference_points.dtype), img_shapes, reference_points)
            out = msda_hip_fwd(img, img_shapes, pts, att, padding_mode, align_corners).to(proj.dtype)
        ctx.save_for_backward(img, img_shapes, proj, reference_points, value_mask, query_mask)
        ctx.padding_mode, ctx.align_corners = padding_mode, align_corners
        return out

    @staticmethod
    @once_differentiable
    @custom_bwd(device_type="cuda")
    def backward(ctx, out_grad):
        img, img_shapes, proj, reference_points, value_mask, query_mask = ctx.saved_tensors
        need_img, _, need_proj, need_ref = ctx.needs_input_grad[:4]
        # (a masked call stays on the fused backward even when only the pyramid wants a gradient — its grad_proj is then
        # discarded: the composition below would have to sanitise the masked queries' inputs)
        masked = value_mask is not None or query_mask is not None
        if ctx.fused and (need_proj or need_ref or masked):
            res = msda_hip_bwd_fused(out_grad, img, img_shapes, proj, reference_points, ctx.padding_mode,
                                     ctx.align_corners, need_img, level_cells=ctx.level_cells, need_ref=need_ref,
                                     value_mask=value_mask, query_mask=query_mask, masks_checked=True)
            if res is not None:
                g_img, g_proj, g_ref = res
                return g_img, None, (g_proj if need_proj else None), (g_ref if need_ref else None), None, None, None, None, None
        if masked:  # (the forward ran masked; only the grad_value pipeline can decline here, and the message says why)
            raise _lib.MSDALibraryError("the masked fused backward was declined after its forward ran: "
                                        + _lib.load().msda_last_error().decode(errors="replace"))
        g_img, g_proj, g_ref = _composed_backward(
            lambda proj_, ref_: module_sampling_inputs(proj_, img_shapes, ref_),
            lambda g, pts, att, want_img, want_sample: msda_hip_bwd(
                g, img, img_shapes, pts, att, ctx.padding_mode, ctx.align_corners, (want_img, want_sample, want_sample),
                level_cells=ctx.level_cells),
            out_grad, proj, reference_points, need_img, need_proj, need_ref)
        return g_img, None, g_proj, g_ref, None, None, None, None, None


def fused_module_core(img, img_shapes, proj, reference_points, padding_mode, align_corners, level_shapes=None,
                      points_per_level=None, value_mask=None, query_mask=None, mask_in_kernels: bool = True,
                      sampling_mode: str = "bilinear", fuse_discrete: Optional[bool] = None) -> torch.Tensor:
    """``multiscale_deformable_attention(img, img_shapes, *module_sampling_inputs(proj, ...))`` — on GPU tensors
    with the prologue fused into the forward kernel; on host tensors exactly that composition.  ``level_shapes``: the
    level sizes as host numbers, optional (:func:`level_cells_of`).  ``points_per_level``: a point count per level; then
    ``proj`` is ``[B, Q, H, S, 3]`` with ``S = sum(points_per_level)``, level-major
    (:func:`msda_triton_amd.ragged.ragged_module_sampling_inputs` states the prologue).  ``value_mask``: ``[B, I]``,
    non-zero = the pixel is real — the result is that of ``where(mask, img, 0)`` whatever the padding pixels hold.
    ``query_mask``: ``[B, Q]``, non-zero = the query is real — a masked query's row of the result is zeros, its ``proj`` and
    ``reference_points`` rows get zero gradients and nothing they hold reaches any result.  On GPU tensors both go into the
    fused kernels (``msda_*_fused_masked_<dtype>``, with ``points_per_level`` ``msda_*_fused_ragged_masked_<dtype>``; a
    call with a query mask only passes a cached all-ones value mask) through the Python ``Function`` — the C++ autograd
    nodes and the compile ops take no mask.  Host tensors, traced calls, ``mask_in_kernels=False``, a library without
    those symbols, a shape beyond the fused kernels' limits (:func:`module_masks_in_kernels`) and a forward the library
    declines (``MSDA_ERR_UNSUPPORTED``) compose :func:`apply_value_mask` / :func:`apply_query_mask` with the unmasked route.
    A BACKWARD the library declines after its forward ran masked — the grad_value pipeline's own limits: 2^22 pixels per
    plane and more, option "strict" with the plane-major place pass — raises ``MSDALibraryError`` with the library's
    message; ``mask_in_kernels=False`` serves such a call.

    ``sampling_mode="discrete"``: every sample reads the one pixel :mod:`msda_triton_amd.discrete` describes
    (``padding_mode`` / ``align_corners`` must be ``"border"`` / ``False``); the reference points and the offset columns of
    ``proj`` get no gradient.  GPU tensors run ``msda_*_fused_discrete_<dtype>`` — softmax, point rule and pixel choice in
    the kernels, at most 8 levels — through a Python ``Function``; host tensors, traced calls, more levels, a library without
    the symbols and a declined forward compose ``module_sampling_inputs`` / ``ragged_module_sampling_inputs`` with the
    discrete operator.  ``fuse_discrete``: ``True`` the kernels whenever they take the call, ``False`` the composition,
    ``None`` the measured per-dtype default (``msda_triton_amd.module.DISCRETE_IN_KERNELS_DTYPES``).  Masks in this mode
    are always composed (``apply_value_mask`` / ``apply_query_mask`` around the route)."""
    if sampling_mode != "bilinear":
        from . import discrete
        if sampling_mode not in discrete.SAMPLING_MODES:
            raise ValueError(f"`sampling_mode` should be one of {list(discrete.SAMPLING_MODES)}, but got {sampling_mode!r}.")
        discrete.check_discrete_mode(padding_mode, align_corners)
        if query_mask is not None:
            out = fused_module_core(img, img_shapes, apply_query_mask(proj, query_mask, 0.0),
                                    apply_query_mask(reference_points, query_mask, 0.5), padding_mode, align_corners,
                                    level_shapes, points_per_level, value_mask, None, mask_in_kernels, sampling_mode,
                                    fuse_discrete)
            return apply_query_mask(out, query_mask, 0.0)
        return discrete.fused_module_discrete_core(apply_value_mask(img, value_mask), img_shapes, proj, reference_points,
                                                   points_per_level, level_shapes, fuse_discrete)
    if points_per_level is not None and (value_mask is not None or query_mask is not None):
        from .ragged import fused_ragged_module_core
        return fused_ragged_module_core(img, img_shapes, proj, reference_points, padding_mode, align_corners,
                                        points_per_level, level_shapes, value_mask, query_mask, mask_in_kernels)
    if value_mask is not None or query_mask is not None:
        if value_mask is not None:
            _validate_value_mask(value_mask, img)
        if query_mask is not None:
            _validate_query_mask(query_mask, proj)
        if mask_in_kernels and proj.dim() == 6 and \
                module_masks_in_kernels(img, proj, reference_points, proj.shape[3] * proj.shape[4]):
            if img_shapes.device != img.device:
                img_shapes = img_shapes.to(img.device)
            _check_devices(img, proj, reference_points)
            _padding_code(padding_mode)
            try:  # (the masks were validated above: converted once, here)
                return _HipFusedModuleCoreFunction.apply(
                    img, img_shapes, proj, reference_points, padding_mode, bool(align_corners),
                    level_cells_of(level_shapes, img_shapes.shape[0], img.shape[1]),
                    _mask_bytes(value_mask) if value_mask is not None else _ones_value_mask(img),
                    None if query_mask is None else _mask_bytes(query_mask))
            except MaskedCallDeclined:
                pass  # nothing was launched: the composition below
    if query_mask is not None:
        out = fused_module_core(img, img_shapes, apply_query_mask(proj, query_mask, 0.0),
                                apply_query_mask(reference_points, query_mask, 0.5), padding_mode, align_corners,
                                level_shapes, points_per_level, value_mask, None, mask_in_kernels)
        return apply_query_mask(out, query_mask, 0.0)
    img = apply_value_mask(img, value_mask)
    if points_per_level is not None:
        from .ragged import fused_ragged_module_core
        return fused_ragged_module_core(img, img_shapes, proj, reference_points, padding_mode, align_corners,
                                        points_per_level, level_shapes)
    level_cells = level_cells_of(level_shapes, img_shapes.shape[0], img.shape[1])
    if img.device.type == "cuda" and img_shapes.device != img.device:
        # the level table is a handful of integers: follow `img` (the reference's module accepts a host-resident
        # img_shapes next to GPU tensors through its fallback, frontend.py:170-172)
        img_shapes = img_shapes.to(img.device)
    if img.device.type == "cuda":
        _check_devices(img, proj, reference_points)
    floating = img.is_floating_point() and proj.is_floating_point() and reference_points.is_floating_point()
    if img.device.type == "cuda" and floating and _autocast_on() and not torch.compiler.is_compiling():
        # under autocast the op computes in fp32 whatever the projections' dtypes are (custom_fwd casts every floating
        # input, frontend.py:111): mixed bf16 projections / fp32 reference points still take the fused kernels
        _padding_code(padding_mode)
        return _HipFusedModuleCoreFunction.apply(img, img_shapes, proj, reference_points, padding_mode,
                                                 bool(align_corners), level_cells)
    if img.device.type == "cuda" and floating and fused_storage_dtypes(img.dtype, proj.dtype, reference_points.dtype) and \
            not torch.compiler.is_compiling():
        # 16-bit value pyramid and projection (what autocast's GEMMs produce) next to fp32 reference points: fp32
        # arithmetic, 16-bit result and gradients — no fp32 copy of either tensor (msda_*_fused_f32_sbf16 / _sf16)
        _padding_code(padding_mode)
        return _HipFusedModuleCoreFunction.apply(img, img_shapes, proj, reference_points, padding_mode,
                                                 bool(align_corners), level_cells)
    if img.device.type == "cuda" and dtypes_supported(img.dtype, proj.dtype) and \
            reference_points.dtype == proj.dtype and not torch.compiler.is_compiling():
        pad = _padding_code(padding_mode)
        ext = _ext.load()
        if ext is not None and KernelTimer.active is None and not _autocast_on():
            # C++ autograd glue (see hip_multiscale_deformable_attention); only when the fused kernels take this L*P
            B, I, H, D = img.shape
            key = (D, proj.element_size())
            limit = _FUSED_LP_LIMIT.get(key)
            if limit is None:
                limit = _FUSED_LP_LIMIT[key] = int(ext.fused_lp_limit(*key))
            if proj.dim() == 6 and proj.shape[3] * proj.shape[4] <= limit and proj.shape[-1] == 3 \
                    and reference_points.dim() == 3 and reference_points.shape[-1] in (2, 4) \
                    and tuple(proj.shape[:3]) == (B, reference_points.shape[1], H) \
                    and reference_points.shape[0] == B and tuple(img_shapes.shape) == (proj.shape[3], 2):
                _shapes_i64(img_shapes)
                return ext.msda_fused(img, img_shapes, proj, reference_points, pad, bool(align_corners), level_cells)
        return _HipFusedModuleCoreFunction.apply(img, img_shapes, proj, reference_points, padding_mode,
                                                 bool(align_corners), level_cells)
    if img.device.type == "cuda" and torch.compiler.is_compiling() and \
            ((dtypes_supported(img.dtype, proj.dtype) and reference_points.dtype == proj.dtype) or
             fused_storage_dtypes(img.dtype, proj.dtype, reference_points.dtype)):
        from . import compile_op  # traced: keep the fused kernels as one custom op per direction
        if compile_op.fused_lp_ok(img, proj, reference_points):
            return compile_op.compiled_fused_module_core(img, img_shapes, proj, reference_points, padding_mode,
                                                         align_corners, level_cells)
    pts, att = module_sampling_inputs(proj, img_shapes, reference_points)
    return multiscale_deformable_attention(img, img_shapes, pts, att, padding_mode, align_corners, level_shapes=level_shapes)


# ------------------------------------------------------------------------------------------
# the same for Hugging Face transformers' attention modules: per-level reference points, transformers' point rule
# (transformers/models/deformable_detr/modeling_deformable_detr.py, DeformableDetrMultiscaleDeformableAttention.forward;
#  Grounding-DINO and the RT-DETR family carry the same lines)
# ------------------------------------------------------------------------------------------
def hf_module_sampling_inputs(proj: torch.Tensor, img_shapes: torch.Tensor, reference_points: torch.Tensor):
    """transformers' prologue in plain PyTorch, with transformers' own operations in transformers' own order: raw
    projection ``[B, N, H, L, P, 3]`` (x offset, y offset, logit) and PER-LEVEL reference points ``[B, N, L, 2 | 4]`` ->
    (sampling_points ``[B, N, H, L, P, 2]``, attention_weights ``[B, N, H, L, P]``).  It differs from
    :func:`module_sampling_inputs` (the reference module's prologue) in the reference points' level axis, in dividing the
    (x, y) offsets by (width, height) — not by ``img_shapes`` in its stored (height, width) order — and in the order of the
    4-d rule's operations."""
    B, N, H, L, P, _ = proj.shape
    sampling_offsets, logits = proj[..., :2], proj[..., 2]
    attention_weights = torch.nn.functional.softmax(logits.reshape(B, N, H, L * P), -1).view(B, N, H, L, P)
    num_coordinates = reference_points.shape[-1]
    if reference_points.dim() != 4 or reference_points.shape[2] != L:
        raise ValueError(f"`reference_points` should be [B, N, {L}, 2 or 4] (a point per level), but got "
                         f"{tuple(reference_points.shape)}.")
    if num_coordinates == 2:
        offset_normalizer = torch.stack([img_shapes[..., 1], img_shapes[..., 0]], -1)
        sampling_locations = (
            reference_points[:, :, None, :, None, :]
            + sampling_offsets / offset_normalizer[None, None, None, :, None, :]
        )
    elif num_coordinates == 4:
        sampling_locations = (
            reference_points[:, :, None, :, None, :2]
            + sampling_offsets / P * reference_points[:, :, None, :, None, 2:] * 0.5
        )
    else:
        raise ValueError(f"`reference_points` should have the last dim either 2 or 4, but got {num_coordinates}.")
    return sampling_locations, attention_weights


def _hf_composition(img, img_shapes, proj, reference_points, padding_mode, align_corners, level_shapes):
    """transformers' prologue as PyTorch ops around the plain operator (host tensors, traced calls, whatever the fused
    kernels decline).  16-bit value / projection next to fp32 reference points: the prologue in fp32, the mixed-storage
    operator, the result back in the projection's dtype."""
    if img.device.type == "cuda" and fused_storage_dtypes(img.dtype, proj.dtype, reference_points.dtype):
        pts, att = hf_module_sampling_inputs(proj.to(reference_points.dtype), img_shapes, reference_points)
        return multiscale_deformable_attention(img, img_shapes, pts, att, padding_mode, align_corners,
                                               level_shapes=level_shapes).to(proj.dtype)
    pts, att = hf_module_sampling_inputs(proj, img_shapes, reference_points)
    return multiscale_deformable_attention(img, img_shapes, pts, att, padding_mode, align_corners, level_shapes=level_shapes)


class _HipFusedHFModuleCoreFunction(Function):
    """:class:`_HipFusedModuleCoreFunction` for per-level reference points and transformers' point rule
    (``msda_*_fused_levelref_<dtype>``).  When the library declines — L*P too large for one LDS pass, or a library built
    before these entry points — transformers' prologue runs in PyTorch around the plain operator."""

    @staticmethod
    @custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, img, img_shapes, proj, reference_points, padding_mode, align_corners, level_cells=0, value_mask=None,
                query_mask=None):
        ctx.level_cells = int(level_cells)
        ctx.value_mask = value_mask  # (uint8 [B, I] or None: the value-mask twins of both kernel families; no gradient)
        ctx.query_mask = query_mask  # (uint8 [B, Q] or None: the query-mask entry points of both families; no gradient)
        out = msda_hip_fwd_fused(img, img_shapes, proj, reference_points, padding_mode, align_corners, levelref=True,
                                 value_mask=value_mask, query_mask=query_mask)
        ctx.fused = out is not None  # the backward has the same limits: do not ask twice
        if out is None:
            # (the prologue in PyTorch sees the masked queries' inputs: sanitised first, the kernels then skip them)
            pts, att = hf_module_sampling_inputs(apply_query_mask(proj, query_mask, 0.0).to(reference_points.dtype), img_shapes,
                                                 apply_query_mask(reference_points, query_mask, 0.5))
            out = msda_hip_fwd(img, img_shapes, pts, att, padding_mode, align_corners, value_mask=value_mask,
                               query_mask=query_mask).to(proj.dtype)
        ctx.save_for_backward(img, img_shapes, proj, reference_points)
        ctx.padding_mode, ctx.align_corners = padding_mode, align_corners
        return out

    @staticmethod
    @once_differentiable
    @custom_bwd(device_type="cuda")
    def backward(ctx, out_grad):
        img, img_shapes, proj, reference_points = ctx.saved_tensors
        need_img, _, need_proj, need_ref = ctx.needs_input_grad[:4]
        if ctx.fused and (need_proj or need_ref):
            res = msda_hip_bwd_fused(out_grad, img, img_shapes, proj, reference_points, ctx.padding_mode,
                                     ctx.align_corners, need_img, level_cells=ctx.level_cells, need_ref=need_ref,
                                     levelref=True, value_mask=ctx.value_mask, query_mask=ctx.query_mask)
            if res is not None:
                g_img, g_proj, g_ref = res
                return g_img, None, (g_proj if need_proj else None), (g_ref if need_ref else None), None, None, None, None, None
        g_img, g_proj, g_ref = _composed_backward(
            # (a query mask: the chain rule runs on the sanitised inputs, so a masked query's gradients are where's zeros)
            lambda proj_, ref_: hf_module_sampling_inputs(apply_query_mask(proj_, ctx.query_mask, 0.0), img_shapes,
                                                          apply_query_mask(ref_, ctx.query_mask, 0.5)),
            lambda g, pts, att, want_img, want_sample: msda_hip_bwd(
                g, img, img_shapes, pts, att, ctx.padding_mode, ctx.align_corners, (want_img, want_sample, want_sample),
                level_cells=ctx.level_cells, value_mask=ctx.value_mask, query_mask=ctx.query_mask),
            out_grad, proj, reference_points, need_img, need_proj, need_ref)
        return g_img, None, g_proj, g_ref, None, None, None, None, None


def fused_hf_module_core(img, img_shapes, proj, reference_points, padding_mode, align_corners, level_shapes=None,
                         value_mask=None, mask_in_kernels: bool = True, query_mask=None) -> torch.Tensor:
    """``multiscale_deformable_attention(img, img_shapes, *hf_module_sampling_inputs(proj, ...))``: the core of a Hugging
    Face attention module between its projections — value pyramid ``[B, I, H, D]``, raw projection ``[B, Q, H, L, P, 3]``,
    per-level reference points ``[B, Q, L, 2 | 4]``.  On GPU tensors the prologue and its chain rule run inside the
    gather kernels (``msda_*_fused_levelref_<dtype>``); on host tensors, while traced by ``torch.compile`` (over the
    registered custom ops) and where the library declines it is exactly that composition.  ``level_shapes``: the level
    sizes as host numbers, optional (:func:`level_cells_of`).  ``value_mask``: ``[B, I]`` bool / uint8, non-zero = the pixel
    is real (transformers' ``attention_mask``; :func:`check_value_mask`) — the result is that of ``where(mask, img, 0)``
    whatever the padding pixels hold.  On GPU tensors the mask goes into the kernels
    (``msda_*_fused_levelref_masked_<dtype>``: no pass over the pyramid in either direction); ``mask_in_kernels=False``,
    host tensors, traced calls and a library without those symbols compose ``masked_fill`` with the unmasked route.
    ``query_mask``: ``[B, Q]`` bool / uint8, non-zero = the query is real (:func:`check_query_mask`) — a masked query's row
    of the result is zeros, its ``proj`` and ``reference_points`` rows get zero gradients and nothing it holds (NaN
    included) reaches any result.  On GPU tensors it goes into the kernels with the value mask
    (``msda_*_fused_levelref_qmasked_<dtype>``: a masked query is neither gathered for nor recorded for ``grad_value``);
    the same other routes compose :func:`apply_query_mask`."""
    qmask = None
    if query_mask is not None:
        _validate_query_mask(query_mask, proj)
        if mask_in_kernels and img.device.type == "cuda" and not torch.compiler.is_compiling() and _lib.has_query_mask():
            qmask = check_query_mask(query_mask, proj)
        else:
            out = fused_hf_module_core(img, img_shapes, apply_query_mask(proj, query_mask, 0.0),
                                       apply_query_mask(reference_points, query_mask, 0.5), padding_mode, align_corners,
                                       level_shapes, value_mask, mask_in_kernels)
            return apply_query_mask(out, query_mask, 0.0)
    mask = None
    if value_mask is not None:
        _validate_value_mask(value_mask, img)
        if mask_in_kernels and img.device.type == "cuda" and not torch.compiler.is_compiling() and _lib.has_value_mask():
            mask = check_value_mask(value_mask, img)
        else:
            img = apply_value_mask(img, value_mask)
    level_cells = level_cells_of(level_shapes, img_shapes.shape[0], img.shape[1])
    cuda = img.device.type == "cuda"
    if cuda and img_shapes.device != img.device:
        img_shapes = img_shapes.to(img.device)  # a handful of integers: follow `img`, as fused_module_core
    if cuda and not torch.compiler.is_compiling():
        _check_devices(img, proj, reference_points)
        floating = img.is_floating_point() and proj.is_floating_point() and reference_points.is_floating_point()
        same = dtypes_supported(img.dtype, proj.dtype) and reference_points.dtype == proj.dtype
        autocast = _autocast_on()
        if floating and (autocast or same or fused_storage_dtypes(img.dtype, proj.dtype, reference_points.dtype)):
            pad = _padding_code(padding_mode)
            ext = _ext.load()
            # (a masked call takes the Python Function: the C++ node has no mask argument)
            if mask is None and qmask is None and same and not autocast and KernelTimer.active is None and ext is not None and \
                    hasattr(ext, "msda_fused_levelref") and _lib.has_fused_levelref():
                # C++ autograd node; only when the fused kernels take this L*P (it never composes)
                B, I, H, D = img.shape
                key = (D, proj.element_size())
                limit = _FUSED_LP_LIMIT.get(key)
                if limit is None:
                    limit = _FUSED_LP_LIMIT[key] = int(ext.fused_lp_limit(*key))
                if proj.dim() == 6 and proj.shape[3] * proj.shape[4] <= limit and proj.shape[-1] == 3 \
                        and reference_points.dim() == 4 and reference_points.shape[-1] in (2, 4) \
                        and tuple(proj.shape[:3]) == (B, reference_points.shape[1], H) \
                        and reference_points.shape[0] == B and reference_points.shape[2] == proj.shape[3] \
                        and tuple(img_shapes.shape) == (proj.shape[3], 2):
                    _shapes_i64(img_shapes)
                    return ext.msda_fused_levelref(img, img_shapes, proj, reference_points, pad, bool(align_corners),
                                                   level_cells)
            return _HipFusedHFModuleCoreFunction.apply(img, img_shapes, proj, reference_points, padding_mode,
                                                       bool(align_corners), level_cells, mask, qmask)
    if qmask is not None:  # (dtypes the kernels do not serve: the composition, as above)
        proj, reference_points = apply_query_mask(proj, query_mask, 0.0), apply_query_mask(reference_points, query_mask, 0.5)
    out = _hf_composition(apply_value_mask(img, mask), img_shapes, proj, reference_points, padding_mode, align_corners,
                          level_shapes)
    return apply_query_mask(out, query_mask if qmask is not None else None, 0.0)


# ------------------------------------------------------------------------------------------
# ... on SPLIT projections: the offsets and the logits as the modules' two Linear layers produce them
# (msda_*_fused_levelref_split_<dtype>)
# ------------------------------------------------------------------------------------------
def split_projection_views(sampling_offsets: torch.Tensor, attention_logits: torch.Tensor, H: int, L: int):
    """The two projections as ``[B, Q, H, L, P, 2]`` and ``[B, Q, H, L, P]``: ``sampling_offsets`` in that shape or the
    ``Linear``'s flat ``[B, Q, H*L*P*2]``, ``attention_logits`` as ``[B, Q, H, L, P]``, ``[B, Q, H, L*P]`` or flat.  Views
    where the layout allows (a ``Linear``'s output always does)."""
    if sampling_offsets.dim() == 3:
        B, Q, flat = sampling_offsets.shape
        if flat % (H * L * 2) != 0 or flat == 0:
            raise ValueError(f"`sampling_offsets` [B, Q, {flat}] is not [B, Q, H*L*P*2] for H = {H}, L = {L}.")
        sampling_offsets = sampling_offsets.reshape(B, Q, H, L, flat // (H * L * 2), 2)
    if sampling_offsets.dim() != 6 or sampling_offsets.shape[-1] != 2 or tuple(sampling_offsets.shape[2:4]) != (H, L):
        raise ValueError(f"`sampling_offsets` should be [B, Q, {H}, {L}, P, 2] or [B, Q, H*L*P*2], but got "
                         f"{tuple(sampling_offsets.shape)}.")
    want = tuple(sampling_offsets.shape[:5])
    if attention_logits.dim() not in (3, 4, 5) or tuple(attention_logits.shape[:2]) != want[:2] or \
            attention_logits.numel() != sampling_offsets.numel() // 2 or \
            (attention_logits.dim() >= 4 and attention_logits.shape[2] != H):
        raise ValueError(f"`attention_logits` should be {list(want)}, [B, Q, H, L*P] or [B, Q, H*L*P] next to "
                         f"`sampling_offsets` {tuple(sampling_offsets.shape)}, but got {tuple(attention_logits.shape)}.")
    return sampling_offsets, attention_logits.reshape(want)


def stack_split_projection(sampling_offsets: torch.Tensor, attention_logits: torch.Tensor) -> torch.Tensor:
    """``[B, Q, H, L, P, 3]`` (dx, dy, logit) from the split pair: the pass :func:`fused_hf_module_core_split` saves."""
    return torch.cat([sampling_offsets, attention_logits[..., None]], -1)


class _SplitCallDeclined(Exception):
    """Raised by the forward of :class:`_HipFusedHFSplitFunction` when the library declines the call
    (``MSDA_ERR_UNSUPPORTED``; nothing was launched): :func:`fused_hf_module_core_split` catches it and composes."""


def msda_hip_fwd_fused_split(img, img_shapes, offsets, logits, reference_points, padding_mode,
                             align_corners) -> Optional[torch.Tensor]:
    """:func:`msda_hip_fwd_fused` with ``levelref=True`` on split projections (``msda_fwd_fused_levelref_split_<dtype>``):
    ``offsets`` ``[B, Q, H, L, P, 2]``, ``logits`` ``[B, Q, H, L, P]``.  None when the library declines or lacks the symbol."""
    B, I, H, D = img.shape
    B2, Q, H2, L, P, two = offsets.shape
    if (B2, H2, two) != (B, H, 2) or tuple(logits.shape) != (B, Q, H, L, P) or logits.dtype != offsets.dtype or \
            tuple(reference_points.shape[:3]) != (B, Q, L) or reference_points.dim() != 4:
        raise ValueError(f"inconsistent shapes: img {tuple(img.shape)}, offsets {tuple(offsets.shape)}, logits "
                         f"{tuple(logits.shape)} ({logits.dtype} / {offsets.dtype}), reference_points "
                         f"{tuple(reference_points.shape)}")
    ref_dim = reference_points.shape[-1]
    if ref_dim not in (2, 4):
        raise ValueError(f"`reference_points` should have the last dim either 2 or 4, but got {ref_dim}.")
    if tuple(img_shapes.shape) != (L, 2):
        raise ValueError(f"`img_shapes` should be [{L}, 2], but got {tuple(img_shapes.shape)}.")
    suf, pad, img, vrow, shapes, offsets, reference_points, _, logits = _fused_prepare(
        img, img_shapes, offsets, reference_points, padding_mode, logits=logits)
    name = "msda_fwd_fused_levelref_split"
    fn = getattr(_lib.load(), f"{name}_{suf}", None)
    if fn is None:
        return None
    out = torch.empty((B, Q, H, D), dtype=offsets.dtype, device=img.device)
    ok = _fused_run(name, f"{name}_{suf}", img.device, fn,
                    (img.data_ptr(), shapes.data_ptr(), offsets.data_ptr(), logits.data_ptr(), reference_points.data_ptr(),
                     out.data_ptr(), B, I, H, D, Q, L, P, ref_dim, pad, int(bool(align_corners)), vrow))
    return out if ok else None


def msda_hip_bwd_fused_split(out_grad, img, img_shapes, offsets, logits, reference_points, padding_mode, align_corners,
                             need_img: bool = True, level_cells: int = 0, need_ref: bool = True):
    """:func:`msda_hip_bwd_fused` with ``levelref=True`` on split projections (``msda_bwd_fused_levelref_split_<dtype>``):
    ``(img_grad | None, offsets_grad, logits_grad, reference_points_grad | None)``, or None when the library declines."""
    B, I, H, D = img.shape
    _, Q, _, L, P, _ = offsets.shape
    ref_dim = reference_points.shape[-1]
    suf, pad, img, vrow, shapes, offsets, reference_points, out_grad, logits = _fused_prepare(
        img, img_shapes, offsets, reference_points, padding_mode, out_grad, logits)
    lib = _lib.load()
    name = "msda_bwd_fused_levelref_split"
    fn = getattr(lib, f"{name}_{suf}", None)
    if fn is None:
        return None
    cdt = offsets.dtype
    g_img = torch.empty((B, I, H, D), dtype=img.dtype, device=img.device) if need_img else None
    g_off = torch.empty((B, Q, H, L, P, 2), dtype=cdt, device=img.device)
    g_lgt = torch.empty((B, Q, H, L, P), dtype=cdt, device=img.device)
    g_ref_part = torch.empty((B, Q, H, L, ref_dim), dtype=reference_points.dtype, device=img.device)
    level_cells = int(level_cells)
    # (the interleaved pair's workspace: its query answers for these calls too)
    ws, ws_bytes = _fused_workspace(need_img, lib.msda_bwd_fused_workspace_bytes, (B, I, H, D, Q, L, P), suf, offsets, img,
                                    level_cells)
    if not _fused_run(name, f"{name}_{suf}", img.device, fn,
                      (out_grad.data_ptr(), img.data_ptr(), shapes.data_ptr(), offsets.data_ptr(), logits.data_ptr(),
                       reference_points.data_ptr(), g_img.data_ptr() if need_img else None, g_off.data_ptr(),
                       g_lgt.data_ptr(), g_ref_part.data_ptr(), B, I, H, D, Q, L, P, ref_dim, pad, int(bool(align_corners)),
                       level_cells, vrow, ws.data_ptr() if need_img else None, ws_bytes)):
        return None
    return g_img, g_off, g_lgt, (g_ref_part.sum(dim=2) if need_ref else None)


class _HipFusedHFSplitFunction(Function):
    """:class:`_HipFusedHFModuleCoreFunction` on split projections (``msda_*_fused_levelref_split_<dtype>``).  A forward the
    library declines raises :class:`_SplitCallDeclined` — the caller composes; a backward it declines (the limits are the
    forward's, so this is a library swapped in between) differentiates that composition."""

    @staticmethod
    @custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, img, img_shapes, offsets, logits, reference_points, padding_mode, align_corners, level_cells=0):
        ctx.level_cells = int(level_cells)
        out = msda_hip_fwd_fused_split(img, img_shapes, offsets, logits, reference_points, padding_mode, align_corners)
        if out is None:
            raise _SplitCallDeclined()
        ctx.save_for_backward(img, img_shapes, offsets, logits, reference_points)
        ctx.padding_mode, ctx.align_corners = padding_mode, align_corners
        return out

    @staticmethod
    @once_differentiable
    @custom_bwd(device_type="cuda")
    def backward(ctx, out_grad):
        img, img_shapes, offsets, logits, reference_points = ctx.saved_tensors
        need_img, _, need_off, need_lgt, need_ref = ctx.needs_input_grad[:5]
        res = msda_hip_bwd_fused_split(out_grad, img, img_shapes, offsets, logits, reference_points, ctx.padding_mode,
                                       ctx.align_corners, need_img, level_cells=ctx.level_cells, need_ref=need_ref)
        if res is None:
            with torch.enable_grad():
                leaves = [t.detach().requires_grad_(n) for t, n in ((img, need_img), (offsets, need_off), (logits, need_lgt),
                                                                    (reference_points, need_ref))]
                out = fused_hf_module_core(leaves[0], img_shapes, stack_split_projection(leaves[1], leaves[2]), leaves[3],
                                           ctx.padding_mode, ctx.align_corners)
                wrt = [t for t in leaves if t.requires_grad]
                got = iter(torch.autograd.grad(out, wrt, out_grad.to(out.dtype), allow_unused=True))
            res = [next(got) if t.requires_grad else None for t in leaves]
        g_img, g_off, g_lgt, g_ref = res
        return (g_img if need_img else None, None, g_off if need_off else None, g_lgt if need_lgt else None,
                g_ref if need_ref else None, None, None, None)


def fused_hf_module_core_split(img, img_shapes, sampling_offsets, attention_logits, reference_points, padding_mode,
                               align_corners, level_shapes=None, value_mask=None, query_mask=None,
                               split_in_kernels: bool = True) -> torch.Tensor:
    """:func:`fused_hf_module_core` on the tensors a Hugging Face (or original Deformable-DETR, or mmcv) attention module
    has: ``sampling_offsets`` ``[B, Q, H, L, P, 2]`` — or its ``Linear``'s flat ``[B, Q, H*L*P*2]`` — and
    ``attention_logits`` ``[B, Q, H, L, P]``, ``[B, Q, H, L*P]`` or flat.  Its definition, and its route for host tensors,
    is ``fused_hf_module_core(img, img_shapes, cat([offsets, logits[..., None]], -1), ...)``.  GPU tensors of the dtypes
    that function's kernels serve (autocast and 16-bit storage next to fp32 reference points included) go to
    ``msda_*_fused_levelref_split_<dtype>``, which read the two tensors where they are — no interleaving pass in either
    direction — and return bit for bit what the interleaved kernels return.  Traced calls, a library without the symbols,
    ``L * P`` beyond ``msda_fused_lp_limit``, a forward the library declines and ``split_in_kernels=False`` take the
    composition.  ``value_mask`` / ``query_mask`` (``[B, I]`` / ``[B, Q]``, non-zero = real) compose around either route
    with :func:`apply_value_mask` / :func:`apply_query_mask`.  Gradients go to ``img``, both projections and
    ``reference_points``."""
    if img.dim() != 4:
        raise ValueError(f"`img` should be [B, I, H, D], but got {tuple(img.shape)}.")
    offsets, logits = split_projection_views(sampling_offsets, attention_logits, img.shape[2], img_shapes.shape[0])
    if query_mask is not None:
        _validate_query_mask(query_mask, offsets)
        offsets, logits = apply_query_mask(offsets, query_mask, 0.0), apply_query_mask(logits, query_mask, 0.0)
        reference_points = apply_query_mask(reference_points, query_mask, 0.5)
    img = apply_value_mask(img, value_mask)
    out = None
    cuda = img.device.type == "cuda"
    if split_in_kernels and cuda and not torch.compiler.is_compiling() and offsets.dtype == logits.dtype and \
            _lib.has_levelref_split():
        _check_devices(img, offsets, logits, reference_points)
        floating = img.is_floating_point() and offsets.is_floating_point() and reference_points.is_floating_point()
        same = dtypes_supported(img.dtype, offsets.dtype) and reference_points.dtype == offsets.dtype
        autocast = _autocast_on()
        storage = fused_storage_dtypes(img.dtype, offsets.dtype, reference_points.dtype)
        if floating and (autocast or same or storage) and \
                offsets.shape[3] * offsets.shape[4] <= fused_lp_limit(img.shape[3], 4 if (autocast or storage)
                                                                      else offsets.element_size()):
            if img_shapes.device != img.device:
                img_shapes = img_shapes.to(img.device)
            try:
                out = _HipFusedHFSplitFunction.apply(img, img_shapes, offsets, logits, reference_points, padding_mode,
                                                     bool(align_corners),
                                                     level_cells_of(level_shapes, img_shapes.shape[0], img.shape[1]))
            except _SplitCallDeclined:
                out = None
    if out is None:
        out = fused_hf_module_core(img, img_shapes, stack_split_projection(offsets, logits), reference_points, padding_mode,
                                   align_corners, level_shapes)
    return apply_query_mask(out, query_mask, 0.0)


# ------------------------------------------------------------------------------------------
# ... and for the Hugging Face modules with per-level point counts and the box rule (D-FINE, DEIMv2, RT-DETRv2:
# transformers/models/d_fine/modeling_d_fine.py, DFineMultiscaleDeformableAttention.forward)
# ------------------------------------------------------------------------------------------
def hf_box_level_scale(points_per_level) -> Tuple[float, ...]:
    """transformers' ``num_points_scale`` per level, as host numbers: the modules build an fp32 buffer from ``1 / P_l``,
    so the scale is ``float32(1 / P_l)`` — in fp64 that value widened, not ``1 / P_l``."""
    return tuple(float(np.float32(1 / int(p))) for p in points_per_level)


def hf_box_sampling_inputs(proj: torch.Tensor, reference_points: torch.Tensor, points_per_level, offset_scale: float = 0.5):
    """The box prologue of transformers' D-FINE / DEIMv2 / RT-DETRv2 attention modules in plain PyTorch, with transformers'
    own operations in transformers' own order: raw projection ``[B, N, H, S, 3]`` (x offset, y offset, logit per sample,
    ``S = sum(points_per_level)``, level-major) and ONE box per query ``[B, N, 4]`` or ``[B, N, 1, 4]`` ->
    (sampling_points ``[B, N, H, S, 2]``, attention_weights ``[B, N, H, S]``).  It differs from
    :func:`msda_triton_amd.ragged.ragged_module_sampling_inputs` (``ref_xy + o * ref_wh / (2 P_l)``) in the order of the
    operations and in the scale, which is the fp32 value :func:`hf_box_level_scale` converted to the working dtype."""
    counts = tuple(int(p) for p in points_per_level)
    if proj.dim() != 5 or proj.shape[-1] != 3 or proj.shape[3] != sum(counts) or any(p < 1 for p in counts):
        raise ValueError(f"expected proj [B,N,H,S,3] with S = sum(points_per_level) = {sum(counts)} and every count at "
                         f"least 1; got {tuple(proj.shape)}, {list(counts)}")
    if reference_points.dim() == 3:
        reference_points = reference_points[:, :, None, :]
    if reference_points.dim() != 4 or reference_points.shape[2] != 1 or reference_points.shape[-1] != 4 or \
            tuple(reference_points.shape[:2]) != tuple(proj.shape[:2]):
        raise ValueError(f"`reference_points` should be [B, N, 4] or [B, N, 1, 4] (one box per query) next to proj "
                         f"{tuple(proj.shape)}, but got {tuple(reference_points.shape)}.")
    sampling_offsets, logits = proj[..., :2], proj[..., 2]
    attention_weights = torch.nn.functional.softmax(logits, dim=-1)
    scale = [s for s, n in zip(hf_box_level_scale(counts), counts) for _ in range(n)]
    num_points_scale = torch.tensor(scale, dtype=torch.float32, device=proj.device).to(dtype=proj.dtype).unsqueeze(-1)
    offset = sampling_offsets * num_points_scale * reference_points[:, :, None, :, 2:] * offset_scale
    sampling_locations = reference_points[:, :, None, :, :2] + offset
    return sampling_locations, attention_weights


def fused_hf_box_core(img, img_shapes, proj, reference_points, points_per_level, offset_scale: float = 0.5,
                      padding_mode: Optional[str] = None, align_corners: Optional[bool] = None, level_shapes=None,
                      value_mask=None, query_mask=None, sampling_mode: str = "bilinear") -> torch.Tensor:
    """``multiscale_deformable_attention(img, img_shapes, *hf_box_sampling_inputs(proj, ...), points_per_level=...)``: the
    core of a D-FINE / DEIMv2 / RT-DETRv2 attention module between its projections — value pyramid ``[B, I, H, D]``, raw
    projection ``[B, Q, H, S, 3]`` (level-major), boxes ``[B, Q, 4]`` or ``[B, Q, 1, 4]``.  On GPU tensors the prologue and
    its chain rule run inside the gather kernels (``msda_*_fused_hfbox_<dtype>``, equal counts included); on host tensors,
    while traced and where the library declines it is exactly that composition (:mod:`msda_triton_amd.ragged`).
    ``value_mask``: ``[B, I]``, non-zero = the pixel is real; composed as ``masked_fill`` in front of the kernels.
    ``query_mask``: ``[B, Q]``, non-zero = the query is real; composed likewise (:func:`apply_query_mask`).
    ``padding_mode`` / ``align_corners`` default to ``"zeros"`` / ``False``, what these modules sample with.

    ``sampling_mode="discrete"`` (the modules' ``decoder_method="discrete"``): the same prologue in front of
    :mod:`msda_triton_amd.discrete` — ``multiscale_deformable_attention(img, img_shapes, *hf_box_sampling_inputs(proj, ...),
    "border", False, points_per_level=..., sampling_mode="discrete")``, on GPU tensors inside
    ``msda_*_fused_hfbox_discrete_<dtype>``.  ``padding_mode`` / ``align_corners`` have no meaning there: leave them out, or
    pass ``"border"`` / ``False``.  ``reference_points`` gets no gradient (``None``) and the offset slots of ``proj`` exact
    zeros: the pixel index is an integer.  The kernels form the point in fp32 from the stored values; for all-16-bit
    tensors transformers forms it in 16 bits and can land on the neighbouring pixel."""
    if sampling_mode not in ("bilinear", "discrete"):
        raise ValueError(f'`sampling_mode` should be "bilinear" or "discrete", but got {sampling_mode!r}.')
    if sampling_mode == "discrete":
        from .discrete import check_discrete_mode
        check_discrete_mode("border" if padding_mode is None else padding_mode, bool(align_corners))
        padding_mode, align_corners = "border", False
    else:
        padding_mode = "zeros" if padding_mode is None else padding_mode
        align_corners = False if align_corners is None else align_corners
    if query_mask is not None:
        out = fused_hf_box_core(img, img_shapes, apply_query_mask(proj, query_mask, 0.0),
                                apply_query_mask(reference_points, query_mask, 0.5), points_per_level, offset_scale,
                                padding_mode, align_corners, level_shapes, value_mask, sampling_mode=sampling_mode)
        return apply_query_mask(out, query_mask, 0.0)
    if sampling_mode == "discrete":
        from .discrete import fused_hf_box_discrete_core
        return fused_hf_box_discrete_core(apply_value_mask(img, value_mask), img_shapes, proj, reference_points,
                                          points_per_level, offset_scale, level_shapes)
    from .ragged import fused_hf_box_module_core
    return fused_hf_box_module_core(apply_value_mask(img, value_mask), img_shapes, proj, reference_points, points_per_level, offset_scale, padding_mode,
                                    align_corners, level_shapes)


# ------------------------------------------------------------------------------------------
# host-tensor path (reference: native_multiscale_deformable_attention, frontend.py:15-68)
# ------------------------------------------------------------------------------------------
def _unnormalise(coord: torch.Tensor, size: int, padding_mode: str, align_corners: bool) -> torch.Tensor:
    pix = coord * (size - 1) if align_corners else coord * size - 0.5
    if padding_mode == "border":
        # grid_sample clips the coordinate to [0, size-1] and kills its gradient at and beyond the border
        inside = (pix > 0) & (pix < size - 1)
        pix = torch.where(inside, pix, pix.detach().clamp(0, size - 1))
    return pix


def native_multiscale_deformable_attention(
    img: torch.Tensor,
    img_shapes: torch.Tensor,
    sampling_points: torch.Tensor,
    attention_weights: torch.Tensor,
    padding_mode: Literal["border", "zeros"],
    align_corners: bool,
) -> torch.Tensor:
    """Plain-PyTorch path for host tensors, differentiable through autograd (the reference's documented CPU
    behaviour, frontend.py:15-68).

    Per level, every (batch, head) plane is one ``[D, h, w]`` image for ``F.grid_sample`` — PyTorch's vectorised
    bilinear sampler, forward and backward — and the level's samples are folded into the result straight away by a
    contraction with the attention weights over the point axis, so the ``[B, Q, H, L, P, D]`` sample tensor is never
    built.  Like the reference it reads ``img_shapes`` on the host.  ``_gather_multiscale_deformable_attention`` below
    states the same operator without ``grid_sample`` (tests hold the two to each other and to the reference's golden
    vectors).
    """
    _padding_code(padding_mode)
    B, I, H, D, Q, L, P = _dims(img, sampling_points, attention_weights, img_shapes)
    dt = torch.result_type(img, sampling_points)
    planes = img.to(dt).permute(0, 2, 3, 1).reshape(B * H, D, I)          # [B*H, D, I]: a plane's channels as images
    grid = (2 * sampling_points.to(dt) - 1).permute(0, 2, 3, 1, 4, 5)      # [B, H, L, Q, P, 2] in grid_sample's [-1, 1]
    weights = attention_weights.to(dt).permute(0, 2, 3, 1, 4)              # [B, H, L, Q, P]
    out = None
    start = 0
    for lvl, (h, w) in enumerate(img_shapes.tolist()):
        level = planes[:, :, start:start + h * w].reshape(B * H, D, h, w)
        sampled = torch.nn.functional.grid_sample(level, grid[:, :, lvl].reshape(B * H, Q, P, 2), mode="bilinear",
                                                  padding_mode=padding_mode, align_corners=align_corners)  # [B*H, D, Q, P]
        part = torch.einsum("ndqp,nqp->nqd", sampled, weights[:, :, lvl].reshape(B * H, Q, P))
        out = part if out is None else out + part
        start += h * w
    if out is None:
        out = planes.new_zeros((B * H, Q, D))
    return out.reshape(B, H, Q, D).permute(0, 2, 1, 3).contiguous()


def _gather_multiscale_deformable_attention(img, img_shapes, sampling_points, attention_weights, padding_mode, align_corners):
    """The operator as index arithmetic + ``gather`` (no ``grid_sample``): an independent statement of SURVEY 9.1, kept
    as a cross-check of the host path (slow: its backward is four ``scatter_add`` per level)."""
    _padding_code(padding_mode)
    B, I, H, D, Q, L, P = _dims(img, sampling_points, attention_weights, img_shapes)
    planes = img.permute(0, 2, 1, 3)  # [B, H, I, D]
    out = img.new_zeros((B, H, Q, D), dtype=torch.result_type(img, sampling_points))
    start = 0
    for lvl, (h, w) in enumerate(img_shapes.tolist()):
        plane = planes[:, :, start:start + h * w]                      # [B, H, h*w, D]
        pts = sampling_points[:, :, :, lvl].permute(0, 2, 1, 3, 4)     # [B, H, Q, P, 2]
        att = attention_weights[:, :, :, lvl].permute(0, 2, 1, 3)      # [B, H, Q, P]
        px = _unnormalise(pts[..., 0], w, padding_mode, align_corners)
        py = _unnormalise(pts[..., 1], h, padding_mode, align_corners)
        x0, y0 = px.detach().floor(), py.detach().floor()
        dx, dy = px - x0, py - y0
        level_sample = 0
        for yo, xo, wgt in ((0, 0, (1 - dy) * (1 - dx)), (0, 1, (1 - dy) * dx), (1, 0, dy * (1 - dx)), (1, 1, dy * dx)):
            xi, yi = x0 + xo, y0 + yo
            valid = (xi >= 0) & (xi <= w - 1) & (yi >= 0) & (yi <= h - 1)
            idx = (yi.clamp(0, h - 1) * w + xi.clamp(0, w - 1)).long()            # [B, H, Q, P]
            rows = plane.gather(2, idx.reshape(B, H, Q * P, 1).expand(-1, -1, -1, D)).reshape(B, H, Q, P, D)
            level_sample = level_sample + rows * (wgt * valid.to(wgt.dtype)).unsqueeze(-1)
        out = out + (level_sample * att.unsqueeze(-1)).sum(dim=3)
        start += h * w
    return out.permute(0, 2, 1, 3).contiguous()


# ------------------------------------------------------------------------------------------
# public entry (reference: multiscale_deformable_attention, frontend.py:145-172)
# ------------------------------------------------------------------------------------------
def multiscale_deformable_attention(
    img: torch.Tensor,
    img_shapes: torch.Tensor,
    sampling_points: torch.Tensor,
    attention_weights: torch.Tensor,
    padding_mode: Literal["border", "zeros"],
    align_corners: bool,
    level_shapes=None,
    points_per_level=None,
    sampling_mode: Literal["bilinear", "discrete"] = "bilinear",
    value_mask: Optional[torch.Tensor] = None,
    query_mask: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """Differentiable multiscale deformable attention.

    Args:
        img: flattened image pyramid ``[batch, num_image, num_heads, num_channels]`` with
            ``num_image = sum(h*w)`` over the levels.
        img_shapes: ``[num_levels, 2]`` integer tensor of (height, width).
        sampling_points: ``[batch, num_queries, num_heads, num_levels, num_points, 2]`` in (x, y)
            order, normalised to [0, 1] with (0, 0) the top-left corner.
        attention_weights: ``[batch, num_queries, num_heads, num_levels, num_points]``.
        padding_mode: ``"border"`` (clamp to the nearest pixel) or ``"zeros"``.
        align_corners: grid alignment, as in ``torch.nn.functional.grid_sample``.
        level_shapes: optional, not in the reference — the same (height, width) pairs as HOST numbers (e.g. Hugging
            Face's ``spatial_shapes_list``).  ``img_shapes`` lives on the device and is never read back, so without
            this the backward must assume the largest level ``num_image`` pixels can form; with it, decoder-sized
            calls over real-image pyramids take the single-launch grad_value kernel (see :func:`level_cells_of`).
        points_per_level: optional, not in the reference — a point count per level (D-FINE / DEIMv2's
            ``num_points_list``).  Then ``sampling_points`` is ``[batch, num_queries, num_heads, S, 2]`` and
            ``attention_weights`` ``[batch, num_queries, num_heads, S]`` with ``S = sum(points_per_level)``, level-major
            (samples ``[start_l, start_l + P_l)`` belong to level ``l``).  Equal counts take the uniform call on a view.
        sampling_mode: optional, not in the reference — ``"bilinear"`` (default) or ``"discrete"``: every sample reads the
            one pixel ``(clamp(trunc(x * w + 0.5), 0, w - 1), clamp(trunc(y * h + 0.5), 0, h - 1))`` and nothing is
            interpolated (transformers' ``method="discrete"``; see :mod:`msda_triton_amd.discrete`).  Accepted only with
            ``padding_mode="border"``, ``align_corners=False`` (neither has a meaning there), with or without
            ``points_per_level``; ``sampling_points`` gets no gradient (``None``).
        value_mask: optional, not in the reference — ``[batch, num_image]`` bool or uint8 on ``img``'s device, non-zero =
            the pixel is real (transformers' ``attention_mask`` polarity; mmcv's ``key_padding_mask`` is the inverse).  A
            padding pixel counts as zeros whatever it holds (NaN included): the results are those of the call on
            ``where(mask, img, 0)``, and ``img``'s gradient is zero there.  The mask takes no gradient.  GPU tensors with
            a uniform point count run the value-mask kernels (no extra pass over the pyramid in either direction);
            host tensors, ``points_per_level``, ``sampling_mode="discrete"`` and traced calls compose ``masked_fill``
            with their route.
        query_mask: optional, not in the reference — ``[batch, num_queries]`` bool or uint8 on the queries' device,
            non-zero = the query is real (the polarity of ``value_mask``; an encoder layer over a padded batch passes one
            mask for both).  A masked query's row of the result is zeros, its sampling points and attention weights get
            zero gradients, and NOTHING it holds — NaN, Inf or far-off coordinates in its points, weights or ``grad_out``
            row — reaches ``img``'s gradient or any other result.  Real queries' rows are those of the call without the
            mask, bit for bit.  The mask takes no gradient.  GPU tensors with a uniform point count run the query-mask
            entry points (a masked query is neither gathered for nor recorded for ``img``'s gradient); host tensors,
            ``points_per_level``, ``sampling_mode="discrete"`` and traced calls compose :func:`apply_query_mask` with
            their route, which is also the definition: the call on inputs whose masked queries hold points 0.5 and
            weights 0, with the masked rows of the result zeroed.

    Returns:
        ``[batch, num_queries, num_heads, num_channels]``.

    Tensors on an AMD GPU ("cuda" device type on ROCm) run the hand-written gfx950 kernels and
    never fall back; host tensors run the plain-PyTorch formulation.
    """
    if query_mask is not None:
        _validate_query_mask(query_mask, sampling_points)
        if sampling_mode == "bilinear" and points_per_level is None and img.device.type == "cuda":
            return hip_multiscale_deformable_attention(img, img_shapes, sampling_points, attention_weights, padding_mode,
                                                       align_corners, level_shapes, value_mask=value_mask,
                                                       query_mask=query_mask)
        out = multiscale_deformable_attention(
            img, img_shapes, apply_query_mask(sampling_points, query_mask, 0.5),
            apply_query_mask(attention_weights, query_mask, 0.0), padding_mode, align_corners, level_shapes,
            points_per_level, sampling_mode, value_mask)
        return apply_query_mask(out, query_mask, 0.0)
    if value_mask is not None:
        _validate_value_mask(value_mask, img)
        if sampling_mode == "bilinear" and points_per_level is None and img.device.type == "cuda":
            return hip_multiscale_deformable_attention(img, img_shapes, sampling_points, attention_weights, padding_mode,
                                                       align_corners, level_shapes, value_mask=value_mask)
        img = apply_value_mask(img, value_mask)
    if sampling_mode != "bilinear":
        if sampling_mode != "discrete":
            raise ValueError(f'`sampling_mode` should be "bilinear" or "discrete", but got {sampling_mode!r}.')
        from .discrete import discrete_multiscale_deformable_attention
        return discrete_multiscale_deformable_attention(img, img_shapes, sampling_points, attention_weights, padding_mode,
                                                        align_corners, points_per_level, level_shapes)
    if points_per_level is not None:
        from .ragged import ragged_multiscale_deformable_attention
        return ragged_multiscale_deformable_attention(img, img_shapes, sampling_points, attention_weights, padding_mode,
                                                      align_corners, points_per_level, level_shapes)
    if img.device.type == "cuda":
        return hip_multiscale_deformable_attention(
            img, img_shapes, sampling_points, attention_weights, padding_mode, align_corners, level_shapes)
    return native_multiscale_deformable_attention(
        img, img_shapes, sampling_points, attention_weights, padding_mode, align_corners)
