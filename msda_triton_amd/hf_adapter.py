"""Adapter for Hugging Face Deformable-DETR / Grounding-DINO style models.

Those models call a parameter-free ``MultiScaleDeformableAttention`` module
(``transformers/models/{deformable_detr,grounding_dino,...}/modeling_*.py``) with

    forward(value, value_spatial_shapes, value_spatial_shapes_list, level_start_index,
            sampling_locations, attention_weights, im2col_step) -> [batch, queries, heads * head_dim]

which is this operator with ``padding_mode="zeros"``, ``align_corners=False`` followed by a flatten of
the (head, channel) axes — the parity demo of the reference's README (README.md:25-37).
``level_start_index`` and ``im2col_step`` are accepted and ignored (level starts are derived from the
shapes in-kernel, exactly as the reference does, kernels.py:58-62).

D-FINE / DEIMv2 (``transformers/models/{d_fine,deimv2}/modeling_*.py``) instead keep their core as an instance
attribute, ``module.ms_deformable_attn_core(value, spatial_shapes_list, sampling_locations, attention_weights,
num_points_list, method)`` with a point count per level; :func:`ms_deformable_attn_core` is that function over the
per-level-count kernels (``method="default"`` only: zeros padding, ``align_corners=False``).
:func:`ms_deformable_attn_core_v2` serves both of transformers' methods — ``"default"`` as above and ``"discrete"`` (one
rounded pixel per sample, :mod:`msda_triton_amd.discrete`) — and is what ``replace_hf_msda(model, discrete=True)`` sets.
"""
from __future__ import annotations

import inspect
import sys

import numpy as np
import torch
from torch import nn

from ._linear import _plain_linear
from .functional import (_autocast_on, fused_hf_box_core, fused_hf_module_core, fused_hf_module_core_split,
                         hf_box_level_scale, multiscale_deformable_attention)


class MultiScaleDeformableAttention(nn.Module):
    """Drop-in for the HF module of the same name; runs the MI355X HIP kernels on GPU tensors."""

    def forward(self, value: torch.Tensor, value_spatial_shapes: torch.Tensor, value_spatial_shapes_list=None,
                level_start_index=None, sampling_locations: torch.Tensor = None,
                attention_weights: torch.Tensor = None, im2col_step: int = 64) -> torch.Tensor:
        shapes = value_spatial_shapes
        if not torch.is_tensor(shapes):
            shapes = torch.as_tensor(shapes if shapes is not None else value_spatial_shapes_list,
                                     dtype=torch.int64, device=value.device)
        elif shapes.device != value.device:
            shapes = shapes.to(value.device)
        # the level sizes as host numbers, when the model carries them (transformers >= 4.46 passes
        # `spatial_shapes_list`): lets the backward size its single-launch grad_value kernel for the real levels
        # (decoder layers at image size: 1.4x faster there); never read back from the device
        level_shapes = value_spatial_shapes_list if isinstance(value_spatial_shapes_list, (list, tuple)) else None
        dtype = value.dtype
        if value.device.type == "cuda" and dtype in (torch.bfloat16, torch.float16) and \
                sampling_locations.dtype == torch.float32 and attention_weights.dtype == torch.float32:
            # what autocast hands this module: a 16-bit value pyramid (from the value projection) next to fp32
            # sampling locations / softmaxed weights.  The mixed-storage kernels read the pyramid as it is and keep
            # the coordinates in fp32 (casting them to 16 bits would cost a quarter pixel on a 64-px level; casting
            # everything to fp32, which autocast's policy for the plain operator does, copies the pyramid).
            autocast = _autocast_on()
            with torch.autocast("cuda", enabled=False):
                out = multiscale_deformable_attention(value, shapes, sampling_locations, attention_weights, "zeros", False,
                                                      level_shapes=level_shapes)
            return (out if autocast else out.to(dtype)).flatten(2)
        if sampling_locations.dtype != dtype:
            sampling_locations = sampling_locations.to(dtype)
        if attention_weights.dtype != dtype:
            attention_weights = attention_weights.to(dtype)
        out = multiscale_deformable_attention(value, shapes, sampling_locations, attention_weights, "zeros", False,
                                              level_shapes=level_shapes)
        return out.flatten(2)


_SHAPES_CACHE: dict = {}  # (shapes tuple, device) -> int64 [L, 2] tensor: no host-to-device copy per call


def _shapes_tensor(shapes_list, device) -> torch.Tensor:
    key = (tuple((int(h), int(w)) for h, w in shapes_list), str(device))
    t = _SHAPES_CACHE.get(key)
    if t is None:
        t = _SHAPES_CACHE[key] = torch.tensor(key[0], dtype=torch.int64, device=device)
    return t


def ms_deformable_attn_core(value: torch.Tensor, spatial_shapes_list, sampling_locations: torch.Tensor,
                            attention_weights: torch.Tensor, num_points_list, method: str = "default") -> torch.Tensor:
    """transformers' ``multi_scale_deformable_attention_v2`` (D-FINE / DEIMv2) for ``method="default"``: value
    ``[B, I, H, D]``, the level shapes as host numbers, sampling locations ``[B, Q, H, S, 2]``, attention weights
    ``[B, Q, H, S]``, ``num_points_list`` the L point counts (S their sum).  Returns ``[B, Q, H * D]``."""
    if method != "default":
        raise ValueError(f"ms_deformable_attn_core serves method='default' only, got {method!r}")
    return _core(value, spatial_shapes_list, sampling_locations, attention_weights, num_points_list, "bilinear")


def ms_deformable_attn_core_v2(value: torch.Tensor, spatial_shapes_list, sampling_locations: torch.Tensor,
                               attention_weights: torch.Tensor, num_points_list, method: str = "default") -> torch.Tensor:
    """transformers' ``multi_scale_deformable_attention_v2`` for both of its methods, with the signature the D-FINE /
    DEIMv2 decoders call: ``"default"`` is :func:`ms_deformable_attn_core`; ``"discrete"`` reads the one pixel
    ``clamp(trunc(x * w + 0.5), 0, w - 1)`` / ``clamp(trunc(y * h + 0.5), 0, h - 1)`` per sample and gives the sampling
    locations no gradient, as transformers' own."""
    if method not in ("default", "discrete"):
        raise ValueError(f"ms_deformable_attn_core_v2 serves method='default' and 'discrete', got {method!r}")
    return _core(value, spatial_shapes_list, sampling_locations, attention_weights, num_points_list,
                 "discrete" if method == "discrete" else "bilinear")


def _core(value, spatial_shapes_list, sampling_locations, attention_weights, num_points_list, mode):
    # bilinear: transformers samples with zeros padding; discrete: no padding mode ("border" is what the call accepts)
    pad = "zeros" if mode == "bilinear" else "border"
    level_shapes = [(int(h), int(w)) for h, w in spatial_shapes_list]
    shapes = _shapes_tensor(level_shapes, value.device)
    counts = [int(p) for p in num_points_list]
    dtype = value.dtype
    if value.device.type == "cuda" and dtype in (torch.bfloat16, torch.float16) and \
            sampling_locations.dtype == torch.float32 and attention_weights.dtype == torch.float32:
        # the mixed storage, as MultiScaleDeformableAttention.forward above
        autocast = _autocast_on()
        with torch.autocast("cuda", enabled=False):
            out = multiscale_deformable_attention(value, shapes, sampling_locations, attention_weights, pad, False,
                                                  level_shapes=level_shapes, points_per_level=counts, sampling_mode=mode)
        return (out if autocast else out.to(dtype)).flatten(2)
    if sampling_locations.dtype != dtype:
        sampling_locations = sampling_locations.to(dtype)
    if attention_weights.dtype != dtype:
        attention_weights = attention_weights.to(dtype)
    out = multiscale_deformable_attention(value, shapes, sampling_locations, attention_weights, pad, False,
                                          level_shapes=level_shapes, points_per_level=counts, sampling_mode=mode)
    return out.flatten(2)


# Measured (profiles/r12_hf_mask_bench.json): with the mask in the kernels the core's forward plus backward is
# ahead of masked_fill + the unmasked kernels by the project's rule — slowest repeat below the other leg's fastest — at
# the Deformable-DETR encoder shape in fp32 and at the Grounding-DINO decoder shape in fp32 and with bf16 storage.  fp16
# and fp64 pyramids were not measured and keep masked_fill.  False: every call keeps masked_fill (A/B runs).
MASK_IN_KERNELS = True


def mask_in_kernels(value: torch.Tensor, num_queries: int) -> bool:
    """Does the fused adapter hand a padding mask to the value-mask kernels (``fused_hf_module_core(value_mask=...)``) for
    this call, or keep transformers' ``masked_fill`` in front of the unmasked kernels?  The project's rule (DESIGN.md 15,
    17): the kernels take the mask only where their slowest measured repeat was below ``masked_fill``'s fastest, forward
    plus backward."""
    return bool(MASK_IN_KERNELS) and value.device.type == "cuda" and value.dtype in (torch.float32, torch.bfloat16)


# Measured (profiles/r17_levelref_split_bench.json): storage dtypes for which the split-projection kernels
# (msda_*_fused_levelref_split_<dtype>) are ahead of `cat` + the interleaved kernels by the project's rule — slowest repeat
# below the other leg's fastest, forward plus backward.  The adapter's non-plain route hands the two layers' outputs to those
# kernels for these dtypes and interleaves them for every other one.
SPLIT_IN_KERNELS_DTYPES = (torch.float32, torch.bfloat16)


def split_in_kernels(value: torch.Tensor) -> bool:
    """Does the adapter's route for non-plain projection layers take the split-projection kernels for this pyramid, or
    interleave the two outputs in front of the interleaved kernels (the rule above)?"""
    return value.device.type == "cuda" and value.dtype in SPLIT_IN_KERNELS_DTYPES


class FusedHFDeformableAttention:
    """Mixed into the class of a Hugging Face attention module (``DeformableDetrMultiscaleDeformableAttention``,
    ``GroundingDinoMultiscaleDeformableAttention``, the RT-DETR family's ...) by ``replace_hf_msda(model, fused=True)``:
    the module keeps its submodules, parameters and ``state_dict`` keys; its forward runs the softmax, the offset
    normalisation and the reference-point broadcast inside the gather kernels (:func:`fused_hf_module_core`).

    The softmaxed attention weights are never materialised, so the second element of the returned pair is ``None``.  A
    caller that records attentions sets ``module.return_attention_weights = True`` (or passes
    ``output_attentions=True``): the module then takes the original forward over the adapter's core.

    ``skip_padded_queries`` (set per module by ``replace_hf_msda(model, fused=True, skip_padded_queries=True)``; off by
    default): in an encoder layer — ``encoder_hidden_states is hidden_states``, so every pixel of the padded pyramid is
    also a query and the ``[B, I]`` ``attention_mask`` covers both roles — the mask also travels as ``query_mask``: a
    padded position is neither gathered for nor recorded for the pyramid's gradient.  Its attended row is then zeros, so
    the layer's output there is ``output_proj``'s BIAS, not the projection of whatever the padded position sampled.  Valid
    positions are unaffected, because every consumer masks the padded ones: the next layer and the decoder's
    cross-attention read them as values through the same mask (a row of zeros whatever they hold), and the two-stage
    proposals ``masked_fill`` them.  Taken only when all three hold: a mask was passed, the layer attends to its own
    hidden states (tested on the arguments, before the position embeddings are added), and the mask's shape is
    ``hidden_states.shape[:2]``.

    The one GEMM reads the two projection layers' ``.weight`` and ``.bias`` and never calls the layers, so it is taken only
    for plain, hook-free ``nn.Linear`` pairs (``_linear._plain_linear``).  A LoRA / PEFT wrapper, a subclass, a quantised
    replacement, a layer with hooks — and every traced call — has the two layers called as they are, and their outputs go
    to :func:`fused_hf_module_core_split`, whose kernels read offsets and logits where the layers left them."""

    return_attention_weights = False
    skip_padded_queries = False

    def _proj_rows(self, device) -> torch.Tensor:
        # row (h, l, p, k) of the one projection: k < 2 the offset rows of `sampling_offsets`, k == 2 the logit row of
        # `attention_weights` (behind them in the concatenation)
        idx = self.__dict__.get("_msda_proj_rows")
        if idx is None or idx.device != device:
            n = self.n_heads * self.n_levels * self.n_points
            s = torch.arange(n, device=device)
            idx = torch.stack([2 * s, 2 * s + 1, 2 * n + s], -1).reshape(-1)
            self.__dict__["_msda_proj_rows"] = idx  # (not a buffer: state_dict stays the HF module's)
        return idx

    def _plain_projections(self) -> bool:
        return not torch.compiler.is_compiling() and _plain_linear(self.sampling_offsets) and \
            _plain_linear(self.attention_weights)

    def _split_route(self, hidden_states, value, reference_points, shapes, level_shapes, mask_kw) -> torch.Tensor:
        """The core behind projection layers that must be CALLED: their outputs, as they are, to the split-projection
        kernels (masks compose there)."""
        offsets, logits = self.sampling_offsets(hidden_states), self.attention_weights(hidden_states)
        kw = dict(level_shapes=level_shapes, value_mask=mask_kw.get("value_mask"), query_mask=mask_kw.get("query_mask"),
                  split_in_kernels=split_in_kernels(value))
        if value.device.type == "cuda" and value.dtype in (torch.bfloat16, torch.float16) and offsets.dtype == value.dtype \
                and logits.dtype == value.dtype and reference_points.dtype == torch.float32:
            with torch.autocast("cuda", enabled=False):  # (the module-storage kernels, as the plain route below)
                return fused_hf_module_core_split(value, shapes, offsets, logits, reference_points, "zeros", False, **kw)
        if offsets.dtype != value.dtype:
            offsets = offsets.to(value.dtype)
        if logits.dtype != value.dtype:
            logits = logits.to(value.dtype)
        if reference_points.dtype != value.dtype:
            reference_points = reference_points.to(value.dtype)
        return fused_hf_module_core_split(value, shapes, offsets, logits, reference_points, "zeros", False, **kw)

    def forward(self, hidden_states, attention_mask=None, encoder_hidden_states=None, encoder_attention_mask=None,
                position_embeddings=None, reference_points=None, spatial_shapes=None, spatial_shapes_list=None,
                level_start_index=None, **kwargs):
        if self.return_attention_weights or kwargs.get("output_attentions"):
            return super().forward(hidden_states, attention_mask=attention_mask, encoder_hidden_states=encoder_hidden_states,
                                   encoder_attention_mask=encoder_attention_mask, position_embeddings=position_embeddings,
                                   reference_points=reference_points, spatial_shapes=spatial_shapes,
                                   spatial_shapes_list=spatial_shapes_list, level_start_index=level_start_index, **kwargs)
        self_attention = encoder_hidden_states is hidden_states  # (on the arguments: the sum below makes a new tensor)
        if position_embeddings is not None:
            hidden_states = hidden_states + position_embeddings
        batch_size, num_queries, _ = hidden_states.shape
        sequence_length = encoder_hidden_states.shape[1]
        # the padding mask travels to the core with the value pyramid (no masked_fill here): fused_hf_module_core applies it
        # inside the kernels where mask_in_kernels() says they are ahead, else as the masked_fill transformers runs
        value = self.value_proj(encoder_hidden_states)
        value = value.view(batch_size, sequence_length, self.n_heads, value.shape[-1] // self.n_heads)
        mask_kw = {}
        if attention_mask is not None:
            mask_kw = dict(value_mask=attention_mask, mask_in_kernels=mask_in_kernels(value, num_queries))
            if self.skip_padded_queries and self_attention and tuple(attention_mask.shape) == (batch_size, num_queries):
                mask_kw["query_mask"] = attention_mask  # every pixel is a query too: the mask covers both roles
        return self._attend(hidden_states, value, reference_points, spatial_shapes, spatial_shapes_list, mask_kw)

    def _attend(self, hidden_states, value, reference_points, spatial_shapes, spatial_shapes_list, mask_kw):
        """Projections, core and output projection: ``hidden_states`` with its position embeddings added, ``value``
        ``[B, I, H, D]`` unmasked, ``mask_kw`` the masks in the core's polarity (non-zero = real)."""
        batch_size, num_queries, _ = hidden_states.shape
        if not self._plain_projections():
            level_shapes = spatial_shapes_list if isinstance(spatial_shapes_list, (list, tuple)) else None
            shapes = spatial_shapes
            if not torch.is_tensor(shapes):
                shapes = _shapes_tensor(shapes if shapes is not None else spatial_shapes_list, value.device)
            out = self._split_route(hidden_states, value, reference_points, shapes, level_shapes, mask_kw)
            return self.output_proj(out.flatten(2)), None
        # ONE GEMM for offsets and logits, laid out [B, Q, H, L, P, 3]; the weight is gathered from the two HF parameters
        # (autograd routes its gradient back to them)
        rows = self._proj_rows(hidden_states.device)
        so, aw = self.sampling_offsets, self.attention_weights
        weight = torch.cat([so.weight, aw.weight], 0).index_select(0, rows)
        bias = torch.cat([so.bias, aw.bias], 0).index_select(0, rows) if so.bias is not None and aw.bias is not None else None
        proj = nn.functional.linear(hidden_states, weight, bias)
        if bias is None and (so.bias is not None or aw.bias is not None):
            raise ValueError("`sampling_offsets` and `attention_weights` should both have a bias or neither")
        proj = proj.view(batch_size, num_queries, self.n_heads, self.n_levels, self.n_points, 3)
        level_shapes = spatial_shapes_list if isinstance(spatial_shapes_list, (list, tuple)) else None
        shapes = spatial_shapes
        if not torch.is_tensor(shapes):
            shapes = _shapes_tensor(shapes if shapes is not None else spatial_shapes_list, value.device)
        if value.device.type == "cuda" and value.dtype in (torch.bfloat16, torch.float16) and proj.dtype == value.dtype \
                and reference_points.dtype == torch.float32:
            # what autocast hands the core: 16-bit value and projection next to fp32 reference points — the module-storage
            # kernels (fp32 arithmetic, 16-bit result), called outside autocast so that nothing is cast to fp32
            with torch.autocast("cuda", enabled=False):
                out = fused_hf_module_core(value, shapes, proj, reference_points, "zeros", False, level_shapes=level_shapes,
                                           **mask_kw)
        else:
            if proj.dtype != value.dtype:
                proj = proj.to(value.dtype)
            if reference_points.dtype != value.dtype:
                reference_points = reference_points.to(value.dtype)
            out = fused_hf_module_core(value, shapes, proj, reference_points, "zeros", False, level_shapes=level_shapes,
                                       **mask_kw)
        return self.output_proj(out.flatten(2)), None


_FUSED_CLASSES: dict = {}  # HF module class -> its fused subclass
_FUSED_ATTRS = ("sampling_offsets", "attention_weights", "value_proj", "output_proj", "n_heads", "n_levels", "n_points")


def _wrap_fused(module: nn.Module) -> bool:
    if isinstance(module, FusedHFDeformableAttention) or not all(hasattr(module, a) for a in _FUSED_ATTRS):
        return False
    attn = getattr(module, "attn", None)
    if not isinstance(attn, nn.Module) or type(attn).__name__ != "MultiScaleDeformableAttention":
        return False
    cls = type(module)
    fused = _FUSED_CLASSES.get(cls)
    if fused is None:
        fused = _FUSED_CLASSES[cls] = type("Fused" + cls.__name__, (FusedHFDeformableAttention, cls), {})
    module.__class__ = fused
    return True


_HIP_CORE = MultiScaleDeformableAttention()  # (parameter-free: the operator with "zeros" padding and the flatten behind it)


class HFPixelDecoderDeformableAttention:
    """Mixed into the class of a Mask2Former / OneFormer pixel-decoder attention module
    (``Mask2FormerPixelDecoderEncoderMultiscaleDeformableAttention``, ``OneFormerPixelDecoderEncoder...``) by
    ``replace_hf_msda(model)``.  Those modules carry the attributes of the Deformable-DETR ones and transformers'
    level-reference rule, but call a module-level function ``multi_scale_deformable_attention`` instead of an ``attn``
    child, take the level shapes as host numbers (``spatial_shapes_list``; older OneFormer: a ``spatial_shapes`` tensor)
    and an ``attention_mask`` of the INVERSE polarity: ``True`` marks padding.  This forward is transformers' own, line by
    line, with that function replaced by the HIP operator; ``state_dict`` keys are unchanged.  ``output_attentions=True``
    (or ``module.return_attention_weights = True``) takes the original forward."""

    return_attention_weights = False

    def _named_args(self, args, kwargs):
        # positional arguments behind `reference_points` follow the wrapped class's own order (Mask2Former's and OneFormer's differ)
        if args:
            names = type(self).__dict__.get("_msda_arg_names")
            if names is None:
                names = tuple(inspect.signature(self._msda_base.forward).parameters)[7:]
                type(self)._msda_arg_names = names
            kwargs.update(zip(names, args))
        return kwargs

    @staticmethod
    def _level_shapes(kwargs, device):
        shapes_list, shapes = kwargs.get("spatial_shapes_list"), kwargs.get("spatial_shapes")
        if shapes_list is None and not torch.is_tensor(shapes):
            shapes_list, shapes = shapes, None
        if torch.is_tensor(shapes):
            return shapes, None
        level_shapes = [(int(h), int(w)) for h, w in shapes_list]
        return _shapes_tensor(level_shapes, device), level_shapes

    def forward(self, hidden_states, attention_mask=None, encoder_hidden_states=None, encoder_attention_mask=None,
                position_embeddings=None, reference_points=None, *args, **kwargs):
        kwargs = self._named_args(args, kwargs)
        if self.return_attention_weights or kwargs.get("output_attentions"):
            return self._msda_base.forward(self, hidden_states, attention_mask, encoder_hidden_states, encoder_attention_mask,
                                           position_embeddings, reference_points, **kwargs)
        if position_embeddings is not None:
            hidden_states = hidden_states + position_embeddings
        batch_size, num_queries, _ = hidden_states.shape
        sequence_length = encoder_hidden_states.shape[1]
        value = self.value_proj(encoder_hidden_states)
        if attention_mask is not None:
            value = value.masked_fill(attention_mask[..., None], float(0))  # (True = padding)
        value = value.view(batch_size, sequence_length, self.n_heads, value.shape[-1] // self.n_heads)
        shapes, level_shapes = self._level_shapes(kwargs, value.device)
        sampling_offsets = self.sampling_offsets(hidden_states).view(
            batch_size, num_queries, self.n_heads, self.n_levels, self.n_points, 2)
        attention_weights = self.attention_weights(hidden_states).view(
            batch_size, num_queries, self.n_heads, self.n_levels * self.n_points)
        attention_weights = nn.functional.softmax(attention_weights, -1).view(
            batch_size, num_queries, self.n_heads, self.n_levels, self.n_points)
        if reference_points.shape[-1] == 2:
            offset_normalizer = torch.stack([shapes[..., 1], shapes[..., 0]], -1)
            sampling_locations = (reference_points[:, :, None, :, None, :]
                                  + sampling_offsets / offset_normalizer[None, None, None, :, None, :])
        elif reference_points.shape[-1] == 4:
            sampling_locations = (reference_points[:, :, None, :, None, :2]
                                  + sampling_offsets / self.n_points * reference_points[:, :, None, :, None, 2:] * 0.5)
        else:
            raise ValueError(f"Last dim of reference_points must be 2 or 4, but got {reference_points.shape[-1]}")
        output = _HIP_CORE(value, shapes, level_shapes, None, sampling_locations, attention_weights)
        return self.output_proj(output), attention_weights


class FusedHFPixelDecoderDeformableAttention(HFPixelDecoderDeformableAttention, FusedHFDeformableAttention):
    """The same modules under ``replace_hf_msda(model, fused=True)``: :class:`FusedHFDeformableAttention`'s forward — one
    GEMM for a plain ``nn.Linear`` pair, the split-projection kernels behind anything else — with the shapes tensor built
    from ``spatial_shapes_list`` and ``~attention_mask`` as ``value_mask`` (and, with ``skip_padded_queries`` in a
    self-attending layer, as ``query_mask``).  The second element of the returned pair is ``None``."""

    def forward(self, hidden_states, attention_mask=None, encoder_hidden_states=None, encoder_attention_mask=None,
                position_embeddings=None, reference_points=None, *args, **kwargs):
        kwargs = self._named_args(args, kwargs)
        if self.return_attention_weights or kwargs.get("output_attentions"):
            return self._msda_base.forward(self, hidden_states, attention_mask, encoder_hidden_states, encoder_attention_mask,
                                           position_embeddings, reference_points, **kwargs)
        self_attention = encoder_hidden_states is hidden_states  # (on the arguments: the sum below makes a new tensor)
        if position_embeddings is not None:
            hidden_states = hidden_states + position_embeddings
        batch_size, num_queries, _ = hidden_states.shape
        sequence_length = encoder_hidden_states.shape[1]
        value = self.value_proj(encoder_hidden_states)
        value = value.view(batch_size, sequence_length, self.n_heads, value.shape[-1] // self.n_heads)
        shapes, level_shapes = self._level_shapes(kwargs, value.device)
        mask_kw = {}
        if attention_mask is not None:
            real = ~attention_mask if attention_mask.dtype == torch.bool else attention_mask == 0
            mask_kw = dict(value_mask=real, mask_in_kernels=mask_in_kernels(value, num_queries))
            if self.skip_padded_queries and self_attention and tuple(attention_mask.shape) == (batch_size, num_queries):
                mask_kw["query_mask"] = real
        return self._attend(hidden_states, value, reference_points, shapes, level_shapes, mask_kw)


def _pixel_decoder_module(module: nn.Module) -> bool:
    """The seven attributes, no ``attn`` child, and a ``multi_scale_deformable_attention`` function in the class's module."""
    if isinstance(module, FusedHFDeformableAttention) or not all(hasattr(module, a) for a in _FUSED_ATTRS):
        return False
    if isinstance(getattr(module, "attn", None), nn.Module):
        return False
    home = sys.modules.get(getattr(type(module), "_msda_base", type(module)).__module__)
    return callable(getattr(home, "multi_scale_deformable_attention", None))


def _wrap_pixel_decoder(module: nn.Module, fused: bool) -> bool:
    """Swap the class of a Mask2Former / OneFormer pixel-decoder attention module (matched by names, as everything here)
    for its subclass with the HIP core — the fused one with ``fused``.  A module wrapped without ``fused`` before is
    upgraded by a later call with it; nothing else is wrapped twice."""
    if not _pixel_decoder_module(module):
        return False
    mixin = FusedHFPixelDecoderDeformableAttention if fused else HFPixelDecoderDeformableAttention
    if isinstance(module, HFPixelDecoderDeformableAttention) and not fused:
        return False
    cls = getattr(type(module), "_msda_base", type(module))
    key = (cls, mixin)
    sub = _FUSED_CLASSES.get(key)
    if sub is None:
        sub = _FUSED_CLASSES[key] = type(("Fused" if fused else "Hip") + cls.__name__, (mixin, cls), {"_msda_base": cls})
    module.__class__ = sub
    return True


def _first_attr(module, *names):
    for n in names:
        if hasattr(module, n):
            return getattr(module, n)
    return None


class FusedHFBoxDeformableAttention(FusedHFDeformableAttention):
    """The same mixin for the Hugging Face attention modules with a point count per level and the box rule
    (``DFineMultiscaleDeformableAttention``, ``Deimv2MultiscaleDeformableAttention``,
    ``RTDetrV2MultiscaleDeformableAttention``): softmax, ``offset * num_points_scale * ref_wh * offset_scale`` and the
    reference-point broadcast run inside the gather kernels (:func:`fused_hf_box_core`).  ``position_embeddings``,
    ``value_proj`` and ``output_proj`` are applied where the module has them (RT-DETRv2); D-FINE's and DEIMv2's value is
    ``encoder_hidden_states`` reshaped.

    The second element of the returned pair is ``None``.  The original forward (over the adapter's core, where the module
    carries one) runs when attention weights are asked for (``return_attention_weights`` / ``output_attentions=True``),
    for 2-d reference points, for a reference-point axis of length other than 1 and for ``method="discrete"`` — unless
    the module was wrapped FOR that method (``replace_hf_msda(model, fused=True, fuse_discrete=True)``): it then runs
    ``fused_hf_box_core(..., sampling_mode="discrete")``, and takes the ``sampling_offsets`` rows of its one GEMM from
    detached parameters, because transformers gives ``sampling_offsets`` no gradient in this mode (the pixel index is an
    integer): their ``.grad`` stays ``None`` and ``hidden_states`` receives exact zeros from those slots."""

    def _proj_rows(self, device) -> torch.Tensor:
        # row (h, s, k) of the one projection: k < 2 the offset rows of `sampling_offsets`, k == 2 the logit row of
        # `attention_weights` (behind them in the concatenation)
        idx = self.__dict__.get("_msda_proj_rows")
        if idx is None or idx.device != device:
            n = self.n_heads * sum(int(p) for p in _first_attr(self, "num_points_list", "n_points_list"))
            s = torch.arange(n, device=device)
            idx = torch.stack([2 * s, 2 * s + 1, 2 * n + s], -1).reshape(-1)
            self.__dict__["_msda_proj_rows"] = idx  # (not a buffer: state_dict stays the HF module's)
        return idx

    def forward(self, hidden_states, attention_mask=None, *args, **kwargs):
        if args:  # positional arguments follow the wrapped class's own order (D-FINE's and RT-DETRv2's differ)
            names = type(self).__dict__.get("_msda_arg_names")
            if names is None:
                names = tuple(inspect.signature(super(FusedHFDeformableAttention, self).forward).parameters)[2:]
                type(self)._msda_arg_names = names
            kwargs.update(zip(names, args))
        reference_points = kwargs.get("reference_points")
        method = _first_attr(self, "decoder_method", "method")
        discrete = method == "discrete" and self.__dict__.get("_msda_fused_discrete", False)
        if self.return_attention_weights or kwargs.get("output_attentions") or \
                (method != "default" and not discrete) or \
                not torch.is_tensor(reference_points) or reference_points.dim() != 4 or \
                reference_points.shape[2] != 1 or reference_points.shape[-1] != 4:
            return super(FusedHFDeformableAttention, self).forward(hidden_states, attention_mask, **kwargs)
        encoder_hidden_states = kwargs["encoder_hidden_states"]
        spatial_shapes, spatial_shapes_list = kwargs.get("spatial_shapes"), kwargs.get("spatial_shapes_list")
        position_embeddings = kwargs.get("position_embeddings")
        if position_embeddings is not None:
            hidden_states = hidden_states + position_embeddings
        batch_size, num_queries, _ = hidden_states.shape
        sequence_length = encoder_hidden_states.shape[1]
        value_proj, output_proj = getattr(self, "value_proj", None), getattr(self, "output_proj", None)
        value = value_proj(encoder_hidden_states) if value_proj is not None else encoder_hidden_states
        if attention_mask is not None and value_proj is not None:  # (RT-DETRv2 masks the rows, D-FINE the reshaped value)
            value = value.masked_fill(~attention_mask[..., None], float(0))
        value = value.reshape(batch_size, sequence_length, self.n_heads, value.shape[-1] // self.n_heads)
        if attention_mask is not None and value_proj is None:
            value = value.masked_fill(~attention_mask[..., None], float(0))
        # ONE GEMM for offsets and logits, laid out [B, Q, H, S, 3]; the weight is gathered from the two HF parameters
        # (autograd routes its gradient back to them)
        rows = self._proj_rows(hidden_states.device)
        so, aw = self.sampling_offsets, self.attention_weights
        if (so.bias is None) != (aw.bias is None):
            raise ValueError("`sampling_offsets` and `attention_weights` should both have a bias or neither")
        so_weight, so_bias = (so.weight.detach(), so.bias.detach() if so.bias is not None else None) if discrete \
            else (so.weight, so.bias)  # (discrete: no gradient reaches the offsets, so none is formed for their parameters)
        weight = torch.cat([so_weight, aw.weight], 0).index_select(0, rows)
        bias = torch.cat([so_bias, aw.bias], 0).index_select(0, rows) if so.bias is not None else None
        counts = [int(p) for p in _first_attr(self, "num_points_list", "n_points_list")]
        proj = nn.functional.linear(hidden_states, weight, bias).view(batch_size, num_queries, self.n_heads, sum(counts), 3)
        level_shapes = spatial_shapes_list if isinstance(spatial_shapes_list, (list, tuple)) else None
        shapes = spatial_shapes
        if not torch.is_tensor(shapes):
            shapes = _shapes_tensor(shapes if shapes is not None else spatial_shapes_list, value.device)
        offset_scale = float(self.offset_scale)
        mode = ("border", False, "discrete") if discrete else ("zeros", False, "bilinear")
        if value.device.type == "cuda" and value.dtype in (torch.bfloat16, torch.float16) and proj.dtype == value.dtype \
                and reference_points.dtype == torch.float32:
            # what autocast hands the core: 16-bit value and projection next to fp32 boxes — the module-storage kernels
            # (fp32 arithmetic, 16-bit result), called outside autocast so that nothing is cast to fp32
            with torch.autocast("cuda", enabled=False):
                out = fused_hf_box_core(value, shapes, proj, reference_points, counts, offset_scale, *mode[:2],
                                        level_shapes=level_shapes, sampling_mode=mode[2])
        else:
            if proj.dtype != value.dtype:
                proj = proj.to(value.dtype)
            if reference_points.dtype != value.dtype:
                reference_points = reference_points.to(value.dtype)
            out = fused_hf_box_core(value, shapes, proj, reference_points, counts, offset_scale, *mode[:2],
                                    level_shapes=level_shapes, sampling_mode=mode[2])
        out = out.flatten(2)
        return (output_proj(out) if output_proj is not None else out), None


_FUSED_BOX_ATTRS = ("sampling_offsets", "attention_weights", "n_heads", "offset_scale")


def _wrap_fused_box(module: nn.Module, discrete: bool = False) -> bool:
    """Wrap a module with per-level point counts and the box rule, matched by attribute names.  The scale buffer is
    compared ONCE, here, with float32(1 / P_l) repeated P_l times — a loaded checkpoint could carry other values, and the
    kernels take the scale from the counts.  ``discrete``: modules whose method is ``"discrete"`` are wrapped too."""
    if isinstance(module, FusedHFDeformableAttention) or not all(hasattr(module, a) for a in _FUSED_BOX_ATTRS):
        return False
    counts, scale = _first_attr(module, "num_points_list", "n_points_list"), _first_attr(module, "num_points_scale", "n_points_scale")
    method = _first_attr(module, "decoder_method", "method")
    if not isinstance(counts, (list, tuple)) or not torch.is_tensor(scale) or not isinstance(module.offset_scale, (int, float)) \
            or not (method == "default" or (discrete and method == "discrete")):
        return False
    counts = [int(p) for p in counts]
    if not counts or any(p < 1 for p in counts):
        return False
    expect = np.asarray([s for s, n in zip(hf_box_level_scale(counts), counts) for _ in range(n)], dtype=np.float32)
    have = scale.detach().to("cpu")  # (`.double()` widens the buffer, the values stay; a 16-bit model's rounded copy differs)
    if not have.is_floating_point() or tuple(have.shape) != expect.shape or \
            not np.array_equal(have.double().numpy(), expect.astype(np.float64)):
        return False
    so, aw = module.sampling_offsets, module.attention_weights
    n = int(module.n_heads) * sum(counts)
    if not isinstance(so, nn.Linear) or not isinstance(aw, nn.Linear) or so.out_features != 2 * n or aw.out_features != n:
        return False
    cls = type(module)
    fused = _FUSED_CLASSES.get(cls)
    if fused is None:
        fused = _FUSED_CLASSES[cls] = type("Fused" + cls.__name__, (FusedHFBoxDeformableAttention, cls), {})
    module.__class__ = fused
    if method == "discrete":
        module.__dict__["_msda_fused_discrete"] = True  # (an instance attribute: state_dict stays the HF module's)
    return True


def replace_hf_msda(model: nn.Module, discrete: bool = False, fused: bool = False, skip_padded_queries: bool = False,
                    fuse_discrete: bool = False) -> int:
    """Swap every HF ``MultiScaleDeformableAttention`` submodule of ``model`` for the adapter, and set
    :func:`ms_deformable_attn_core` on every module that carries an ``ms_deformable_attn_core`` attribute with
    ``decoder_method == "default"`` (D-FINE / DEIMv2; ``"discrete"`` modules are left alone).  With ``discrete=True``
    (opt-in) modules whose ``decoder_method`` is ``"discrete"`` are patched too, with
    :func:`ms_deformable_attn_core_v2`.  With ``fused=True`` (opt-in) every attention module that owns such a core as
    its child ``attn`` next to ``sampling_offsets``, ``attention_weights``, ``value_proj``, ``output_proj``, ``n_heads``,
    ``n_levels`` and ``n_points`` (Deformable-DETR, Grounding-DINO, the RT-DETR family; matched by these names, not by
    class) additionally becomes a :class:`FusedHFDeformableAttention`, and every module that has ``sampling_offsets``,
    ``attention_weights``, ``n_heads``, ``offset_scale``, a point list (``num_points_list`` / ``n_points_list``), a scale
    buffer (``num_points_scale`` / ``n_points_scale``) equal to ``float32(1 / P_l)`` repeated ``P_l`` times and method
    ``"default"`` (D-FINE, DEIMv2, RT-DETRv2; by these names as well) a :class:`FusedHFBoxDeformableAttention` — with
    ``fused=True, fuse_discrete=True`` (opt-in, no effect without ``fused=True``) also those whose method is
    ``"discrete"``, which then run the box rule's discrete kernels.  ``fused=True`` leaves them unwrapped, with or without
    ``discrete=True``, as it always did; ``discrete=True`` stays the switch for their cores, which a wrapped module still
    uses when it runs its original forward, so a discrete D-FINE model takes all three flags.  Returns
    the number of modules replaced, patched or wrapped: without ``fused`` exactly what it always returned, with it that
    number plus the modules wrapped (a D-FINE decoder layer then counts twice, once for its core and once for the
    wrapper).  ``skip_padded_queries=True`` (opt-in, no effect without ``fused=True``) sets
    :attr:`FusedHFDeformableAttention.skip_padded_queries` on every module wrapped as one: encoder layers then hand their
    padding mask to the core as ``query_mask`` too (see the class); the count is what it is without the flag.
    Mask2Former's and OneFormer's pixel-decoder attention modules — the seven attributes above, no ``attn`` child, a
    ``multi_scale_deformable_attention`` function in their class's module — have their class swapped for a subclass and are
    counted: :class:`HFPixelDecoderDeformableAttention` without ``fused``, :class:`FusedHFPixelDecoderDeformableAttention`
    with it (``skip_padded_queries`` applies to those as well)."""
    count = 0
    for parent in model.modules():
        for name, child in list(parent.named_children()):
            if type(child).__name__ == "MultiScaleDeformableAttention" and not isinstance(child, MultiScaleDeformableAttention):
                setattr(parent, name, MultiScaleDeformableAttention())
                count += 1
    for module in model.modules():
        if hasattr(module, "ms_deformable_attn_core") and getattr(module, "decoder_method", None) == "default" and \
                module.ms_deformable_attn_core is not ms_deformable_attn_core:
            module.ms_deformable_attn_core = ms_deformable_attn_core
            count += 1
        elif discrete and hasattr(module, "ms_deformable_attn_core") and \
                getattr(module, "decoder_method", None) == "discrete" and \
                module.ms_deformable_attn_core is not ms_deformable_attn_core_v2:
            module.ms_deformable_attn_core = ms_deformable_attn_core_v2
            count += 1
    for module in list(model.modules()):
        if _wrap_pixel_decoder(module, fused):  # (Mask2Former / OneFormer: no `attn` child to swap, the class carries the core)
            count += 1
    if fused:
        for module in list(model.modules()):
            if _wrap_fused(module) or _wrap_fused_box(module, fuse_discrete):
                count += 1
            if skip_padded_queries and isinstance(module, FusedHFDeformableAttention) and \
                    not isinstance(module, FusedHFBoxDeformableAttention):
                module.skip_padded_queries = True  # (an instance attribute: state_dict stays the HF module's)
    return count
