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

import torch
from torch import nn

from .functional import _autocast_on, multiscale_deformable_attention


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


def replace_hf_msda(model: nn.Module, discrete: bool = False) -> int:
    """Swap every HF ``MultiScaleDeformableAttention`` submodule of ``model`` for the adapter, and set
    :func:`ms_deformable_attn_core` on every module that carries an ``ms_deformable_attn_core`` attribute with
    ``decoder_method == "default"`` (D-FINE / DEIMv2; ``"discrete"`` modules are left alone).  With ``discrete=True``
    (opt-in) modules whose ``decoder_method`` is ``"discrete"`` are patched too, with
    :func:`ms_deformable_attn_core_v2`.  Returns the number of modules replaced or patched."""
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
    return count
