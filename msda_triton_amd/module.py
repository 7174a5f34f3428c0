"""``MultiscaleDeformableAttention`` — the reference's nn.Module interface
(/root/reference/src/msda_triton/frontend.py:175-292) over the HIP operator.

Parameter names (``img_input_proj``, ``query_input_proj``, ``query_output_proj``) and shapes are
the reference's, so state dicts interchange.  The projections are ``nn.Linear`` layers (library
GEMMs; ``_linear.py`` only re-shapes their weight gradient for tall inputs); the deformable-attention core is custom.
"""
from __future__ import annotations

import numbers
from typing import Literal, Optional, Sequence, Union

import torch
from torch import nn

from ._linear import projection
from .discrete import SAMPLING_MODES, check_discrete_mode
from .functional import fused_module_core, module_sampling_inputs
from .ragged import ragged_module_sampling_inputs

# Both padding masks inside the fused kernels (msda_*_fused_masked_<dtype>, msda_*_fused_ragged_masked_<dtype>) instead of
# masked_fill / where passes around them.  The per-dtype default follows the project's rule: a storage
# dtype goes to the kernels only where the masked leg's slowest measured repeat was below the composition's fastest,
# forward plus backward (tools/module_mask_bench.py).  False: every call composes (A/B runs, and the parent's behaviour).
MASK_IN_KERNELS = True
MASK_IN_KERNELS_DTYPES = (torch.float32, torch.bfloat16)


# sampling_mode="discrete": softmax, point rule and pixel choice inside msda_*_fused_discrete_<dtype> instead of the
# prologue in PyTorch around the discrete operator.  The same rule per storage dtype of the value pyramid (DESIGN.md 21,
# tools/module_discrete_bench.py, profiles/r16_module_discrete_bench.json): fp32 and bf16 were measured and are ahead in
# every repeat, forward plus backward; fp16 and fp64 were not measured and compose.  False: every call composes.
DISCRETE_IN_KERNELS = True
DISCRETE_IN_KERNELS_DTYPES = (torch.float32, torch.bfloat16)


def mask_in_kernels(value: torch.Tensor) -> bool:
    """Does ``MultiscaleDeformableAttention.forward`` ask the core to take ``value_mask`` / ``query_mask`` into its fused
    kernels for this projected pyramid (``fused_module_core(mask_in_kernels=True)``), or compose them?  ``value`` is the
    pyramid as the kernels will read it — after the cast to the module's ``value_dtype``, so ``value_dtype=torch.float16``
    composes like every fp16 pyramid."""
    return bool(MASK_IN_KERNELS) and value.device.type == "cuda" and value.dtype in MASK_IN_KERNELS_DTYPES


class MultiscaleDeformableAttention(nn.Module):
    """Multiscale deformable attention with input/output projections (Deformable-DETR, fig. 2).

    Args:
        emb_dim: feature dimension of ``img`` and ``queries``.
        hidden_dim: projected feature dimension; must be divisible by ``num_heads``.
        num_levels: number of pyramid levels.
        num_heads: number of attention heads.
        num_points: sampling points per level; or (not in the reference) one count per level, e.g. ``[3, 6, 3]`` — the
            D-FINE / DEIMv2 / RT-DETRv2 layout: the query projection then holds ``sum(num_points)`` samples per head,
            level-major, the softmax runs over all of them and a 4-d reference box scales a sample's offset by
            ``1 / (2 * num_points[l])`` of its own level.  A list of equal counts is the same module as the ``int``
            (same parameters, same numbers).
        padding_mode: ``"border"`` or ``"zeros"``.
        align_corners: grid alignment.
        value_dtype: (not in the reference; GPU only) ``torch.bfloat16`` / ``torch.float16``: keep the projected value
            pyramid — the largest tensor the attention core reads, and the one autograd saves — in 16 bits, in the
            kernel's ``[B, I, H, D]`` layout, while sampling offsets, attention logits, reference points and the
            result stay fp32 (the kernels' mixed-storage entry points; arithmetic is fp32 either way).  Under
            ``torch.autocast`` to that dtype the projection GEMM writes it directly; otherwise its output is cast
            once.  ``None`` (default): the reference's behaviour — everything in the parameters' dtype, fp32 under
            autocast.
        sampling_mode: (not in the reference) ``"bilinear"`` (default) or ``"discrete"``: every sample reads its ONE
            nearest pixel (``msda_triton_amd.discrete``; what D-FINE / DEIMv2 / RT-DETRv2 decoders are deployed with).
            Needs ``padding_mode="border"``, ``align_corners=False``.  Same parameters and ``state_dict``; the sampling
            offsets and the reference points get no gradient in this mode.

    Raises:
        ValueError: if ``hidden_dim`` is not divisible by ``num_heads`` (frontend.py:211-212); for an unknown
            ``sampling_mode``, or ``"discrete"`` with another padding mode or ``align_corners``.
    """

    def __init__(self, emb_dim: int, hidden_dim: int, num_levels: int, num_heads: int,
                 num_points: Union[int, Sequence[int]], padding_mode: Literal["border", "zeros"], align_corners: bool,
                 value_dtype: Optional[torch.dtype] = None, sampling_mode: Literal["bilinear", "discrete"] = "bilinear"):
        super().__init__()
        if sampling_mode not in SAMPLING_MODES:
            raise ValueError(f"`sampling_mode` should be one of {list(SAMPLING_MODES)}, but got {sampling_mode!r}.")
        if sampling_mode == "discrete":
            check_discrete_mode(padding_mode, align_corners)
        self.sampling_mode = sampling_mode
        # `fuse_discrete` of the core: None = the measured per-dtype default above; True / False for A/B runs
        self.fuse_discrete = None
        if hidden_dim % num_heads != 0:
            raise ValueError(
                f"Hidden dimension ({hidden_dim=}) should be divisible by number of heads ({num_heads=}).")
        if value_dtype not in (None, torch.bfloat16, torch.float16):
            raise ValueError(f"`value_dtype` should be None, torch.bfloat16 or torch.float16, but got {value_dtype}.")
        # per-level point counts; None with an `int` (one count for every level: the reference's module, unchanged)
        self.points_per_level = None
        if not isinstance(num_points, numbers.Integral):
            counts = tuple(int(p) for p in num_points)
            if len(counts) != num_levels:
                raise ValueError(f"`num_points` has {len(counts)} entries, but the module has {num_levels=} levels.")
            if any(p < 1 for p in counts):
                raise ValueError(f"every entry of `num_points` should be at least 1, but got {list(counts)}.")
            if all(p == counts[0] for p in counts):
                num_points = counts[0]  # equal counts: the uniform module
            else:
                self.points_per_level = counts
        self.value_dtype = value_dtype
        self.num_levels = num_levels
        self.num_heads = num_heads
        self.num_points = num_points
        self.hidden_dim = hidden_dim
        self.padding_mode = padding_mode
        self.align_corners = align_corners
        # one fused query projection: (x offset, y offset, attention logit) per (head, level, point)
        self.img_input_proj = nn.Linear(emb_dim, hidden_dim)
        # (per-level counts: laid out [H, S, 3] with S = sum(num_points), samples level-major)
        samples = num_levels * num_points if self.points_per_level is None else sum(self.points_per_level)
        self.query_input_proj = nn.Linear(emb_dim, num_heads * samples * 3)
        self.query_output_proj = nn.Linear(hidden_dim, emb_dim)

    def sampling_inputs(self, img_shapes: torch.Tensor, queries: torch.Tensor, reference_points: torch.Tensor):
        """Query projection -> (sampling_points [B,N,H,L,P,2], attention_weights [B,N,H,L,P]); with per-level point
        counts ([B,N,H,S,2], [B,N,H,S]), level-major."""
        B, N, _ = queries.shape
        if self.points_per_level is not None:
            proj = self.query_input_proj(queries).reshape(B, N, self.num_heads, sum(self.points_per_level), 3)
            return ragged_module_sampling_inputs(proj, img_shapes, reference_points, self.points_per_level)
        proj = self.query_input_proj(queries).reshape(B, N, self.num_heads, self.num_levels, self.num_points, 3)
        return module_sampling_inputs(proj, img_shapes, reference_points)

    def forward(self, img: torch.Tensor, img_shapes: torch.Tensor, queries: torch.Tensor,
                reference_points: torch.Tensor, level_shapes=None, value_mask=None, query_mask=None) -> torch.Tensor:
        """
        Args:
            img: flattened pyramid ``[batch, num_image, emb_dim]``.
            img_shapes: ``[num_levels, 2]`` (height, width).
            queries: ``[batch, num_queries, emb_dim]``.
            reference_points: ``[batch, num_queries, 2]`` (x, y) or ``[batch, num_queries, 4]``
                (cx, cy, w, h), normalised to [0, 1].
            level_shapes: optional (not in the reference): the same (height, width) pairs as host numbers; see
                ``msda_triton_amd.functional.level_cells_of``.
            value_mask: optional (not in the reference): ``[batch, num_image]`` bool or uint8, non-zero = the pixel is
                real (transformers' ``attention_mask`` polarity): the projected pyramid counts as
                ``where(mask, value, 0)``.  On the GPU the mask goes into the fused kernels (``mask_in_kernels``); elsewhere
                it is applied as ``masked_fill``; see ``functional.fused_module_core``.
            query_mask: optional (not in the reference): ``[batch, num_queries]`` bool or uint8, non-zero = the query is
                real.  A masked query's attended row is zeros, so its row of the result is the output projection's bias,
                and nothing its projection or reference point holds reaches a gradient.  Handed to the core with
                ``value_mask`` (on the GPU the fused kernels skip the query; elsewhere ``functional.apply_query_mask``).

        Returns:
            ``[batch, num_queries, emb_dim]``.
        """
        B, I, _ = img.shape  # noqa: E741
        N = queries.shape[1]
        H, L, P = self.num_heads, self.num_levels, self.num_points
        if reference_points.shape[-1] not in (2, 4):
            raise ValueError(
                f"`reference_points` should have the last dim either 2 or 4, but got {reference_points.shape[-1]}.")
        # one projection holds (x offset, y offset, attention logit) per (head, level, point); on the GPU the softmax
        # and the offset -> sampling-point math run inside the attention kernel's prologue
        counts = self.points_per_level
        proj = projection(self.query_input_proj, queries)
        proj = proj.reshape(B, N, H, L, P, 3) if counts is None else proj.reshape(B, N, H, sum(counts), 3)
        # (the value pyramid is this module's own tensor: for large fp32 calls its pixels' rows are written one 128-byte line
        #  apart, which takes them off the vector L1's tag-RAM skew — functional.value_row_pad; the kernels read that layout
        #  in place.  Measured at the c2 module shape, fp32, tools/module_pad_ab.py: step 1.05 -> 1.02 ms at 10 000 queries,
        #  no gain at 2 500, and a LOSS at 900 — a host-bound step that the two extra small launches lengthen — so only
        #  from 32 768 (b, q) rows on)
        value = projection(self.img_input_proj, img, pad_rows=B * N >= 32768).reshape(B, I, H, self.hidden_dim // H)
        # both masks travel to the core, which takes them into its kernels or composes them (module-level MASK_IN_KERNELS,
        # decided on the dtype the kernels will read the pyramid in: below, after any cast to `value_dtype`)
        storage16 = value.device.type == "cuda" and proj.dtype in (torch.bfloat16, torch.float16) and \
            self.value_dtype in (None, proj.dtype) and value.dtype == proj.dtype
        if not storage16 and self.value_dtype is not None and value.device.type == "cuda":
            value = value.to(self.value_dtype)  # nothing to do when autocast already produced this dtype
        masks = dict(value_mask=value_mask, query_mask=query_mask, mask_in_kernels=mask_in_kernels(value),
                     sampling_mode=self.sampling_mode, fuse_discrete=self.fuse_discrete)
        if storage16:
            # 16-bit projections (autocast's GEMMs, or 16-bit parameters) with fp32 reference points: the kernels read
            # and write the 16-bit tensors as they are and compute in fp32 — what the reference's core does under
            # autocast (it casts every input to fp32, frontend.py:111) without the fp32 copies of value, projection,
            # result and their gradients; rounding happens at the same places (the GEMMs' outputs / inputs)
            with torch.autocast("cuda", enabled=False):
                attended = fused_module_core(value, img_shapes, proj, reference_points.float(), self.padding_mode,
                                             self.align_corners, level_shapes, counts, **masks)
        elif self.value_dtype is not None and value.device.type == "cuda":
            # 16-bit value pyramid next to fp32 sampling inputs: the mixed-storage kernels read it as it is (no fp32
            # copy, which is what autocast's cast_inputs would make), so the call sits outside autocast
            # (cast above, in front of the masks' routing decision)
            with torch.autocast("cuda", enabled=False):
                attended = fused_module_core(value, img_shapes, proj.float(), reference_points.float(),
                                             self.padding_mode, self.align_corners, level_shapes, counts,
                                             **masks).to(proj.dtype)
        else:
            attended = fused_module_core(value, img_shapes, proj, reference_points, self.padding_mode,
                                         self.align_corners, level_shapes, counts, **masks)
        return projection(self.query_output_proj, attended.reshape(B, N, self.hidden_dim))
