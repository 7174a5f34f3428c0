/*
 * msda_hip.h — C ABI of libmsda_hip.so, the MI355X (gfx950) multi-scale deformable
 * attention kernels.  Plain pointers and sizes only: no torch / HIP types in the
 * signatures (the stream is passed as an opaque void* holding a hipStream_t).
 *
 * This is the drop-in boundary for the reference's L1 launcher pair (paths relative
 * to the reference checkout, rziga/msda-triton @ 2025-08-24):
 *
 *   msda_fwd_<dtype>  replaces  triton_multi_scale_deformable_attention_fwd
 *                                 src/msda_triton/kernels.py:351-379   (called from frontend.py:124-126)
 *   msda_bwd_<dtype>  replaces  triton_multi_scale_deformable_attention_bwd
 *                                 src/msda_triton/kernels.py:556-592   (called from frontend.py:139-141)
 *
 * Tensor conventions are the reference's (frontend.py:157-160, kernels.py:9-15); every
 * buffer is device memory, dense row-major, and is never modified unless it is an output:
 *
 *   value      [B, I, H, D]        packed pyramid, level l occupies pixels
 *                                  [start_l, start_l + h_l*w_l), row-major (y*w_l + x)
 *   shapes     [L, 2]  int64       (height, width) per level, on the device; the level
 *                                  start offsets are derived in-kernel (kernels.py:58-62)
 *   loc        [B, Q, H, L, P, 2]  (x, y) normalised to [0,1]
 *   attn       [B, Q, H, L, P]
 *   out        [B, Q, H, D]
 *   grad_out   [B, Q, H, D]
 *   grad_value / grad_loc / grad_attn   shaped like value / loc / attn
 *
 * <dtype> in {f32, f16, bf16, f64} is the storage type of every floating-point buffer
 * (one dtype per call, as in the reference).  Coordinates, bilinear weights and all
 * accumulation are float (double for f64); results are rounded once on store.
 *
 * padding_mode: MSDA_PADDING_BORDER | MSDA_PADDING_ZEROS   (frontend.py:150,161)
 * align_corners: 0 | 1                                      (frontend.py:151,162)
 *
 * Outputs are fully overwritten (no pre-zeroing required, no accumulation into them).
 * msda_bwd_*: grad_value may be NULL (that gradient is skipped), and grad_loc / grad_attn may
 * be NULL together (both skipped) — the autograd caller passes only what needs_input_grad asks.
 *
 * msda_fwd_fused_<dtype> is the forward of the reference's nn.Module core with its prologue fused in
 * (src/msda_triton/frontend.py:253-282): `proj` [B, Q, H, L, P, 3] is the raw query projection
 * (x offset, y offset, attention logit); `ref` [B, Q, ref_dim] the reference points, ref_dim 2 = (x, y),
 * 4 = (cx, cy, w, h).  The kernel takes the softmax over each (b, q, h)'s L*P logits and forms the
 * sampling points (ref + offset / img_shapes[l] — in the reference's (h, w) order — or
 * ref_xy + offset * ref_wh / (2 P)) in its prologue, so neither tensor is ever materialised.
 * Returns MSDA_ERR_UNSUPPORTED when L*P is too large for one pass (callers then use msda_fwd_<dtype>).
 *
 * msda_bwd_fused_<dtype> is its backward with the prologue's chain rule fused in (what autograd does for
 * frontend.py:253-282): from grad_out to grad_value [B, I, H, D] (may be NULL), grad_proj [B, Q, H, L, P, 3]
 * (offset gradients scaled back, softmax backward applied to the logits) and grad_ref_partial
 * [B, Q, H, ref_dim] — the per-head partial sums of the reference points' gradient, which the caller adds up
 * over H.  It needs msda_bwd_fused_workspace_bytes(...) of workspace when grad_value is wanted (the derived
 * sampling points / attention weights are parked there for the grad_value passes — in the arithmetic type, except
 * that the 16-bit operators (bf16, f16) park them in float32 and run the float32 grad_value passes on their 16-bit rows,
 * as the f32_s* suffixes do: grad_value is sampled where `out` and grad_proj are.  The fused workspace queries therefore
 * size an elem_size of 2 as 4, and such a backward with grad_value has the float32 size limits).  Same
 * MSDA_ERR_UNSUPPORTED rule as the fused forward (nothing is launched then).
 *
 * Backward workspace: grad_value is computed as a gather over a per-call inverted index (sample
 * records sorted by bilinear cell), which lives in caller-provided device memory so that the
 * library never allocates: pass `workspace` (256-byte aligned) of at least
 * msda_bwd_workspace_bytes(...) bytes; its contents are scratch and need no initialisation.
 * msda_bwd_workspace_bytes(...) is 0 for small problems (Grounding-DINO / Deformable-DETR decoder shapes): they take a
 * single-launch kernel that keeps its inverted index in LDS.  A larger problem without (enough) workspace is rejected
 * with MSDA_ERR_BAD_ARG when grad_value is wanted (grad_loc / grad_attn never need workspace).
 * Calls are asynchronous on `stream`; there is no host synchronisation and no allocation
 * inside, so a call sequence can be captured into a hipGraph.
 *
 * Return value: 0 on success; a negative MSDA_ERR_* for rejected arguments (nothing was
 * launched); a positive hipError_t if a launch failed.  msda_last_error() describes the
 * most recent failure on the calling thread.
 */
#ifndef MSDA_HIP_H
#define MSDA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSDA_ABI_VERSION 12

#if defined(__GNUC__)
#define MSDA_API __attribute__((visibility("default")))
#else
#define MSDA_API
#endif

#define MSDA_PADDING_BORDER 0
#define MSDA_PADDING_ZEROS 1

#define MSDA_MAX_LEVELS 32

#define MSDA_ERR_BAD_ARG (-1)      /* null pointer, negative size, unknown padding mode */
#define MSDA_ERR_TOO_MANY_LEVELS (-2) /* L > MSDA_MAX_LEVELS */
#define MSDA_ERR_TOO_LARGE (-3)    /* a per-batch-element extent does not fit the 32-bit plane offsets: I*H*D*sizeof, Q*H*D*sizeof or Q*H*L*P*2 >= 2^31, or I, Q >= 2^24 (sizeof: of the sampling / arithmetic type, 4 for every f32_* suffix; the full list: DESIGN.md 2, "Size limits") */
#define MSDA_ERR_MISALIGNED (-4)   /* a buffer is not aligned to its element size */
#define MSDA_ERR_UNSUPPORTED (-5)  /* valid arguments this entry point cannot serve (use the unfused call) */

/*
 * ONE forward and ONE backward entry point per storage type (since ABI 10; ABI 9 carried three generations of them).
 *
 * ABI 11 CHANGED THE ARGUMENT LISTS of these entry points and of msda_bwd_fused_workspace_bytes under their old names
 * (value_row_stride inserted in front of `workspace` / `stream`; a flags argument appended): a caller built against ABI
 * 10 still links and would pass its workspace pointer as a stride.  EVERY caller must check msda_abi_version() ==
 * MSDA_ABI_VERSION once after loading the library, before its first call (INTEGRATION.md shows it for ctypes and C).
 *
 * value_row_stride (ABI 11): bytes from one pixel's H rows of `value` to the next pixel's; 0 = dense (H * D * sizeof).
 * `value` is then addressed as value[b][i] at ((b * I + i) * value_row_stride) bytes, the head's row at h * D * sizeof
 * inside it; the last pixel needs only its H * D * sizeof bytes.  Must be a multiple of the element size (of 16 bytes for
 * the vector path: otherwise the scalar kernels run), >= H * D * sizeof, with I * value_row_stride < 2^31.  Why a caller
 * would pad: the gather kernels are bound by the vector L1, which picks one of its four tag RAMs from the low bits of a
 * row's 128-byte line index; rows exactly 1 024 bytes apart (H * D * sizeof = 1 KB: 8 heads x 32 channels x fp32) put
 * every row of one head on half of them, and that head's plane gathers ~20 % slower.  One extra 128-byte line per pixel
 * (1 152) makes every head cycle through all residues: forward -3.5 ... -8 %, sample gradients -10 % at B = 4 with 5 000
 * / 10 000 queries and at B = 8 with 900 (profiles/r06_row_stride_ab.txt; the whole training step -2.5 ... -5 %,
 * r06_padded_step_ab.txt; nothing at B = 4 with 1 000).  A caller that OWNS the layout — a module that writes the value projection itself — can do
 * that for free (GEMM output with a leading dimension of H * D + 32 floats); grad_value is always dense.  Results are
 * bit-identical to the dense layout.
 *
 * max_level_cells (backward): what the caller knows about the level sizes ON THE HOST.  `shapes` lives on the device, so
 * the library sizes the single-launch grad_value kernel's LDS cell table for the worst level `I` pixels can form,
 * (2 I + 2 L) cells — which rules that kernel out for the pyramids of real images (a 100 x 134 ... 13 x 17 pyramid:
 * 35.6 k cells by the bound, 13.6 k in its largest level) and sends decoder-sized calls on them to the sorted pipeline,
 * 1.4x slower there.  A caller that knows the level sizes (Hugging Face models carry `spatial_shapes_list`) passes the
 * bilinear cells of the largest level, max_l (h_l + 1) * (w_l + 1); 0 = unknown.  The workspace query takes the same
 * number.  A level larger than stated cannot be reported from the kernel: its grad_value rows come back NaN.
 */
#define MSDA_DECLARE(SUF)                                                                          \
    MSDA_API int msda_fwd_##SUF(const void *value, const int64_t *shapes, const void *loc,                  \
                       const void *attn, void *out, int64_t B, int64_t I, int64_t H, int64_t D,    \
                       int64_t Q, int64_t L, int64_t P, int padding_mode, int align_corners,       \
                       int64_t value_row_stride, void *stream);                                    \
    MSDA_API int msda_fwd_fused_##SUF(const void *value, const int64_t *shapes, const void *proj,           \
                       const void *ref, void *out, int64_t B, int64_t I, int64_t H, int64_t D,    \
                       int64_t Q, int64_t L, int64_t P, int ref_dim, int padding_mode,             \
                       int align_corners, int64_t value_row_stride, void *stream);                 \
    MSDA_API int msda_bwd_##SUF(const void *grad_out, const void *value, const int64_t *shapes,             \
                       const void *loc, const void *attn, void *grad_value, void *grad_loc,        \
                       void *grad_attn, int64_t B, int64_t I, int64_t H, int64_t D, int64_t Q,     \
                       int64_t L, int64_t P, int padding_mode, int align_corners,                  \
                       int64_t max_level_cells, int64_t value_row_stride, void *workspace,         \
                       int64_t workspace_bytes, void *stream);                                     \
    MSDA_API int msda_bwd_fused_##SUF(const void *grad_out, const void *value, const int64_t *shapes, \
                       const void *proj, const void *ref, void *grad_value, void *grad_proj,       \
                       void *grad_ref_partial, int64_t B, int64_t I, int64_t H, int64_t D,          \
                       int64_t Q, int64_t L, int64_t P, int ref_dim, int padding_mode,              \
                       int align_corners, int64_t max_level_cells, int64_t value_row_stride,        \
                       void *workspace, int64_t workspace_bytes, void *stream);                    \
    MSDA_API int msda_fwd_ragged_##SUF(const void *value, const int64_t *shapes, const void *loc,           \
                       const void *attn, void *out, int64_t B, int64_t I, int64_t H, int64_t D,    \
                       int64_t Q, int64_t L, const int32_t *points_per_level, int padding_mode,    \
                       int align_corners, int64_t value_row_stride, void *stream);                 \
    MSDA_API int msda_bwd_ragged_##SUF(const void *grad_out, const void *value, const int64_t *shapes,      \
                       const void *loc, const void *attn, void *grad_value, void *grad_loc,        \
                       void *grad_attn, int64_t B, int64_t I, int64_t H, int64_t D, int64_t Q,     \
                       int64_t L, const int32_t *points_per_level, int padding_mode,               \
                       int align_corners, int64_t max_level_cells, int64_t value_row_stride,       \
                       void *workspace, int64_t workspace_bytes, void *stream);                    \
    MSDA_API int msda_fwd_discrete_##SUF(const void *value, const int64_t *shapes, const void *loc,         \
                       const void *attn, void *out, int64_t B, int64_t I, int64_t H, int64_t D,    \
                       int64_t Q, int64_t L, const int32_t *points_per_level,                      \
                       int64_t value_row_stride, void *stream);                                    \
    MSDA_API int msda_bwd_discrete_##SUF(const void *grad_out, const void *value, const int64_t *shapes,    \
                       const void *loc, const void *attn, void *grad_value, void *grad_attn,       \
                       int64_t B, int64_t I, int64_t H, int64_t D, int64_t Q, int64_t L,           \
                       const int32_t *points_per_level, int64_t max_level_cells,                   \
                       int64_t value_row_stride, void *workspace, int64_t workspace_bytes,         \
                       void *stream);                                                              \
    MSDA_API int msda_fwd_fused_ragged_##SUF(const void *value, const int64_t *shapes, const void *proj,\
                       const void *ref, void *out, int64_t B, int64_t I, int64_t H, int64_t D,      \
                       int64_t Q, int64_t L, const int32_t *points_per_level, int ref_dim,          \
                       int padding_mode, int align_corners, int64_t value_row_stride, void *stream);\
    MSDA_API int msda_bwd_fused_ragged_##SUF(const void *grad_out, const void *value,               \
                       const int64_t *shapes, const void *proj, const void *ref, void *grad_value,  \
                       void *grad_proj, void *grad_ref_partial, int64_t B, int64_t I, int64_t H,    \
                       int64_t D, int64_t Q, int64_t L, const int32_t *points_per_level, int ref_dim,\
                       int padding_mode, int align_corners, int64_t max_level_cells,                \
                       int64_t value_row_stride, void *workspace, int64_t workspace_bytes, void *stream);\
    MSDA_API int msda_fwd_fused_levelref_##SUF(const void *value, const int64_t *shapes, const void *proj,\
                       const void *ref, void *out, int64_t B, int64_t I, int64_t H, int64_t D,      \
                       int64_t Q, int64_t L, int64_t P, int ref_dim, int padding_mode,              \
                       int align_corners, int64_t value_row_stride, void *stream);                  \
    MSDA_API int msda_bwd_fused_levelref_##SUF(const void *grad_out, const void *value,             \
                       const int64_t *shapes, const void *proj, const void *ref, void *grad_value,  \
                       void *grad_proj, void *grad_ref_partial, int64_t B, int64_t I, int64_t H,    \
                       int64_t D, int64_t Q, int64_t L, int64_t P, int ref_dim, int padding_mode,   \
                       int align_corners, int64_t max_level_cells, int64_t value_row_stride,        \
                       void *workspace, int64_t workspace_bytes, void *stream);\
    MSDA_API int msda_fwd_masked_##SUF(const void *value, const uint8_t *value_mask,                \
                       const int64_t *shapes, const void *loc, const void *attn, void *out,         \
                       int64_t B, int64_t I, int64_t H, int64_t D, int64_t Q, int64_t L, int64_t P, \
                       int padding_mode, int align_corners, int64_t value_row_stride, void *stream);\
    MSDA_API int msda_bwd_masked_##SUF(const void *grad_out, const void *value,                     \
                       const uint8_t *value_mask, const int64_t *shapes, const void *loc,           \
                       const void *attn, void *grad_value, void *grad_loc, void *grad_attn,         \
                       int64_t B, int64_t I, int64_t H, int64_t D, int64_t Q, int64_t L, int64_t P, \
                       int padding_mode, int align_corners, int64_t max_level_cells,                \
                       int64_t value_row_stride, void *workspace, int64_t workspace_bytes, void *stream);\
    MSDA_API int msda_fwd_fused_levelref_masked_##SUF(const void *value, const uint8_t *value_mask, \
                       const int64_t *shapes, const void *proj, const void *ref, void *out,         \
                       int64_t B, int64_t I, int64_t H, int64_t D, int64_t Q, int64_t L, int64_t P, \
                       int ref_dim, int padding_mode, int align_corners, int64_t value_row_stride,  \
                       void *stream);                                                               \
    MSDA_API int msda_bwd_fused_levelref_masked_##SUF(const void *grad_out, const void *value,      \
                       const uint8_t *value_mask, const int64_t *shapes, const void *proj,          \
                       const void *ref, void *grad_value, void *grad_proj, void *grad_ref_partial,  \
                       int64_t B, int64_t I, int64_t H, int64_t D, int64_t Q, int64_t L, int64_t P, \
                       int ref_dim, int padding_mode, int align_corners, int64_t max_level_cells,   \
                       int64_t value_row_stride, void *workspace, int64_t workspace_bytes, void *stream);\
    MSDA_API int msda_fwd_fused_hfbox_##SUF(const void *value, const int64_t *shapes, const void *proj,   \
                       const void *ref, void *out, int64_t B, int64_t I, int64_t H, int64_t D,      \
                       int64_t Q, int64_t L, const int32_t *points_per_level,                       \
                       const float *level_scale, double offset_scale, int ref_dim, int padding_mode,\
                       int align_corners, int64_t value_row_stride, void *stream);                  \
    MSDA_API int msda_bwd_fused_hfbox_##SUF(const void *grad_out, const void *value,                \
                       const int64_t *shapes, const void *proj, const void *ref, void *grad_value,  \
                       void *grad_proj, void *grad_ref_partial, int64_t B, int64_t I, int64_t H,    \
                       int64_t D, int64_t Q, int64_t L, const int32_t *points_per_level,            \
                       const float *level_scale, double offset_scale, int ref_dim, int padding_mode,\
                       int align_corners, int64_t max_level_cells, int64_t value_row_stride,        \
                       void *workspace, int64_t workspace_bytes, void *stream);

/*
 * Per-level point counts (ABI 12, additive): msda_fwd_ragged_<dtype> / msda_bwd_ragged_<dtype> take the arguments of
 * msda_fwd_<dtype> / msda_bwd_<dtype>, except that P becomes `points_per_level`, a HOST array of L counts P_l >= 1 (read
 * during the call, never kept; a count below 1 is MSDA_ERR_BAD_ARG).  With S = sum_l P_l the sample axis is level-major:
 *
 *   loc        [B, Q, H, S, 2]     samples [start_l, start_l + P_l) of a (b, q, h) belong to level l
 *   attn       [B, Q, H, S]        (grad_loc / grad_attn shaped alike)
 *
 * as the D-FINE / DEIMv2 decoders lay them out (decoder_n_points = [3, 6, 3] ...).  Every size check of the uniform
 * entry points applies with L * P read as S; value_row_stride, MSDA_WS_RECORDS_IN_GRADS and MSDA_WS_PASSES(n) mean what
 * they mean there, and the workspace comes from msda_bwd_ragged_workspace_bytes.  grad_value is bitwise reproducible
 * while max_l P_l <= 1024.
 *
 * The module's fused pair with per-level counts — ADDITIONS WITHIN ABI 12, probed by symbol like the discrete entry points
 * below: msda_fwd_fused_ragged_<suffix> / msda_bwd_fused_ragged_<suffix> take the arguments of msda_fwd_fused_<suffix> /
 * msda_bwd_fused_<suffix> with P replaced by `points_per_level`, for the same eight suffixes (f32, f16, bf16, f64,
 * f32_vbf16, f32_vf16, f32_sbf16, f32_sf16):
 *
 *   proj       [B, Q, H, S, 3]     (x offset, y offset, attention logit) per sample, level-major; grad_proj shaped alike
 *   weights    softmax of the logits over all S samples of a (b, q, h) unit
 *   ref_dim 2  point = ref + (ox / shapes[l][0], oy / shapes[l][1])             (the stored (h, w) order, as the uniform pair)
 *   ref_dim 4  point = ref_xy + (ox, oy) * ref_wh / (2 * P_l)                   with the count of the sample's OWN level
 *
 * (D-FINE's offset * num_points_scale * ref_wh * offset_scale with num_points_scale = 1 / P_l, offset_scale = 0.5).
 * grad_ref_partial is [B, Q, H, ref_dim] as there.  All S samples of a unit must fit one LDS pass (S <=
 * msda_fused_lp_limit(D, elem_size)) and L must be at most 8 (the fused kernels' level scan is bounded, to keep their
 * scalar registers out of scratch memory): otherwise MSDA_ERR_UNSUPPORTED and nothing is launched — compose the prologue
 * around msda_fwd_ragged_ / msda_bwd_ragged_<dtype> then.  value_row_stride,
 * max_level_cells and MSDA_WS_PASSES(n) mean what they mean in the uniform fused calls; the workspace comes from
 * msda_bwd_fused_ragged_workspace_bytes, and grad_value runs the ragged operator's pipelines (bitwise reproducible while
 * max_l P_l <= 1024).
 *
 * The module's fused pair for PER-LEVEL REFERENCE POINTS — ADDITIONS WITHIN ABI 12, probed by symbol:
 * msda_fwd_fused_levelref_<suffix> / msda_bwd_fused_levelref_<suffix>, the argument lists of msda_fwd_fused_<suffix> /
 * msda_bwd_fused_<suffix> for the same eight suffixes.  They are the prologue of Hugging Face transformers' attention
 * modules (Deformable-DETR, Grounding-DINO, the RT-DETR family), which differs from the reference module's in three ways:
 *
 *   ref        [B, Q, L, ref_dim]  a reference point per LEVEL (transformers multiplies them by each level's valid ratio)
 *   ref_dim 2  point = ref_l + (ox / w_l, oy / h_l)                 — (x, y) by (width, height), not the stored (h, w) order
 *   ref_dim 4  point = ref_l.xy + (ox, oy) / P * ref_l.wh * 0.5     — in this order, every operation rounded once
 *   grad_ref_partial  [B, Q, H, L, ref_dim]  a partial per head AND level; the caller sums over the heads
 *
 * The weights are the softmax over the L * P logits of a (b, q, h) unit, as in the uniform pair.  Uniform point count P
 * only.  The sampling point is formed by exactly the operations above (no fused multiply-add), so it is bit for bit what
 * the same expression gives on the host, and the copy parked for grad_value names the cell the forward sampled.  The limits
 * are the uniform pair's (L * P <= msda_fused_lp_limit(D, elem_size), else MSDA_ERR_UNSUPPORTED and nothing is launched;
 * every size guard of msda_fwd_fused_ / msda_bwd_fused_<suffix>).  grad_value IS the uniform pipeline on the derived points:
 * the workspace is the uniform pair's — msda_bwd_fused_workspace_bytes answers for these calls too, there is no query of
 * their own — and value_row_stride, max_level_cells and MSDA_WS_PASSES(n) mean what they mean there.
 *
 * The module's fused pair for HUGGING FACE'S BOX RULE WITH PER-LEVEL POINT COUNTS — ADDITIONS WITHIN ABI 12, probed by
 * symbol: msda_fwd_fused_hfbox_<suffix> / msda_bwd_fused_hfbox_<suffix> for the same eight suffixes, the argument lists
 * of msda_fwd_fused_ragged_<suffix> / msda_bwd_fused_ragged_<suffix> with two arguments behind `points_per_level`:
 *
 *   level_scale   HOST array of L floats: s_l, the scale of level l's offsets.  transformers' modules (D-FINE, DEIMv2,
 *                 RT-DETRv2) keep float32(1 / P_l) in an fp32 buffer; the caller passes those values
 *   offset_scale  the modules' offset_scale (a double; 0.5 in the default configurations)
 *   ref           [B, Q, 4] boxes (cx, cy, w, h); ref_dim must be 4, anything else is MSDA_ERR_BAD_ARG
 *   grad_ref_partial  [B, Q, H, 4], the caller sums over the heads
 *
 * The sampling point of an offset o of level l follows transformers' expression
 * `ref.xy + o * num_points_scale * ref.wh * offset_scale`, exactly these operations in this order, each rounded once
 * in the arithmetic type (fp32; fp64 for _f64), s_l and offset_scale first converted to that type:
 *
 *   q = o * s_l      t = q * wh      u = t * offset_scale      point = ref.xy + u     (no fused multiply-add)
 *
 * so the point is bit for bit the host expression's — in fp64 too, where s_l is float32(1 / P_l) widened and not
 * 1 / P_l — and the copy parked for grad_value (formed again from the parked q by the same operations) names the cell the
 * forward sampled.  The weights are the softmax over the unit's S logits.  Gradients: grad_o = gX * s_l * wh * offset_scale,
 * grad_wh = offset_scale * sum gX * q, grad_xy = sum gX.  Limits, size guards, value_row_stride, max_level_cells and
 * MSDA_WS_PASSES(n) are the fused per-level-count pair's (S <= msda_fused_lp_limit(D, elem_size) and L <= 8, else
 * MSDA_ERR_UNSUPPORTED and nothing is launched); grad_value IS that pair's pipeline on the derived points, and the workspace
 * is its workspace: msda_bwd_fused_ragged_workspace_bytes answers for these calls too.  Equal counts are served as any
 * others (the uniform pairs implement other rules).
 *
 * The VALUE PADDING MASK twins — ADDITIONS WITHIN ABI 12, probed by symbol: msda_fwd_masked_<dtype> / msda_bwd_masked_<dtype>
 * (the six suffixes of msda_fwd_<dtype>) and msda_fwd_fused_levelref_masked_<suffix> / msda_bwd_fused_levelref_masked_<suffix>
 * (the eight suffixes of the per-level-reference pair) take their twins' argument lists with one argument behind `value`:
 *
 *   value_mask   [B, I] bytes on the device, one per pixel of the pyramid: non-zero = the pixel is real, 0 = padding
 *                (transformers' attention_mask polarity; mmcv's key_padding_mask is the inverse)
 *
 * A padding pixel counts as a row of zeros WHATEVER BITS IT HOLDS — NaN and Inf there reach no output:
 *
 *   out, grad_loc, grad_attn (grad_proj, grad_ref_partial)   those of the twin on where(mask, value, 0), bit for bit
 *   grad_value                                                where(mask, the twin's grad_value, +0)
 *
 * The mask acts on the corner's address, never as a factor: in phase 1 of the forward and of the sample gradients a corner
 * whose pixel is padding takes the offset of a corner dropped by "zeros" padding and reads 0 without touching memory; the
 * grad_value finish pass (or the single-launch kernel's final store) stores a padding pixel's row as zeros, so neither
 * direction has a pass of its own over the pyramid.  The mask is read through a range-checked descriptor of I bytes per
 * batch element and takes no gradient.  A NULL value_mask is MSDA_ERR_BAD_ARG, refused before any other argument is looked
 * at: a caller without a mask calls the twin.  Size guards, limits, value_row_stride (the mask indexes PIXELS, not bytes),
 * max_level_cells, MSDA_WS_RECORDS_IN_GRADS and MSDA_WS_PASSES(n) are the twins', and so are the workspaces:
 * msda_bwd_workspace_bytes / msda_bwd_fused_workspace_bytes answer for these calls too.  The one-wave-per-unit forward is
 * never chosen for a masked call (msda_last_launch_info("fwd_variant") says 0 or 1).
 *
 * The QUERY PADDING MASK entry points — ADDITIONS WITHIN ABI 12, probed by symbol: msda_fwd_qmasked_<dtype> /
 * msda_bwd_qmasked_<dtype> (the six suffixes of the _masked_ pair) and msda_fwd_fused_levelref_qmasked_<suffix> /
 * msda_bwd_fused_levelref_qmasked_<suffix> (the eight of that pair) take the _masked_ twins' argument lists with one
 * argument behind `value_mask`, and run the twins' kernels:
 *
 *   query_mask   [B, Q] bytes on the device, one per query: non-zero = the query is real, 0 = padding
 *
 * BOTH masks are required — a NULL in either is MSDA_ERR_BAD_ARG before anything else is looked at; a caller without a
 * value mask passes all ones.  With plain(...) the _masked_ call on the same arguments:
 *
 *   real queries     their rows of out, grad_loc, grad_attn (grad_proj, grad_ref_partial) are plain's, bit for bit
 *   masked queries   those rows are zeros, every one of them written; their sampling inputs (points, weights, projection,
 *                    reference point, grad_out row) are never loaded, so NO BIT of them reaches any output
 *   grad_value       the sum over the real queries' samples only.  The count and place passes of the sorted pipeline and
 *                    the single-launch kernel's walks drop a masked query's samples where they drop a "zeros" sample
 *                    outside every cell; scan, gather and finish see shorter lists.  Against plain on sanitised inputs
 *                    (masked queries: points 0.5, weights / logits 0, grad_out row 0) it is equal on exactly representable
 *                    inputs only: removing records moves the gather's window cuts, and on general inputs the last bit can
 *                    differ (MSDA_WS_PASSES below has the same property).  It is bitwise reproducible under the conditions
 *                    that hold without the mask.
 *
 * The forward and the sample-gradient kernel look a wave's units up before phase 0; a call with a query mask gives up those
 * kernels' input prefetches (they would request a masked query's points).  Size guards, limits, workspaces,
 * msda_bwd_supported, MSDA_WS_RECORDS_IN_GRADS and MSDA_WS_PASSES(n) (the mask pointer advances with value_mask) are the
 * twins'.  The _masked_ entry points are these kernels with query_mask = NULL.
 *
 * Discrete (nearest-pixel) sampling — ADDITIONS WITHIN ABI 12: no existing signature changes and MSDA_ABI_VERSION stays
 * 12, so a caller PROBES FOR THESE BY SYMBOL (dlsym / hasattr) instead of by version; a library built before them simply
 * lacks them.  msda_fwd_discrete_<dtype> / msda_bwd_discrete_<dtype> take the ragged layout above (`points_per_level`,
 * loc [B, Q, H, S, 2], attn [B, Q, H, S]; the uniform layout is the same call with equal counts).  Every sample reads
 * exactly ONE value row:
 *
 *   ix = clamp(trunc(x * w + 0.5), 0, w - 1)      iy = clamp(trunc(y * h + 0.5), 0, h - 1)
 *   out[b, q, head, :] += attn * value[b, start_l + iy * w + ix, head, :]
 *
 * (transformers' multi_scale_deformable_attention_v2(method="discrete"); not grid_sample's "nearest").  The index is
 * computed in fp32 from the stored coordinate (fp64 for f64) as a rounded multiply followed by a rounded add — never a
 * fused multiply-add, so the pixel is the one the same expression picks on the host — and clamped in floating point
 * before the conversion: out-of-range and infinite coordinates take the edge pixel, NaN some in-range pixel.  There is
 * no padding_mode / align_corners argument (they have no meaning here) and no grad_loc (the sampling points get no
 * gradient).  msda_bwd_discrete_<dtype> writes grad_value [B, I, H, D] (dense) and grad_attn [B, Q, H, S]; EITHER MAY BE
 * NULL.  grad_value runs the bilinear call's cell pipelines on one-corner records (no floating-point atomics, bitwise
 * reproducible while max_l P_l <= 1024), so their limits carry over: msda_bwd_discrete_supported says whether it exists
 * for a shape (I < 2^22 ...), msda_bwd_discrete_workspace_bytes sizes its workspace (flags: 0 | MSDA_WS_PASSES(n);
 * MSDA_WS_RECORDS_IN_GRADS is ignored — there is no grad_loc buffer to lend).  Errors as everywhere: a null buffer or a
 * count below 1 is MSDA_ERR_BAD_ARG, L > MSDA_MAX_LEVELS is MSDA_ERR_TOO_MANY_LEVELS, and nothing is launched.
 */
MSDA_DECLARE(f32)
MSDA_DECLARE(f16)
MSDA_DECLARE(bf16)
MSDA_DECLARE(f64)
/* Mixed storage: `value` and `grad_value` are bf16 / fp16, every other tensor (sampling points, attention weights,
 * projection, reference points, out, grad_out and the other gradients) is fp32.  For modules that keep the value
 * pyramid in 16 bits (the value projection written straight in the kernel's layout and dtype) without
 * giving up fp32 sampling coordinates; arithmetic is fp32 as everywhere.  Same signatures; workspace sizes are those
 * of elem_size 4, value_elem_size 2. */
MSDA_DECLARE(f32_vbf16)
MSDA_DECLARE(f32_vf16)
#undef MSDA_DECLARE
/* Module storage (round 5; fused entry points only): `value`, `proj`, `out` and their gradients (grad_value, grad_proj,
 * grad_out) are bf16 / fp16, the reference points `ref` and `grad_ref_partial` fp32, all arithmetic fp32 — what the
 * reference's nn.Module computes under torch.autocast (its core casts every input to fp32, frontend.py:111) without the
 * fp32 copies of the projection and of the result and their gradients: a 16-bit projection holds exactly what autocast's
 * GEMM produced, while reference points in 16 bits would put the samples up to a quarter pixel off.  Same signatures as
 * msda_fwd_fused_<dtype> / msda_bwd_fused_<dtype>; workspace: msda_bwd_fused_workspace_bytes(..., elem_size 4,
 * value_elem_size 2, ...). */
#define MSDA_DECLARE_FUSED_STORAGE(SUF)                                                                \
    MSDA_API int msda_fwd_fused_##SUF(const void *value, const int64_t *shapes, const void *proj,      \
                       const void *ref, void *out, int64_t B, int64_t I, int64_t H, int64_t D,        \
                       int64_t Q, int64_t L, int64_t P, int ref_dim, int padding_mode,                 \
                       int align_corners, int64_t value_row_stride, void *stream);                     \
    MSDA_API int msda_bwd_fused_##SUF(const void *grad_out, const void *value, const int64_t *shapes, \
                       const void *proj, const void *ref, void *grad_value, void *grad_proj,           \
                       void *grad_ref_partial, int64_t B, int64_t I, int64_t H, int64_t D,              \
                       int64_t Q, int64_t L, int64_t P, int ref_dim, int padding_mode,                  \
                       int align_corners, int64_t max_level_cells, int64_t value_row_stride,            \
                       void *workspace, int64_t workspace_bytes, void *stream);                        \
    MSDA_API int msda_fwd_fused_ragged_##SUF(const void *value, const int64_t *shapes, const void *proj,\
                       const void *ref, void *out, int64_t B, int64_t I, int64_t H, int64_t D,      \
                       int64_t Q, int64_t L, const int32_t *points_per_level, int ref_dim,          \
                       int padding_mode, int align_corners, int64_t value_row_stride, void *stream);\
    MSDA_API int msda_bwd_fused_ragged_##SUF(const void *grad_out, const void *value,               \
                       const int64_t *shapes, const void *proj, const void *ref, void *grad_value,  \
                       void *grad_proj, void *grad_ref_partial, int64_t B, int64_t I, int64_t H,    \
                       int64_t D, int64_t Q, int64_t L, const int32_t *points_per_level, int ref_dim,\
                       int padding_mode, int align_corners, int64_t max_level_cells,                \
                       int64_t value_row_stride, void *workspace, int64_t workspace_bytes, void *stream);\
    MSDA_API int msda_fwd_fused_levelref_##SUF(const void *value, const int64_t *shapes, const void *proj,\
                       const void *ref, void *out, int64_t B, int64_t I, int64_t H, int64_t D,      \
                       int64_t Q, int64_t L, int64_t P, int ref_dim, int padding_mode,              \
                       int align_corners, int64_t value_row_stride, void *stream);                  \
    MSDA_API int msda_bwd_fused_levelref_##SUF(const void *grad_out, const void *value,             \
                       const int64_t *shapes, const void *proj, const void *ref, void *grad_value,  \
                       void *grad_proj, void *grad_ref_partial, int64_t B, int64_t I, int64_t H,    \
                       int64_t D, int64_t Q, int64_t L, int64_t P, int ref_dim, int padding_mode,   \
                       int align_corners, int64_t max_level_cells, int64_t value_row_stride,        \
                       void *workspace, int64_t workspace_bytes, void *stream);\
    MSDA_API int msda_fwd_fused_levelref_masked_##SUF(const void *value, const uint8_t *value_mask, \
                       const int64_t *shapes, const void *proj, const void *ref, void *out,         \
                       int64_t B, int64_t I, int64_t H, int64_t D, int64_t Q, int64_t L, int64_t P, \
                       int ref_dim, int padding_mode, int align_corners, int64_t value_row_stride,  \
                       void *stream);                                                               \
    MSDA_API int msda_bwd_fused_levelref_masked_##SUF(const void *grad_out, const void *value,      \
                       const uint8_t *value_mask, const int64_t *shapes, const void *proj,          \
                       const void *ref, void *grad_value, void *grad_proj, void *grad_ref_partial,  \
                       int64_t B, int64_t I, int64_t H, int64_t D, int64_t Q, int64_t L, int64_t P, \
                       int ref_dim, int padding_mode, int align_corners, int64_t max_level_cells,   \
                       int64_t value_row_stride, void *workspace, int64_t workspace_bytes, void *stream);\
    MSDA_API int msda_fwd_fused_hfbox_##SUF(const void *value, const int64_t *shapes, const void *proj,   \
                       const void *ref, void *out, int64_t B, int64_t I, int64_t H, int64_t D,      \
                       int64_t Q, int64_t L, const int32_t *points_per_level,                       \
                       const float *level_scale, double offset_scale, int ref_dim, int padding_mode,\
                       int align_corners, int64_t value_row_stride, void *stream);                  \
    MSDA_API int msda_bwd_fused_hfbox_##SUF(const void *grad_out, const void *value,                \
                       const int64_t *shapes, const void *proj, const void *ref, void *grad_value,  \
                       void *grad_proj, void *grad_ref_partial, int64_t B, int64_t I, int64_t H,    \
                       int64_t D, int64_t Q, int64_t L, const int32_t *points_per_level,            \
                       const float *level_scale, double offset_scale, int ref_dim, int padding_mode,\
                       int align_corners, int64_t max_level_cells, int64_t value_row_stride,        \
                       void *workspace, int64_t workspace_bytes, void *stream);
MSDA_DECLARE_FUSED_STORAGE(f32_sbf16)
MSDA_DECLARE_FUSED_STORAGE(f32_sf16)
#undef MSDA_DECLARE_FUSED_STORAGE

/* The query-mask entry points (see "QUERY PADDING MASK" above), declared by macros of their own: the six suffixes of
 * msda_fwd_masked_<dtype> for the plain pair, the eight of msda_fwd_fused_levelref_masked_<suffix> for the fused one. */
#define MSDA_QUERY_MASK_PLAIN(SUF)                                                                     \
    MSDA_API int msda_fwd_qmasked_##SUF(const void *value, const uint8_t *value_mask,               \
                       const uint8_t *query_mask, const int64_t *shapes, const void *loc,           \
                       const void *attn, void *out, int64_t B, int64_t I, int64_t H, int64_t D,     \
                       int64_t Q, int64_t L, int64_t P, int padding_mode, int align_corners,        \
                       int64_t value_row_stride, void *stream);                                     \
    MSDA_API int msda_bwd_qmasked_##SUF(const void *grad_out, const void *value,                    \
                       const uint8_t *value_mask, const uint8_t *query_mask, const int64_t *shapes, \
                       const void *loc, const void *attn, void *grad_value, void *grad_loc,         \
                       void *grad_attn, int64_t B, int64_t I, int64_t H, int64_t D, int64_t Q,      \
                       int64_t L, int64_t P, int padding_mode, int align_corners,                   \
                       int64_t max_level_cells, int64_t value_row_stride, void *workspace,          \
                       int64_t workspace_bytes, void *stream);
#define MSDA_QUERY_MASK_FUSED(SUF)                                                                     \
    MSDA_API int msda_fwd_fused_levelref_qmasked_##SUF(const void *value, const uint8_t *value_mask,\
                       const uint8_t *query_mask, const int64_t *shapes, const void *proj,          \
                       const void *ref, void *out, int64_t B, int64_t I, int64_t H, int64_t D,      \
                       int64_t Q, int64_t L, int64_t P, int ref_dim, int padding_mode,              \
                       int align_corners, int64_t value_row_stride, void *stream);                  \
    MSDA_API int msda_bwd_fused_levelref_qmasked_##SUF(const void *grad_out, const void *value,     \
                       const uint8_t *value_mask, const uint8_t *query_mask, const int64_t *shapes, \
                       const void *proj, const void *ref, void *grad_value, void *grad_proj,        \
                       void *grad_ref_partial, int64_t B, int64_t I, int64_t H, int64_t D,          \
                       int64_t Q, int64_t L, int64_t P, int ref_dim, int padding_mode,              \
                       int align_corners, int64_t max_level_cells, int64_t value_row_stride,        \
                       void *workspace, int64_t workspace_bytes, void *stream);
MSDA_QUERY_MASK_PLAIN(f32) MSDA_QUERY_MASK_PLAIN(f16) MSDA_QUERY_MASK_PLAIN(bf16) MSDA_QUERY_MASK_PLAIN(f64)
MSDA_QUERY_MASK_PLAIN(f32_vbf16) MSDA_QUERY_MASK_PLAIN(f32_vf16)
MSDA_QUERY_MASK_FUSED(f32) MSDA_QUERY_MASK_FUSED(f16) MSDA_QUERY_MASK_FUSED(bf16) MSDA_QUERY_MASK_FUSED(f64)
MSDA_QUERY_MASK_FUSED(f32_vbf16) MSDA_QUERY_MASK_FUSED(f32_vf16) MSDA_QUERY_MASK_FUSED(f32_sbf16) MSDA_QUERY_MASK_FUSED(f32_sf16)
#undef MSDA_QUERY_MASK_PLAIN
#undef MSDA_QUERY_MASK_FUSED

/*
 * Both padding masks inside the MODULE's own fused kernels — ADDITIONS WITHIN ABI 12, probed by symbol:
 * msda_fwd_fused_masked_<suffix> / msda_bwd_fused_masked_<suffix> (one reference point per query, uniform point count) and
 * msda_fwd_fused_ragged_masked_<suffix> / msda_bwd_fused_ragged_masked_<suffix> (per-level point counts), the eight suffixes
 * of the fused pairs.  Each list is its unmasked twin's (msda_*_fused_<suffix>, msda_*_fused_ragged_<suffix>) with two
 * arguments directly behind `value`:
 *
 *   value_mask   [B, I] bytes, non-zero = the pixel is real.  NULL is MSDA_ERR_BAD_ARG, refused before any other argument
 *                is looked at (a caller with a query mask only passes all ones)
 *   query_mask   [B, Q] bytes, non-zero = the query is real.  NULL = every query is real: the call keeps what a query mask
 *                costs it (below)
 *
 * The contracts are the ones stated above for the value mask (out, grad_proj, grad_ref_partial: the twin's on
 * where(mask, value, 0), bit for bit; grad_value: where(mask, the twin's, +0)) and for the query mask (real queries' rows
 * unchanged bit for bit, masked queries' rows of out / grad_proj / grad_ref_partial stored as zeros with no bit of their
 * inputs read, grad_value the sum over the real queries' samples).  The hooks are those of the per-level-reference pair:
 * mask_taps behind make_taps in phase 1, the per-slice ballot of live units before phase 0, the masked finish pass / the
 * single-launch kernel's zero rows and skipped walks, and — with a query mask only — the count and place passes on the
 * masked kernarg.  With a query mask the fused backward takes the 256-thread sample-gradient kernel (the 1024-thread one
 * with LDS-served levels has no room for the hook: "sample_variant" says 0); the forward may still serve levels from LDS.
 * The one-wave-per-unit forward is never chosen.  Size guards, alignment, ref_dim, msda_fused_lp_limit, L <= 8 for the
 * per-level pair (MSDA_ERR_UNSUPPORTED), their order of precedence and the workspaces are the twins':
 * msda_bwd_fused_workspace_bytes / msda_bwd_fused_ragged_workspace_bytes answer for these calls, MSDA_WS_PASSES(n) included
 * (both mask pointers advance with the batch groups).  Everything is answered before anything is launched.
 */
#define MSDA_MODULE_MASK(SUF)                                                                          \
    MSDA_API int msda_fwd_fused_masked_##SUF(const void *value, const uint8_t *value_mask,          \
                       const uint8_t *query_mask, const int64_t *shapes, const void *proj,          \
                       const void *ref, void *out, int64_t B, int64_t I, int64_t H, int64_t D,      \
                       int64_t Q, int64_t L, int64_t P, int ref_dim, int padding_mode,              \
                       int align_corners, int64_t value_row_stride, void *stream);                  \
    MSDA_API int msda_bwd_fused_masked_##SUF(const void *grad_out, const void *value,               \
                       const uint8_t *value_mask, const uint8_t *query_mask, const int64_t *shapes, \
                       const void *proj, const void *ref, void *grad_value, void *grad_proj,        \
                       void *grad_ref_partial, int64_t B, int64_t I, int64_t H, int64_t D,          \
                       int64_t Q, int64_t L, int64_t P, int ref_dim, int padding_mode,              \
                       int align_corners, int64_t max_level_cells, int64_t value_row_stride,        \
                       void *workspace, int64_t workspace_bytes, void *stream);                     \
    MSDA_API int msda_fwd_fused_ragged_masked_##SUF(const void *value, const uint8_t *value_mask,   \
                       const uint8_t *query_mask, const int64_t *shapes, const void *proj,          \
                       const void *ref, void *out, int64_t B, int64_t I, int64_t H, int64_t D,      \
                       int64_t Q, int64_t L, const int32_t *points_per_level, int ref_dim,          \
                       int padding_mode, int align_corners, int64_t value_row_stride, void *stream);\
    MSDA_API int msda_bwd_fused_ragged_masked_##SUF(const void *grad_out, const void *value,        \
                       const uint8_t *value_mask, const uint8_t *query_mask, const int64_t *shapes, \
                       const void *proj, const void *ref, void *grad_value, void *grad_proj,        \
                       void *grad_ref_partial, int64_t B, int64_t I, int64_t H, int64_t D,          \
                       int64_t Q, int64_t L, const int32_t *points_per_level, int ref_dim,          \
                       int padding_mode, int align_corners, int64_t max_level_cells,                \
                       int64_t value_row_stride, void *workspace, int64_t workspace_bytes, void *stream);
MSDA_MODULE_MASK(f32) MSDA_MODULE_MASK(f16) MSDA_MODULE_MASK(bf16) MSDA_MODULE_MASK(f64)
MSDA_MODULE_MASK(f32_vbf16) MSDA_MODULE_MASK(f32_vf16) MSDA_MODULE_MASK(f32_sbf16) MSDA_MODULE_MASK(f32_sf16)
#undef MSDA_MODULE_MASK

/*
 * Hugging Face's box rule in front of DISCRETE sampling (D-FINE / DEIMv2 / RT-DETRv2 with decoder_method = "discrete") —
 * ADDITIONS WITHIN ABI 12, probed by symbol: msda_fwd_fused_hfbox_discrete_<suffix> / msda_bwd_fused_hfbox_discrete_<suffix>
 * (the eight suffixes of the hfbox pair) and msda_bwd_fused_hfbox_discrete_workspace_bytes.  The argument lists are the
 * hfbox pair's WITHOUT ref_dim (boxes only: `ref` [B, Q, 4]), padding_mode, align_corners (discrete sampling has neither)
 * and grad_ref_partial (the pixel index is an integer: nothing differentiable reaches the point, hence nothing the box):
 *
 *   a_s   = softmax over the unit's S logits proj[..., 2]
 *   point = ref.xy + proj[..., :2] * level_scale[l] * ref.wh * offset_scale     four roundings, as the hfbox pair's
 *   out[b, q, head, :] = sum_s a_s * value[b, start_l + iy * w + ix, head, :]   the pixel rule of msda_fwd_discrete_<dtype>
 *
 * The point and the pixel are formed in fp32 from the stored values (fp64 for f64), never with a fused multiply-add, by
 * the very helpers of the two families this one joins, so for fp32 / fp64 inputs the pixel is the one transformers'
 * expressions pick on the same projection.  The ALL-16-BIT suffixes (f16, bf16) differ from transformers there: it forms
 * the point in 16 bits and can land on the neighbouring pixel; the kernel's point is the fp32 one.
 * msda_bwd_fused_hfbox_discrete_<suffix> writes EVERY element of grad_proj [B, Q, H, S, 3]: the two offset slots are stored
 * zeros, the logit slot is a_s (g_s - sum_t a_t g_t) with g_s = <the sample's row, the unit's grad_out row>.  grad_value
 * == NULL means a frozen pyramid: no workspace is needed and one kernel runs.  Otherwise the head of the workspace
 * receives the sampling points [B, Q, H, S, 2] and behind them the softmaxed weights [B, Q, H, S] (float for the 16-bit
 * operators, as the hfbox pair parks them), and msda_bwd_discrete_<dtype>'s grad_value pipeline runs on those two buffers —
 * its limits, reproducibility and MSDA_WS_PASSES(n) carry over; msda_bwd_fused_hfbox_discrete_workspace_bytes (the
 * arguments of msda_bwd_discrete_workspace_bytes) is the size, 0 where the call needs none or is refused.
 * L <= 8 (the scales ride in the kernel arguments): more is MSDA_ERR_UNSUPPORTED.  S = sum of points_per_level has NO limit
 * of its own beyond the common size guards (msda_fused_lp_limit does not apply: nothing per sample is held in LDS).  A
 * null level_scale is MSDA_ERR_BAD_ARG; a grad_value the pipeline cannot produce for the shape is MSDA_ERR_UNSUPPORTED and a
 * workspace that is too small MSDA_ERR_BAD_ARG; all of these are answered BEFORE anything is launched.
 * msda_last_launch_info: "fwd_variant" 4, "sample_variant" 3.
 */
#define MSDA_HFBOX_DISCRETE(SUF)                                                                       \
    MSDA_API int msda_fwd_fused_hfbox_discrete_##SUF(const void *value, const int64_t *shapes,      \
                       const void *proj, const void *ref, void *out, int64_t B, int64_t I,          \
                       int64_t H, int64_t D, int64_t Q, int64_t L, const int32_t *points_per_level, \
                       const float *level_scale, double offset_scale, int64_t value_row_stride,     \
                       void *stream);                                                               \
    MSDA_API int msda_bwd_fused_hfbox_discrete_##SUF(const void *grad_out, const void *value,       \
                       const int64_t *shapes, const void *proj, const void *ref, void *grad_value,  \
                       void *grad_proj, int64_t B, int64_t I, int64_t H, int64_t D, int64_t Q,      \
                       int64_t L, const int32_t *points_per_level, const float *level_scale,        \
                       double offset_scale, int64_t max_level_cells, int64_t value_row_stride,      \
                       void *workspace, int64_t workspace_bytes, void *stream);
#define MSDA_HFBOX_DISCRETE_QUERY(WHAT)                                                                \
    MSDA_API int64_t msda_bwd_fused_hfbox_discrete_##WHAT(int64_t B, int64_t I, int64_t H,          \
                       int64_t D, int64_t Q, int64_t L, const int32_t *points_per_level,            \
                       int elem_size, int value_elem_size, int64_t max_level_cells, int flags);
MSDA_HFBOX_DISCRETE(f32) MSDA_HFBOX_DISCRETE(f16) MSDA_HFBOX_DISCRETE(bf16) MSDA_HFBOX_DISCRETE(f64)
MSDA_HFBOX_DISCRETE(f32_vbf16) MSDA_HFBOX_DISCRETE(f32_vf16) MSDA_HFBOX_DISCRETE(f32_sbf16) MSDA_HFBOX_DISCRETE(f32_sf16)
MSDA_HFBOX_DISCRETE_QUERY(workspace_bytes)
#undef MSDA_HFBOX_DISCRETE
#undef MSDA_HFBOX_DISCRETE_QUERY

/*
 * The REFERENCE MODULE's rule in front of DISCRETE sampling (MultiscaleDeformableAttention(sampling_mode="discrete"),
 * functional.fused_module_core(..., sampling_mode="discrete")) — ADDITIONS WITHIN ABI 12, probed by symbol:
 * msda_fwd_fused_discrete_<suffix> / msda_bwd_fused_discrete_<suffix> (the same eight suffixes) and
 * msda_bwd_fused_discrete_workspace_bytes.  The argument lists are the hfbox-discrete pair's with `int ref_dim` in place of
 * `level_scale, offset_scale`; `proj` is [B, Q, H, S, 3] level-major (a uniform point count is the same call with equal
 * counts), `ref` [B, Q, ref_dim]:
 *
 *   a_s   = softmax over the unit's S logits proj[..., 2]
 *   point, ref_dim 2:  x = ref_x + ox / shapes[l][0]           y = ref_y + oy / shapes[l][1]     (the stored (h, w) order,
 *                                                                                                as msda_fwd_fused_<dtype>)
 *   point, ref_dim 4:  x = ref_x + ox * ref_w / (2 P_l)        y = ref_y + oy * ref_h / (2 P_l)  (P_l: the sample's level)
 *   out[b, q, head, :] = sum_s a_s * value[b, start_l + iy * w + ix, head, :]   the pixel rule of msda_fwd_discrete_<dtype>
 *
 * Every operation is rounded once in fp32 (fp64 for f64; the 16-bit operators form the point in fp32 from the stored
 * values): a multiply, a correctly rounded TRUE division — not a multiplication by a reciprocal —, an add, then the
 * discrete operator's multiply and add, none of them fused.  The kernel bodies, grad_proj (offset slots stored zeros, no
 * gradient for `ref`), the parked points and weights, the discrete grad_value pipeline behind them, the frozen-pyramid
 * call, the workspace (msda_bwd_fused_discrete_workspace_bytes answers what the hfbox-discrete query answers) and the
 * limits are the hfbox-discrete pair's: L <= 8 (more: MSDA_ERR_UNSUPPORTED), S unbounded.  ref_dim other than 2 / 4 is
 * MSDA_ERR_BAD_ARG.  Everything is answered BEFORE anything is launched.  No padding masks (the caller composes them).
 * msda_last_launch_info: "fwd_variant" 4, "sample_variant" 3 — the box-rule discrete pair's, the bodies are the same.
 */
#define MSDA_MODULE_DISCRETE(SUF)                                                                      \
    MSDA_API int msda_fwd_fused_discrete_##SUF(const void *value, const int64_t *shapes,            \
                       const void *proj, const void *ref, void *out, int64_t B, int64_t I,          \
                       int64_t H, int64_t D, int64_t Q, int64_t L, const int32_t *points_per_level, \
                       int ref_dim, int64_t value_row_stride, void *stream);                        \
    MSDA_API int msda_bwd_fused_discrete_##SUF(const void *grad_out, const void *value,             \
                       const int64_t *shapes, const void *proj, const void *ref, void *grad_value,  \
                       void *grad_proj, int64_t B, int64_t I, int64_t H, int64_t D, int64_t Q,      \
                       int64_t L, const int32_t *points_per_level, int ref_dim,                     \
                       int64_t max_level_cells, int64_t value_row_stride, void *workspace,          \
                       int64_t workspace_bytes, void *stream);
#define MSDA_MODULE_DISCRETE_QUERY(WHAT)                                                               \
    MSDA_API int64_t msda_bwd_fused_discrete_##WHAT(int64_t B, int64_t I, int64_t H, int64_t D,     \
                       int64_t Q, int64_t L, const int32_t *points_per_level, int elem_size,        \
                       int value_elem_size, int64_t max_level_cells, int flags);
MSDA_MODULE_DISCRETE(f32) MSDA_MODULE_DISCRETE(f16) MSDA_MODULE_DISCRETE(bf16) MSDA_MODULE_DISCRETE(f64)
MSDA_MODULE_DISCRETE(f32_vbf16) MSDA_MODULE_DISCRETE(f32_vf16) MSDA_MODULE_DISCRETE(f32_sbf16) MSDA_MODULE_DISCRETE(f32_sf16)
MSDA_MODULE_DISCRETE_QUERY(workspace_bytes)
#undef MSDA_MODULE_DISCRETE
#undef MSDA_MODULE_DISCRETE_QUERY

/*
 * The per-level-reference pair on SPLIT projections (functional.fused_hf_module_core_split; the Hugging Face adapter's
 * route for LoRA-wrapped, hooked or otherwise non-plain projection layers, and the tensors every module in the
 * ecosystem has) — ADDITIONS WITHIN ABI 12, probed by symbol: msda_fwd_fused_levelref_split_<suffix> /
 * msda_bwd_fused_levelref_split_<suffix> for the same eight suffixes.  The argument lists are
 * msda_fwd_fused_levelref_<suffix>'s / msda_bwd_fused_levelref_<suffix>'s with
 *
 *   offsets, logits            [B, Q, H, L, P, 2] (x offset, y offset) and [B, Q, H, L, P] in place of `proj` — what the
 *                              modules' two Linear layers produce, byte for byte the `loc` / `attn` layouts of msda_fwd_<dtype>
 *   grad_offsets, grad_logits  shaped alike, in place of `grad_proj`; every element of both is written
 *
 * Phase 0 reads (ox, oy) at 2 * s, 2 * s + 1 of `offsets` and the logit at s of `logits`; nothing behind those loads
 * differs from the interleaved pair — the arithmetic and its order, the parked points and weights, grad_value's pipeline,
 * the variants with LDS-served levels — so the results are BIT FOR BIT that pair's on the same numbers.  Every guard is that
 * pair's, in its order (sizes — the interleaved pair's 3 * Q * H * L * P bound included —, alignment to the element size,
 * ref_dim, L * P <= msda_fused_lp_limit(D, elem_size) else MSDA_ERR_UNSUPPORTED and nothing is launched); a NULL `offsets`
 * or `logits` (backward: `grad_offsets`, `grad_logits` too) is MSDA_ERR_BAD_ARG.  grad_ref_partial, the workspace,
 * MSDA_WS_PASSES(n), max_level_cells and value_row_stride are the pair's: msda_bwd_fused_workspace_bytes answers for these
 * calls too.  msda_last_launch_info reports the pair's variants; option "profile" names the launches
 * msda_fwd_fused_levelref_split / msda_bwd_fused_levelref_split.  No padding masks (the caller composes them).
 */
#define MSDA_LEVELREF_SPLIT(SUF)                                                                       \
    MSDA_API int msda_fwd_fused_levelref_split_##SUF(const void *value, const int64_t *shapes,      \
                       const void *offsets, const void *logits, const void *ref, void *out,         \
                       int64_t B, int64_t I, int64_t H, int64_t D, int64_t Q, int64_t L, int64_t P, \
                       int ref_dim, int padding_mode, int align_corners, int64_t value_row_stride,  \
                       void *stream);                                                               \
    MSDA_API int msda_bwd_fused_levelref_split_##SUF(const void *grad_out, const void *value,       \
                       const int64_t *shapes, const void *offsets, const void *logits,              \
                       const void *ref, void *grad_value, void *grad_offsets, void *grad_logits,    \
                       void *grad_ref_partial, int64_t B, int64_t I, int64_t H, int64_t D,          \
                       int64_t Q, int64_t L, int64_t P, int ref_dim, int padding_mode,              \
                       int align_corners, int64_t max_level_cells, int64_t value_row_stride,        \
                       void *workspace, int64_t workspace_bytes, void *stream);
MSDA_LEVELREF_SPLIT(f32) MSDA_LEVELREF_SPLIT(f16) MSDA_LEVELREF_SPLIT(bf16) MSDA_LEVELREF_SPLIT(f64)
MSDA_LEVELREF_SPLIT(f32_vbf16) MSDA_LEVELREF_SPLIT(f32_vf16) MSDA_LEVELREF_SPLIT(f32_sbf16) MSDA_LEVELREF_SPLIT(f32_sf16)
#undef MSDA_LEVELREF_SPLIT

/*
 * Bytes of device workspace msda_bwd_<dtype> wants for these sizes.  elem_size: of everything but `value`;
 * value_elem_size: of `value` / `grad_value` (0: the same — 2 next to elem_size 4 for the mixed-storage entry points);
 * max_level_cells: as for the call (0: unknown).
 * flags: MSDA_WS_RECORDS_IN_GRADS — the call will ALSO ask for grad_loc / grad_attn (all three gradient buffers
 * non-NULL and 16-byte aligned): the sorted sample records are dead once the gather has run, grad_loc / grad_attn are
 * written last and grad_value only by the finish kernel behind the gather, so the records of as many (batch, head)
 * planes as fit are kept in those buffers and the workspace shrinks (c2 @ 10k: 180 -> 98 MB).  A call with such a
 * workspace but without grad_loc / grad_attn (or misaligned buffers) is rejected (MSDA_ERR_BAD_ARG); a larger workspace
 * is fine.
 * Every workspace query answers 0 for sizes the call itself refuses with MSDA_ERR_TOO_LARGE and for sizes without a
 * grad_value route (msda_bwd_supported == 0): there is nothing to size, and no product of such sizes is formed.
 */
#define MSDA_WS_RECORDS_IN_GRADS 1
/*
 * MSDA_WS_PASSES(n), n = 2, 4, 8 ... (ABI 11): the size for n PASSES OVER THE BATCH.  The sorted pipeline's tables and partial
 * rows are per (batch, head) plane of the call; msda_bwd_<dtype> given a workspace that does not hold the whole batch but
 * does hold ceil(B / 2), ceil(B / 4) ... batch elements runs the pipeline once per such group in the same memory
 * (the workspace it is GIVEN decides: the fewest passes that fit).  c2 @ 10k fp32 with MSDA_WS_RECORDS_IN_GRADS:
 * 107 MB in one pass, 59 MB in two, 35 MB in four — the step's peak memory by the reference's recipe
 * (scripts/benchmark.py:158-172) 277 -> 229 -> 205 MB — for +16 % / +48 % of the step (0.307 -> 0.358 / 0.456 ms: the
 * pipeline's five kernels run at 68 % / 50 % of their rate on half / a quarter of the planes), which is why one pass is
 * the default.  grad_loc / grad_attn do not depend on the passes; grad_value is bitwise reproducible for a given number
 * of passes, and between two numbers of passes equal up to the rounding of the last bit (a group of fewer planes is cut
 * into more query slices, so a cell's records can sit in another order).
 */
#define MSDA_WS_PASSES(n) (((n) & 0xff) << 8)
MSDA_API int64_t msda_bwd_workspace_bytes(int64_t B, int64_t I, int64_t H, int64_t D, int64_t Q, int64_t L,
                                          int64_t P, int elem_size, int value_elem_size, int64_t max_level_cells,
                                          int flags);
/* ... msda_bwd_ragged_<dtype> (ABI 12; 0 for an unusable points_per_level) ... */
MSDA_API int64_t msda_bwd_ragged_workspace_bytes(int64_t B, int64_t I, int64_t H, int64_t D, int64_t Q, int64_t L,
                                                 const int32_t *points_per_level, int elem_size, int value_elem_size,
                                                 int64_t max_level_cells, int flags);
/* ... msda_bwd_discrete_<dtype> (within ABI 12, probe by symbol; flags: 0 | MSDA_WS_PASSES(n); 0 for an unusable
 * points_per_level and for every shape msda_bwd_discrete_supported answers 0 for) ... */
MSDA_API int64_t msda_bwd_discrete_workspace_bytes(int64_t B, int64_t I, int64_t H, int64_t D, int64_t Q, int64_t L,
                                                   const int32_t *points_per_level, int elem_size, int value_elem_size,
                                                   int64_t max_level_cells, int flags);
/* ... msda_bwd_fused_ragged_<suffix> (grad_value != NULL; within ABI 12, probe by symbol; flags: 0 | MSDA_WS_PASSES(n);
 * elem_size: of the arithmetic type — 4 for the f32_s* suffixes; 0 for an unusable points_per_level) ... */
MSDA_API int64_t msda_bwd_fused_ragged_workspace_bytes(int64_t B, int64_t I, int64_t H, int64_t D, int64_t Q, int64_t L,
                                                       const int32_t *points_per_level, int elem_size,
                                                       int value_elem_size, int64_t max_level_cells, int flags);
/* ... and msda_bwd_fused_<dtype> (grad_value != NULL). */
MSDA_API int64_t msda_bwd_fused_workspace_bytes(int64_t B, int64_t I, int64_t H, int64_t D, int64_t Q, int64_t L,
                                                int64_t P, int elem_size, int value_elem_size,
                                                int64_t max_level_cells, int flags /* 0 | MSDA_WS_PASSES(n) */);

/*
 * 1 when msda_bwd_<dtype> can produce grad_value for these sizes, 0 when it would return MSDA_ERR_UNSUPPORTED (a plane
 * of 2^22 pixels or more, or a head dimension beyond the 32-bit slot offsets of the sorted pipeline, on a problem that
 * is also too large for the single-launch kernel).  Host arithmetic only: a caller asks at FORWARD time when the value
 * pyramid requires a gradient, instead of learning it from the backward in the middle of a training step.
 */
MSDA_API int msda_bwd_supported(int64_t B, int64_t I, int64_t H, int64_t D, int64_t Q, int64_t L, int64_t P,
                                int elem_size);
/* ... for msda_bwd_ragged_<dtype> (ABI 12). */
MSDA_API int msda_bwd_ragged_supported(int64_t B, int64_t I, int64_t H, int64_t D, int64_t Q, int64_t L,
                                       const int32_t *points_per_level, int elem_size);
/* ... for msda_bwd_discrete_<dtype>'s grad_value (within ABI 12, probe by symbol). */
MSDA_API int msda_bwd_discrete_supported(int64_t B, int64_t I, int64_t H, int64_t D, int64_t Q, int64_t L,
                                         const int32_t *points_per_level, int elem_size);

/* Largest L*P the fused entry points accept for head dimension D and this element size (beyond it they return
 * MSDA_ERR_UNSUPPORTED and the caller composes the prologue around msda_fwd_/msda_bwd_<dtype>). */
MSDA_API int64_t msda_fused_lp_limit(int64_t D, int elem_size);

/* ABI version of the loaded library (== MSDA_ABI_VERSION it was built with). */
MSDA_API int msda_abi_version(void);

/* Human-readable description of the last non-zero return on this thread ("" if none). */
MSDA_API const char *msda_last_error(void);

/*
 * Kernel-variant switches for A/B measurements (bench.py, profiling, the option-variant test runs).  Not needed for
 * normal use: the defaults are the fastest measured variants.  Unknown keys return MSDA_ERR_BAD_ARG.  Keys:
 *   "xcd_map"    1 (default): blockIdx -> (batch, head) mapping keeps each (b,h) plane on one XCD's L2
 *                0: plain linear mapping   2: as 1 with the planes of an XCD rotated through the heads
 *   "linear_slots" 320 (default): launches over 128-byte rows 1 KB apart (H * D * sizeof = 1024: the layout with a slow
 *                   head) with at least this many workgroups per (batch, head) plane use the plain
 *                   linear block order instead of the XCD-aware one of "xcd_map" 1 (they walk the planes one after another
 *                   anyway, and all XCDs then share every plane's work: c5 step 11.2 -> 10.4 ms)
 *   "lds_levels" 1 (default): problems large enough to amortise it run the forward / sample-gradient kernels with the
 *                   coarsest pyramid levels served from LDS (1024-thread workgroups, one per CU: c2 @ 10k forward
 *                   99 -> 75 us) — fp32 arithmetic over fp32 or 16-bit rows, and the 16-bit operators' forward over
 *                   64-byte rows; bit-identical results;  0: never;  2: wherever the variant exists (tests)
 *   "lds_planes" 0 (default): the LDS-level forward kernels (and the module's fused backward) serve TWO planes — the
 *                   neighbouring heads (b, 2k), (b, 2k + 1) — per workgroup where both planes' levels fit and the
 *                   pairs' workgroups come out no heavier than single planes' would; its waves take slices of whichever plane has more left
 *                   (c2 @ 10k forward 69.5 -> 64.3 us; bit-identical results);  1: never;  2: whenever H is even (tests)
 *   "unit_fwd"   1 (default): forwards of at most 12 288 (b, q, h) units take the one-wave-per-unit kernel (decoder
 *                   calls: cold-cache forward at Q = 100 12.8 -> 9.3 us);  0: never;  2: wherever it exists (tests)
 *   "unit_waves" 1 (default): that kernel serves one unit per wave;  2: two (one per half wave) where its rows allow it:
 *                   ~1 us faster at Q = 200-300 with the pyramid in HBM, 0.3-0.6 us slower with it cached
 *   "touch"      1 (default): a forward of few queries that will read most of the pyramid anyway (4 Q L P >= 2 I, at most
 *                   65 536 (b, q, h) units, one round of workgroups with at most 768 rows of the plane each, not the
 *                   one-wave-per-unit kernel) has its workgroups request one dword of every row of their plane behind
 *                   their first sampling points, so that the rows stream into the XCD's L2 while the points are on their
 *                   way: with the pyramid in HBM (nothing in L2 or the Infinity Cache) forward at B = 4, H = 8, Q = 900
 *                   26.6 -> 22.7 us, Q = 2000 35.8 -> 32.9; nothing measurable when the rows are cached (larger shares
 *                   per workgroup do cost then: hence the 768); the values are not used, results are bit-identical;
 *                   0: never;  2: every forward through msda_fwd_kernel (tests)
 *   "value_path" 0 (default): grad_value by the single-launch LDS kernel when a (plane, level) fits one workgroup
 *                   (small problems; no workspace needed), else by the sorted gather in the caller's workspace
 *                2: the sorted gather always   3: the single-launch kernel whenever it fits
 *   "small_ns"   0 (default): workgroups per (plane, level) of the single-launch kernel chosen by the plane count; 1..16
 *   "q_round"    0 (default): queries per round of the sorted pipeline chosen by size; n: that many (tests)
 *   "overlap"    -1 (default) / 0: the backward's kernels run one after the other on the caller's stream;  1: grad_loc /
 *                   grad_attn run on a forked side stream next to grad_value (fork / join with events inside the call,
 *                   graph-capturable; costs ~14 us of host time and ~19 us of latency; does not pay since round 4)
 *   "place_path" 0 (default) / 2: the level-major place pass;  1: the plane-major one;  3: the level-major pass with
 *                   256-thread workgroups everywhere (measurement only)
 *   "strict"     0 (default);  1: a backward whose grad_value would NOT be bitwise reproducible is refused with
 *                   MSDA_ERR_UNSUPPORTED instead of run — see "Reproducibility" below
 *   "records_in_grads" 1 (default): msda_bwd_<dtype> with all three gradients keeps sorted records in the grad_loc /
 *                   grad_attn buffers until the sample-gradient kernel overwrites them;  0: never
 *   "profile"    0 (default);  1: event pairs around every kernel launch, read with msda_profile_read (measurement only)
 *   "level_cells" 0 (default): unknown;  n: process-wide form of the max_level_cells argument (an argument wins)
 *   "ws_passes"  1 (default): passes over the batch the workspace queries size for when their flags carry no MSDA_WS_PASSES(n)
 *                   (n: smaller workspace, the sorted pipeline runs once per group of ceil(B / n) batch elements — callers that
 *                   simply allocate what the query returns follow it without a change; see MSDA_WS_PASSES for the price)
 * Builds with -DMSDA_DEV (development only; the shipped library rejects these keys) add the experiment knobs
 * "cell_slices", "gather_win", "wg_target", "lds_budget", "lds_stagger", "lds_over" and the ablation / phase-clock mask "debug":
 * see msda_triton_amd/csrc/msda_launch.hpp, msda_value_sorted.hpp and tools/phase_clock.py.
 *
 * Reproducibility.  out, grad_loc and grad_attn are bitwise reproducible by construction (no atomics, fixed summation
 * orders).  grad_value is bitwise reproducible for P <= 1024 points per level: the gather sums a cell's records in list
 * order, and the place pass of the sorted pipeline and the single-launch kernel both let their waves take the
 * list-cursor atomics in TURNS (acquire / release on the turn word), so the list order is the same in every run.  This
 * rests on OBSERVED, not architected, behaviour of gfx950: lanes of ONE wave instruction that hit the same LDS word
 * with ds_add_rtn_u32 are served in a fixed order.  It holds in every run of the test suite (three dedicated tests,
 * all storage types, option variants) and of the fuzzers, and it is what the tests pin; a future part may differ.
 * P > 1024 points per level (and "place_path" 1) take the plane-major place pass, whose order follows free-running
 * atomics: grad_value may then differ in the last bit from run to run — or, with "strict" 1, the call is refused.
 */
MSDA_API int msda_set_option(const char *key, int value);
/* Measurement only.  With msda_set_option("profile", 1) every kernel the library launches is bracketed by a HIP event
 * pair on its stream; msda_profile_read waits for the events recorded (by any thread) since the last read and
 * writes one line per kernel — "name launches total_microseconds\n" — into buf (NUL-terminated, at most cap bytes);
 * returns the characters written.  The read consumes the records.  bench.py's per-kernel figures come from here. */
MSDA_API int msda_profile_read(char *buf, int cap);
MSDA_API int msda_get_option(const char *key);
/* Measurement only (ABI 11): which variants the most recent launches took (process-wide; bench.py reads it to say how many
 * of the forward's rows came from LDS).  Keys: "fwd_variant" 0 = 256-thread kernel, 1 = LDS-served coarse levels, 2 = one
 * wave per unit, 3 = the discrete-sampling forward (msda_fwd_discrete_<dtype>), 4 = the box rule's discrete forward
 * (msda_fwd_fused_hfbox_discrete_<suffix>; its backward kernel: "sample_variant" 3);  "fwd_lds_level_bytes" LDS bytes per plane set aside for level rows (the kernel keeps the longest suffix
 * of the level list that fits);  "fwd_lds_planes";  "fwd_workgroups";  "sample_variant", "sample_lds_level_bytes" the same
 * for the sample-gradient kernel (2 = the discrete attention-weight gradient);  "value_path" 1 = single-launch kernel, 2 = sorted pipeline;  "value_passes" its passes
 * over the batch.
 * WHICH TEMPLATE INSTANTIATION ran (last values too, added within ABI 12 — keys are looked up by name): "fwd_vec",
 * "fwd_group", "fwd_chunks" of the last forward launch (plain, LDS-served, one wave per unit — group = D / vec, one chunk —,
 * discrete, and the fused forwards);  "sample_vec", "sample_group", "sample_chunks" of the last sample-gradient launch
 * (discrete: the attention-weight gradient);  "value_vec", "value_group", "value_chunks" of the last grad_value launch (the
 * single-launch kernel, or the sorted pipeline's gather and finish passes).  vec: channels per lane — 16 bytes of the
 * arithmetic type, or 1 when D is no multiple of that or a row pointer is not 16-byte aligned;  group: lanes per (b, q, h)
 * unit, the smallest of 4, 8, 16, 32, 64 that holds ceil(D / vec) — 64 beyond;  chunks: ceil(D / (group * vec)) trips
 * of the kernels' channel loop.  0 before the first launch of that kind.
 * PASSES OVER A UNIT'S SAMPLES (last values, added within ABI 12): "fwd_trips" of the last forward launch and "sample_trips"
 * of the last sample-gradient launch — ceil(S / sc) for a unit of S samples (L * P, or the sum of points_per_level), sc being
 * the samples the kernel parks in LDS per trip (the 256-thread kernels: 48 KiB of records for the workgroup's 256 / group
 * units, less one; the LDS-served-level kernels: 72 KiB, or 100 KiB for the fused backward, for 1024 / group units, a
 * multi-trip sc rounded down to a multiple of group) or, in the one-wave-per-unit forward, the 64 / U samples a wave's
 * U units take per trip.  1 for the discrete kernels, which park nothing.
 * THE SORTED PIPELINE'S TABLES (last values, added within ABI 12 by name; all 0 after a single-launch grad_value):
 * "value_cell_cap" cells of the LDS table of the count pass (and of the plane-major place pass) — a plane with more cells is
 * walked in ceil(cells / value_cell_cap) trips, a plane's cells being sum_l (h_l + 1) * (w_l + 1);  "value_place_cells" cells of
 * the level-major place pass's table (a level with more cells takes several trips), 0 when the plane-major pass ran;
 * "value_place_variant" 0 = plane-major place pass, 1 = level-major with 1024 threads, 2 = level-major with 256 threads;
 * "value_slices" query slices per plane of the count and place passes;  "value_rounds" rounds over the queries;
 * "value_win" records per gather window.  With several passes over the batch: the last pass's values.
 * "grid_xcd3d_launches", "grid_linear2d_launches", "grid_flat_launches" are COUNTERS, not last values: launches so far in this
 * process whose (plane, slot) grid took the XCD-aware 3-D form dim3(8, slots, ceil(planes / 8)), the linear 2-D form
 * dim3(slots, planes), or the flat 1-D form that decodes its block index with a division (more than 65535 slots, plane
 * groups or — in linear order — planes).  They only rise (reported modulo 2^31); take the difference around a call.
 * Unknown key: MSDA_ERR_BAD_ARG. */
MSDA_API int msda_last_launch_info(const char *key);

#ifdef __cplusplus
}
#endif
#endif /* MSDA_HIP_H */
