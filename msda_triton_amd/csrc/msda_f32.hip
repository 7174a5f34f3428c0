// msda_f32.hip — C-ABI entry points msda_fwd_f32 / msda_bwd_f32 (storage type float), and the size / support queries of
// every dtype (include/msda_hip.h): the templates they are made of are visible here.
#include "msda_launch.hpp"

MSDA_DEFINE_ENTRY_POINTS(f32, float)

namespace msda {

// the uniform queries' dimensions are given one by one, the per-level queries' last two come out of ragged_counts
static bool any_negative(int64_t B, int64_t I, int64_t H, int64_t D, int64_t Q, int64_t L = 0, int64_t P = 0)
{
    return B < 0 || I < 0 || H < 0 || D < 0 || Q < 0 || L < 0 || P < 0;
}
// passes over the batch a query sizes for: MSDA_WS_PASSES(n) in its flags, else option "ws_passes"
static int passes_of(int flags) { return ((flags >> 8) & 0xff) ? ((flags >> 8) & 0xff) : option_ws_passes(); }

// Size of the sorted pipeline's workspace (shared by every dtype: the accumulate type decides the record sizes).  d.S:
// samples per unit with per-level point counts, d.P their maximum; 0: L * P.
static int64_t sorted_ws_bytes(Dims d, int elem_size, bool records_in_grads, int value_elem_size, int passes)
{
    // dimensions the call itself refuses (MSDA_ERR_TOO_LARGE) have no workspace to size: 0, never a wrapped product
    if (elem_size <= 0 || common_limits_exceeded(d, elem_size)) return 0;
    // problems the single-launch kernel takes need no workspace at all
    if (elem_size == 8 ? small_path_chosen<double>(d) : small_path_chosen<float>(d)) return 0;
    // ... and so have shapes without a grad_value route (MSDA_ERR_UNSUPPORTED; msda_bwd_supported)
    if (!(elem_size == 8 ? sorted_fits<double>(d) : sorted_fits<float>(d))) return 0;
    // passes over the batch (MSDA_WS_PASSES): the workspace of ceil(B / passes) batch elements, used once per group
    int64_t B = d.B;
    if (passes > 1 && B > 1) B = (B + passes - 1) / passes;
    // records in the gradient buffers need every group's share of them 16-byte aligned (msda_launch.hpp)
    const bool rg = records_in_grads && records_fit_grads(d, B, (size_t)elem_size) && option_records_in_grads() != 0;
    // the larger of the 16-byte-vector and the scalar layout: which one a call takes depends on the alignment of its
    // grad_out / grad_value pointers (a slice of a shard's buffers can be misaligned), and a workspace that is too
    // small would be rejected (MSDA_ERR_BAD_ARG)
    const size_t acc = elem_size == 8 ? 8 : 4;
    const size_t vec = sorted_ws_layout(B, d.I, d.H, d.D, d.Q, d.L, samples(d), acc, (size_t)elem_size, true, rg, (size_t)value_elem_size).total;
    const size_t sca = sorted_ws_layout(B, d.I, d.H, d.D, d.Q, d.L, samples(d), acc, (size_t)elem_size, false, rg, (size_t)value_elem_size).total;
    return (int64_t)(vec > sca ? vec : sca);
}

// Size of a fused backward's workspace (grad_value != NULL): the derived sampling points + attention weights (3 elements
// per sample, rounded up to 256 bytes: msda_launch.hpp, fused_mat_bytes), then the sorted pipeline's own workspace.
static int64_t fused_ws_bytes(const Dims &d, int elem_size, int passes)
{
    // (a call of this size is refused)
    if (elem_size <= 0 || common_limits_exceeded(d, elem_size) || fused_limit_exceeded(d)) return 0;
    // the 16-bit operators park the derived points in float and run the float grad_value passes (msda_common.hpp, ParkType)
    if (elem_size == 2) elem_size = 4;
    if (common_limits_exceeded(d, elem_size)) return 0;
    return (int64_t)fused_mat_bytes(d.B, d.H, d.Q, samples(d), (size_t)elem_size) + sorted_ws_bytes(d, elem_size, false, 0, passes);
}

// can grad_value be produced for these sizes at all (include/msda_hip.h: msda_bwd_supported)
static int bwd_supported(const Dims &d, int elem_size)
{
    if (elem_size <= 0 || d.L > MSDA_MAX_LEVELS) return 0;
    if (d.B * d.Q * d.H * d.D == 0 || samples(d) == 0 || d.I == 0) return 1;  // all-zero gradients
    switch (elem_size) {
    case 8: return sorted_fits<double>(d) || small_fits<double>(d);
    case 2: return sorted_fits<_Float16>(d) || small_fits<_Float16>(d);
    default: return sorted_fits<float>(d) || small_fits<float>(d);
    }
}

// the dimensions of a per-level query (S = sum of points_per_level samples per unit, P their maximum); false: no such call
static bool ragged_dims(Dims &d, int64_t B, int64_t I, int64_t H, int64_t D, int64_t Q, int64_t L, const int32_t *ppl,
                        int64_t max_level_cells = 0)
{
    d = Dims{B, I, H, D, Q, L, 0, max_level_cells > 0 ? max_level_cells : 0};
    return !any_negative(B, I, H, D, Q) && ragged_counts(ppl, L, d.P, d.S) == 0;
}

}  // namespace msda

extern "C" int64_t msda_bwd_workspace_bytes(int64_t B, int64_t I, int64_t H, int64_t D, int64_t Q, int64_t L,
                                            int64_t P, int elem_size, int value_elem_size, int64_t max_level_cells,
                                            int flags)
{
    if (msda::any_negative(B, I, H, D, Q, L, P)) return 0;
    return msda::sorted_ws_bytes(msda::Dims{B, I, H, D, Q, L, P, max_level_cells > 0 ? max_level_cells : 0}, elem_size,
                                 (flags & MSDA_WS_RECORDS_IN_GRADS) != 0, value_elem_size > 0 ? value_elem_size : elem_size,
                                 msda::passes_of(flags));
}

extern "C" int64_t msda_bwd_fused_workspace_bytes(int64_t B, int64_t I, int64_t H, int64_t D, int64_t Q, int64_t L,
                                                  int64_t P, int elem_size, int value_elem_size, int64_t max_level_cells,
                                                  int flags)
{
    (void)value_elem_size;
    if (msda::any_negative(B, I, H, D, Q, L, P)) return 0;
    return msda::fused_ws_bytes(msda::Dims{B, I, H, D, Q, L, P, max_level_cells > 0 ? max_level_cells : 0}, elem_size,
                                msda::passes_of(flags));
}

extern "C" int msda_bwd_supported(int64_t B, int64_t I, int64_t H, int64_t D, int64_t Q, int64_t L, int64_t P, int elem_size)
{
    if (msda::any_negative(B, I, H, D, Q, L, P)) return 0;
    return msda::bwd_supported(msda::Dims{B, I, H, D, Q, L, P}, elem_size);
}

// largest L*P the fused-prologue kernels (msda_fwd_fused / msda_bwd_fused) take for this head dimension and
// element size: all records of a unit must sit in LDS at once (plan_gather); the 16-byte vector path and the
// backward's larger records give the smaller bound
extern "C" int64_t msda_fused_lp_limit(int64_t D, int elem_size)
{
    if (D <= 0 || elem_size <= 0) return 0;
    const size_t acc = elem_size == 8 ? 8 : 4;
    int64_t best = INT64_MAX;
    for (int vec : {16 / elem_size, 1}) {
        const int NU = msda::kBlock / msda::pick_group((int)((D + vec - 1) / vec));
        int sc;
        size_t lds;
        msda::plan_gather(NU, 1 << 22, acc, sc, lds, true);
        if (sc < best) best = sc;
    }
    return best;
}

// per-level point counts (include/msda_hip.h): the sizes above with S = sum of points_per_level samples per unit and P their
// maximum
extern "C" int64_t msda_bwd_ragged_workspace_bytes(int64_t B, int64_t I, int64_t H, int64_t D, int64_t Q, int64_t L,
                                                   const int32_t *points_per_level, int elem_size, int value_elem_size,
                                                   int64_t max_level_cells, int flags)
{
    msda::Dims d;
    if (!msda::ragged_dims(d, B, I, H, D, Q, L, points_per_level, max_level_cells)) return 0;
    return msda::sorted_ws_bytes(d, elem_size, (flags & MSDA_WS_RECORDS_IN_GRADS) != 0,
                                 value_elem_size > 0 ? value_elem_size : elem_size, msda::passes_of(flags));
}

extern "C" int64_t msda_bwd_fused_ragged_workspace_bytes(int64_t B, int64_t I, int64_t H, int64_t D, int64_t Q, int64_t L,
                                                         const int32_t *points_per_level, int elem_size, int value_elem_size,
                                                         int64_t max_level_cells, int flags)
{
    (void)value_elem_size;
    msda::Dims d;
    if (elem_size <= 0 || !msda::ragged_dims(d, B, I, H, D, Q, L, points_per_level, max_level_cells)) return 0;
    return msda::fused_ws_bytes(d, elem_size, msda::passes_of(flags));
}

extern "C" int msda_bwd_ragged_supported(int64_t B, int64_t I, int64_t H, int64_t D, int64_t Q, int64_t L,
                                         const int32_t *points_per_level, int elem_size)
{
    msda::Dims d;
    if (elem_size <= 0 || !msda::ragged_dims(d, B, I, H, D, Q, L, points_per_level)) return 0;
    return msda::bwd_supported(d, elem_size);
}

// discrete sampling (include/msda_hip.h): the same cell pipelines on one-corner records, which always stay in the workspace
extern "C" int64_t msda_bwd_discrete_workspace_bytes(int64_t B, int64_t I, int64_t H, int64_t D, int64_t Q, int64_t L,
                                                     const int32_t *points_per_level, int elem_size, int value_elem_size,
                                                     int64_t max_level_cells, int flags)
{
    // (0 where msda_bwd_discrete_supported says no: there is no grad_value call to size a workspace for)
    if (elem_size <= 0 || !msda_bwd_ragged_supported(B, I, H, D, Q, L, points_per_level, elem_size)) return 0;
    return msda_bwd_ragged_workspace_bytes(B, I, H, D, Q, L, points_per_level, elem_size, value_elem_size, max_level_cells,
                                           flags & ~MSDA_WS_RECORDS_IN_GRADS);
}

// the box rule in front of discrete sampling: the parked points and weights (3 elements per sample, float for the 16-bit
// operators), then the discrete pipeline's workspace; 0 where the call is refused or needs none
extern "C" int64_t msda_bwd_fused_hfbox_discrete_workspace_bytes(int64_t B, int64_t I, int64_t H, int64_t D, int64_t Q,
                                                                 int64_t L, const int32_t *points_per_level, int elem_size,
                                                                 int value_elem_size, int64_t max_level_cells, int flags)
{
    (void)value_elem_size;
    msda::Dims d;
    if (elem_size <= 0 || L > msda::kFusedRaggedMaxLevels || !msda::ragged_dims(d, B, I, H, D, Q, L, points_per_level, max_level_cells))
        return 0;
    if (msda::common_limits_exceeded(d, elem_size)) return 0;
    if (elem_size == 2) elem_size = 4;  // (ParkType: the float grad_value passes)
    if (msda::common_limits_exceeded(d, elem_size) || !msda::bwd_supported(d, elem_size)) return 0;
    return (int64_t)msda::fused_mat_bytes(d.B, d.H, d.Q, msda::samples(d), (size_t)elem_size) +
           msda::sorted_ws_bytes(d, elem_size, false, 0, msda::passes_of(flags));
}

// the reference module's rule in front of discrete sampling: the same buffers, so the same answer
extern "C" int64_t msda_bwd_fused_discrete_workspace_bytes(int64_t B, int64_t I, int64_t H, int64_t D, int64_t Q, int64_t L,
                                                           const int32_t *points_per_level, int elem_size,
                                                           int value_elem_size, int64_t max_level_cells, int flags)
{
    return msda_bwd_fused_hfbox_discrete_workspace_bytes(B, I, H, D, Q, L, points_per_level, elem_size, value_elem_size,
                                                         max_level_cells, flags);
}

extern "C" int msda_bwd_discrete_supported(int64_t B, int64_t I, int64_t H, int64_t D, int64_t Q, int64_t L,
                                           const int32_t *points_per_level, int elem_size)
{
    return msda_bwd_ragged_supported(B, I, H, D, Q, L, points_per_level, elem_size);
}
