// msda_f32.hip — C-ABI entry points msda_fwd_f32 / msda_bwd_f32 (storage type float).
#include "msda_launch.hpp"

MSDA_DEFINE_ENTRY_POINTS(f32, float)

// size of the backward workspace (shared by every dtype: the accumulate type decides the record sizes)
extern "C" __attribute__((visibility("hidden"))) int64_t msda_bwd_workspace_bytes_impl(
    int64_t B, int64_t I, int64_t H, int64_t D, int64_t Q, int64_t L, int64_t P, int elem_size, int records_in_grads,
    int value_elem_size, int64_t max_level_cells, int passes, int64_t S)
{
    // problems the single-launch kernel takes need no workspace at all (S: samples per unit with per-level point counts,
    // P their maximum; 0: L * P)
    msda::Dims d{B, I, H, D, Q, L, P, max_level_cells > 0 ? max_level_cells : 0};
    d.S = S;
    // dimensions the call itself refuses (MSDA_ERR_TOO_LARGE) have no workspace to size: 0, never a wrapped product
    if (elem_size <= 0 || msda::common_limits_exceeded(d, elem_size)) return 0;
    const bool small = elem_size == 8 ? msda::small_path_chosen<double>(d) : msda::small_path_chosen<float>(d);
    const size_t acc = elem_size == 8 ? 8 : 4;
    if (small) return 0;
    // ... and so have shapes without a grad_value route (MSDA_ERR_UNSUPPORTED; msda_bwd_supported)
    if (!(elem_size == 8 ? msda::sorted_fits<double>(d) : msda::sorted_fits<float>(d))) return 0;
    // passes over the batch (MSDA_WS_PASSES): the workspace of ceil(B / passes) batch elements, used once per group
    if (passes > 1 && B > 1) B = (B + passes - 1) / passes;
    // records in the gradient buffers need every group's share of them 16-byte aligned (msda_launch.hpp)
    if (!msda::records_fit_grads(d, B, (size_t)elem_size)) records_in_grads = 0;
    // the larger of the 16-byte-vector and the scalar layout: which one a call takes depends on the alignment of its
    // grad_out / grad_value pointers (a slice of a shard's buffers can be misaligned), and a workspace that is too
    // small would be rejected (MSDA_ERR_BAD_ARG)
    const bool rg = records_in_grads != 0 && msda::option_records_in_grads() != 0;
    const size_t vec = msda::sorted_ws_layout(B, I, H, D, Q, L, msda::samples(d), acc, (size_t)elem_size, true, rg, (size_t)value_elem_size).total;
    const size_t sca = msda::sorted_ws_layout(B, I, H, D, Q, L, msda::samples(d), acc, (size_t)elem_size, false, rg, (size_t)value_elem_size).total;
    return (int64_t)(vec > sca ? vec : sca);
}

// would a fused call with these sizes be refused for its size (the fused workspace queries then answer 0)
extern "C" __attribute__((visibility("hidden"))) int msda_fused_dims_refused_impl(int64_t B, int64_t I, int64_t H, int64_t D,
                                                                                int64_t Q, int64_t L, int64_t P, int elem_size, int64_t S)
{
    msda::Dims d{B, I, H, D, Q, L, P};
    d.S = S;
    return elem_size <= 0 || msda::common_limits_exceeded(d, elem_size) || msda::fused_limit_exceeded(d);
}

// can grad_value be produced for these sizes at all (include/msda_hip.h: msda_bwd_supported)
extern "C" __attribute__((visibility("hidden"))) int msda_bwd_supported_impl(int64_t B, int64_t I, int64_t H, int64_t D,
                                                                           int64_t Q, int64_t L, int64_t P, int elem_size, int64_t S)
{
    msda::Dims d{B, I, H, D, Q, L, P};
    d.S = S;
    if (L > MSDA_MAX_LEVELS) return 0;
    if (B * Q * H * D == 0 || msda::samples(d) == 0 || I == 0) return 1;  // all-zero gradients
    switch (elem_size) {
    case 8: return msda::sorted_fits<double>(d) || msda::small_fits<double>(d);
    case 2: return msda::sorted_fits<_Float16>(d) || msda::small_fits<_Float16>(d);
    default: return msda::sorted_fits<float>(d) || msda::small_fits<float>(d);
    }
}

// largest L*P the fused-prologue kernels (msda_fwd_fused / msda_bwd_fused) take for this head dimension and
// element size: all records of a unit must sit in LDS at once (plan_gather); the 16-byte vector path and the
// backward's larger records give the smaller bound
extern "C" __attribute__((visibility("hidden"))) int64_t msda_fused_lp_limit_impl(int64_t D, int elem_size)
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

namespace msda {
int option_ws_passes();
}

// per-level point counts (include/msda_hip.h): the sizes above with S = sum of points_per_level samples per unit and P their
// maximum
extern "C" int64_t msda_bwd_ragged_workspace_bytes(int64_t B, int64_t I, int64_t H, int64_t D, int64_t Q, int64_t L,
                                                   const int32_t *points_per_level, int elem_size, int value_elem_size,
                                                   int64_t max_level_cells, int flags)
{
    int64_t pmax, S;
    if (B < 0 || I < 0 || H < 0 || D < 0 || Q < 0 || msda::ragged_counts(points_per_level, L, pmax, S) != 0) return 0;
    return msda_bwd_workspace_bytes_impl(B, I, H, D, Q, L, pmax, elem_size, (flags & MSDA_WS_RECORDS_IN_GRADS) ? 1 : 0,
                                         value_elem_size > 0 ? value_elem_size : elem_size, max_level_cells,
                                         ((flags >> 8) & 0xff) ? ((flags >> 8) & 0xff) : msda::option_ws_passes(), S);
}

// msda_bwd_fused_ragged_<dtype> (grad_value != NULL): the derived sampling points + attention weights (3 elements per
// sample, rounded up to 256 bytes: msda_launch.hpp, fused_mat_bytes), then the ragged operator's sorted-pipeline workspace
extern "C" int64_t msda_bwd_fused_ragged_workspace_bytes(int64_t B, int64_t I, int64_t H, int64_t D, int64_t Q, int64_t L,
                                                         const int32_t *points_per_level, int elem_size, int value_elem_size,
                                                         int64_t max_level_cells, int flags)
{
    int64_t pmax, S;
    if (B < 0 || I < 0 || H < 0 || D < 0 || Q < 0 || elem_size <= 0 || msda::ragged_counts(points_per_level, L, pmax, S) != 0)
        return 0;
    (void)value_elem_size;
    if (msda_fused_dims_refused_impl(B, I, H, D, Q, L, pmax, elem_size, S)) return 0;
    // the 16-bit operators park the derived points in float and run the float grad_value passes (msda_common.hpp, ParkType)
    if (elem_size == 2) elem_size = 4;
    if (msda_fused_dims_refused_impl(B, I, H, D, Q, L, pmax, elem_size, S)) return 0;
    const int64_t mat = (B * Q * H * S * 3 * (int64_t)elem_size + 255) / 256 * 256;
    return mat + msda_bwd_workspace_bytes_impl(B, I, H, D, Q, L, pmax, elem_size, 0, 0, max_level_cells,
                                               ((flags >> 8) & 0xff) ? ((flags >> 8) & 0xff) : msda::option_ws_passes(), S);
}

extern "C" int msda_bwd_ragged_supported(int64_t B, int64_t I, int64_t H, int64_t D, int64_t Q, int64_t L,
                                         const int32_t *points_per_level, int elem_size)
{
    int64_t pmax, S;
    if (B < 0 || I < 0 || H < 0 || D < 0 || Q < 0 || elem_size <= 0 || msda::ragged_counts(points_per_level, L, pmax, S) != 0)
        return 0;
    return msda_bwd_supported_impl(B, I, H, D, Q, L, pmax, elem_size, S);
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

extern "C" int msda_bwd_discrete_supported(int64_t B, int64_t I, int64_t H, int64_t D, int64_t Q, int64_t L,
                                           const int32_t *points_per_level, int elem_size)
{
    return msda_bwd_ragged_supported(B, I, H, D, Q, L, points_per_level, elem_size);
}
