// msda_discrete.hpp — discrete (nearest-pixel) sampling: every sample reads exactly ONE value row, chosen by rounding.
//
//   ix = clamp(trunc(x * w + 0.5), 0, w - 1)      iy = clamp(trunc(y * h + 0.5), 0, h - 1)
//   out[b, q, head, :] += a * value[b, start_l + iy * w + ix, head, :]
//
// (transformers' multi_scale_deformable_attention_v2(method="discrete"); NOT grid_sample's "nearest": no pixel-centre
// shift, out-of-range samples clamp to the edge pixel, padding_mode / align_corners have no meaning.)  The layout is the
// per-level-count one (RaggedParams: S = sum_l P_l samples per unit, level-major); the sampling points get no gradient.
//
//   forward            msda_fwd_discrete_kernel       one row per sample, attention-weighted, summed over the unit's S
//   grad_attn          msda_bwd_discrete_attn_kernel  one row per sample, dot with the unit's grad_out row, group_sum
//   grad_value         the sorted / single-launch cell pipelines (msda_value_sorted.hpp, msda_value_place.hpp,
//                      msda_value_small.hpp) instantiated for DiscreteParams: a discrete sample is a record of cell
//                      (x0, y0) = (ix, iy) with dx = dy = 0 — the whole weight on corner 00 (cell_of, msda_value_sorted.hpp); the scan,
//                      gather and finish kernels are the bilinear call's own (they take Params and are not instantiated
//                      again).  Atomic-free on floating-point data and bitwise reproducible, as the bilinear one.
//
// Both kernels here use the bilinear forward's addressing: a workgroup serves ONE (b, head) plane (decode_block), the plane
// is a buffer descriptor over a 64-bit base with 32-bit in-plane offsets (so a level table that disagrees with I reads
// zeros, never out of bounds), rows are Params::v_row bytes apart, the level table is read in-kernel from the device
// shapes tensor and a sample finds its level from the level starts.
#pragma once

#include "msda_kernels.hpp"  // DiscreteParams, discrete_pixel

namespace msda {

// units (b, q, head) per 256-thread workgroup: kBlock / G, G lanes per unit and VEC channels per lane
template <typename T, int VEC, int G, typename TV>
__global__ __launch_bounds__(kBlock) void msda_fwd_discrete_kernel(const DiscreteParams p)
{
    using A = typename Traits<T>::acc;
    using TR = Traits<T>;
    constexpr int NU = kBlock / G;
    __shared__ LevelTab tab;
    int pair, slot;
    if (!decode_block(p.grid3d, p.B * p.H, p.nqc, p.xcd_map, pair, slot)) return;
    load_level_table(&tab, p.shapes, p.L);
    __syncthreads();
    const int b = (int)fast_div((uint32_t)pair, p.div_h), h = pair - b * p.H;
    const int tid = threadIdx.x, j = tid % G;
    const int q = slot * NU + tid / G;
    const bool live = q < p.Q;  // (dead units keep their lanes: the group's shuffles below are wave-wide instructions)
    const rsrc_t rs = make_rsrc(plane_base<TV>(p, b, h), plane_span<TV>(p, h));
    const int S = p.LP;
    const size_t unit = ((size_t)b * p.Q + (live ? q : 0)) * p.H + h;
    const T *loc = static_cast<const T *>(p.loc) + 2 * unit * S;
    const T *attn = static_cast<const T *>(p.attn) + unit * S;
    // (rows wider than G * VEC channels — D = 512 in fp32 — take several trips, each over all samples)
    const int nchunk = (p.D + G * VEC - 1) / (G * VEC);
    for (int ch = 0; ch < nchunk; ++ch) {
    const int c0 = (ch * G + j) * VEC;
    const bool lane_on = c0 < p.D;
    const uint32_t lane_off = (uint32_t)(c0 * (int)sizeof(TV));
    A acc[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc[i] = (A)0;
    for (int s0 = 0; s0 < S; s0 += G) {
        // lane j of the unit: the row offset and weight of sample s0 + j
        const int s = s0 + j;
        uint32_t off = kMaskedOffset;
        A a = (A)0;
        if (live && s < S) {
            const Pack<T, 2> xy = *reinterpret_cast<const Pack<T, 2> *>(loc + 2 * s);
            a = TR::to_acc(attn[s]);
            const int l = lvl_of(p, s, 0.0f);
            const int w = tab.w[l];
            const int ix = discrete_pixel<A>(TR::to_acc(xy.v[0]), w), iy = discrete_pixel<A>(TR::to_acc(xy.v[1]), tab.h[l]);
            off = mad24(mad24((uint32_t)iy, (uint32_t)w, (uint32_t)tab.start[l]) + (uint32_t)ix, (uint32_t)p.v_row, 0u);
        }
        const int n = min(G, S - s0);  // (uniform)
#pragma unroll 4
        for (int k = 0; k < n; ++k) {
            const uint32_t o = (uint32_t)__shfl((int)off, k, G);
            const A wgt = __shfl(a, k, G);
            A row[VEC];
            load_row<TV, VEC>(rs, lane_on && o != kMaskedOffset ? o + lane_off : kMaskedOffset, row);
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc[i] = fma_t(wgt, row[i], acc[i]);
        }
    }
    if (live && lane_on) {
        Pack<T, VEC> o;
#pragma unroll
        for (int i = 0; i < VEC; ++i) o.v[i] = TR::from_acc(acc[i]);
        store_stream(static_cast<T *>(p.out) + unit * p.D + c0, o);
    }
    }
}

// grad_attn[b, q, head, s] = <value[b, pixel(s), head, :], grad_out[b, q, head, :]>
template <typename T, int VEC, int G, typename TV>
__global__ __launch_bounds__(kBlock) void msda_bwd_discrete_attn_kernel(const DiscreteParams p)
{
    using A = typename Traits<T>::acc;
    using TR = Traits<T>;
    constexpr int NU = kBlock / G;
    __shared__ LevelTab tab;
    int pair, slot;
    if (!decode_block(p.grid3d, p.B * p.H, p.nqc, p.xcd_map, pair, slot)) return;
    load_level_table(&tab, p.shapes, p.L);
    __syncthreads();
    const int b = (int)fast_div((uint32_t)pair, p.div_h), h = pair - b * p.H;
    const int tid = threadIdx.x, j = tid % G;
    const int q = slot * NU + tid / G;
    const bool live = q < p.Q;
    const rsrc_t rs = make_rsrc(plane_base<TV>(p, b, h), plane_span<TV>(p, h));
    const int S = p.LP;
    const size_t unit = ((size_t)b * p.Q + (live ? q : 0)) * p.H + h;
    const T *loc = static_cast<const T *>(p.loc) + 2 * unit * S;
    T *gattn = static_cast<T *>(p.grad_attn) + unit * S;
    // Rows wider than G * VEC channels (D = 512 in fp32) are walked in chunks INSIDE a sample: its dot product is complete,
    // in the accumulate type, before the one group_sum and the one store.  The first chunk's grad_out slice stays in
    // registers (the only chunk for every usual D); later chunks reload theirs per sample, from L1.
    const int nchunk = (p.D + G * VEC - 1) / (G * VEC);
    const T *go_row = static_cast<const T *>(p.grad_out) + unit * p.D;
    const int c00 = j * VEC;
    const bool lane_on = c00 < p.D;
    const uint32_t lane_off = (uint32_t)(c00 * (int)sizeof(TV));
    A g[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) g[i] = (A)0;
    if (live && lane_on) {
        const Pack<T, VEC> gp = *reinterpret_cast<const Pack<T, VEC> *>(go_row + c00);
#pragma unroll
        for (int i = 0; i < VEC; ++i) g[i] = TR::to_acc(gp.v[i]);
    }
    for (int s0 = 0; s0 < S; s0 += G) {
        const int s = s0 + j;
        uint32_t off = kMaskedOffset;
        if (live && s < S) {
            const Pack<T, 2> xy = *reinterpret_cast<const Pack<T, 2> *>(loc + 2 * s);
            const int l = lvl_of(p, s, 0.0f);
            const int w = tab.w[l];
            const int ix = discrete_pixel<A>(TR::to_acc(xy.v[0]), w), iy = discrete_pixel<A>(TR::to_acc(xy.v[1]), tab.h[l]);
            off = mad24(mad24((uint32_t)iy, (uint32_t)w, (uint32_t)tab.start[l]) + (uint32_t)ix, (uint32_t)p.v_row, 0u);
        }
        const int n = min(G, S - s0);
        A mine = (A)0;
#pragma unroll 4
        for (int k = 0; k < n; ++k) {
            const uint32_t o = (uint32_t)__shfl((int)off, k, G);
            A row[VEC];
            load_row<TV, VEC>(rs, lane_on && o != kMaskedOffset ? o + lane_off : kMaskedOffset, row);
            A dot = (A)0;
#pragma unroll
            for (int i = 0; i < VEC; ++i) dot = fma_t(row[i], g[i], dot);
            for (int ch = 1; ch < nchunk; ++ch) {  // (uniform trip count)
                const int c0 = (ch * G + j) * VEC;
                const bool on = live && c0 < p.D && o != kMaskedOffset;
                load_row<TV, VEC>(rs, on ? o + (uint32_t)(c0 * (int)sizeof(TV)) : kMaskedOffset, row);
                if (on) {
                    const Pack<T, VEC> gp = *reinterpret_cast<const Pack<T, VEC> *>(go_row + c0);
#pragma unroll
                    for (int i = 0; i < VEC; ++i) dot = fma_t(row[i], TR::to_acc(gp.v[i]), dot);
                }
            }
            dot = group_sum<G>(dot);
            if (j == k) mine = dot;
        }
        if (live && s < S) gattn[s] = TR::from_acc(mine);
    }
}

}  // namespace msda
