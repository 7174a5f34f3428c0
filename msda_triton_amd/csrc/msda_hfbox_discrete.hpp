// msda_hfbox_discrete.hpp — Hugging Face's box rule in front of DISCRETE sampling (D-FINE / DEIMv2 / RT-DETRv2 with
// decoder_method = "discrete"): msda_{fwd,bwd}_fused_hfbox_discrete_<suffix> — and, through the same two kernels
// instantiated for another kernarg type, the reference module's own rule: msda_{fwd,bwd}_fused_discrete_<suffix>
// (ModuleDiscreteParams; the rule is stated at its fused_discrete_sample overload below).
//
// The kernels are msda_discrete.hpp's — one (b, head) plane per workgroup, G lanes per unit, VEC channels per lane, chunked
// trips over wide rows, the plane behind a buffer descriptor — with the module's prologue in the lanes instead of loaded
// points and weights: `proj` is the raw projection [B, Q, H, S, 3] (x offset, y offset, logit; level-major) and `ref` one
// box per query [B, Q, 4].
//
//   weight   a_s = exp(l_s - m) / sum_t exp(l_t - m) over the unit's S logits (UnitSoftmax: the ONE definition both
//            kernels call, so the weights the backward parks for grad_value are the forward's bit for bit)
//   point    hfbox_point(ref.xy, o * hfbox_scale(l), ref.wh, offset_scale), then discrete_pixel — the helpers of
//            msda_kernels.hpp with their guards against contraction: a fused multiply-add here picks another pixel
//
//   forward    msda_fwd_hfbox_discrete_kernel   one row per sample, weighted, summed over the unit's S
//   backward   msda_bwd_hfbox_discrete_kernel   g_s = <row, grad_out row>, grad_logit_s = a_s (g_s - sum_t a_t g_t); the two
//              offset slots of grad_proj are stored zeros (nothing differentiable reaches the pixel index, and so nothing
//              reaches the box either); with Params::mat_loc set, the points and weights are parked for the grad_value
//              passes, which are the discrete pipeline's own (DiscreteParams, cell_of)
//
// S is unbounded: nothing per sample is kept in registers or LDS across trips.  The statistics take two walks over the
// unit's logits, the weights are recomputed per trip from the logits (L1-resident after the first walk), and the backward
// leaves g_s in the sample's own grad_proj triple until the unit's sum is known — every lane reads back only what it wrote.
#pragma once

#include "msda_discrete.hpp"

namespace msda {

// max and 1 / sum(exp) of a unit's logits, left in every lane of the unit
template <typename A, int G> struct UnitSoftmax {
    A m, inv;
    template <typename TS> __device__ __forceinline__ UnitSoftmax(const TS *proj3, int S, bool live, int j)
    {
        using SR = Traits<TS>;
        m = (A)(-__builtin_inff());
        for (int s = j; s < S; s += G)
            if (live) m = fmax_t(m, SR::to_acc(proj3[3 * s + 2]));
        m = group_max<G>(m);
        A sum = (A)0;
        for (int s = j; s < S; s += G)
            if (live) sum += exp_t(SR::to_acc(proj3[3 * s + 2]) - m);
        inv = (A)1 / group_sum<G>(sum);
    }
    __device__ __forceinline__ A weight(A logit) const { return exp_t(logit - m) * inv; }
};

// the box of a unit's query, widened
template <typename A> struct UnitBox {
    A x, y, w, h;
};
template <typename T> __device__ __forceinline__ UnitBox<typename Traits<T>::acc> load_unit_box(const Params &p, int b, int q)
{
    using TR = Traits<T>;
    const T *r = static_cast<const T *>(p.ref) + ((size_t)b * p.Q + q) * 4;
    return {TR::to_acc(r[0]), TR::to_acc(r[1]), TR::to_acc(r[2]), TR::to_acc(r[3])};
}

// Sample s of a unit from its projection triple: the point (x, y), the logit and the row offset of its ONE pixel.
template <typename A, typename TS>
__device__ __forceinline__ uint32_t fused_discrete_sample(const HfBoxDiscreteParams &p, const LevelTab &tab, const TS *proj3, int s,
                                                         const UnitBox<A> &box, A &x, A &y, A &logit)
{
    using SR = Traits<TS>;
    const A ox = SR::to_acc(proj3[3 * s]), oy = SR::to_acc(proj3[3 * s + 1]);
    logit = SR::to_acc(proj3[3 * s + 2]);
    const int l = lvl_of(p, s, 0.0f);
    const A sc = hfbox_scale<A>(p, l), os = (A)p.off_scale;
    x = hfbox_point<A>(box.x, ox * sc, box.w, os);
    y = hfbox_point<A>(box.y, oy * sc, box.h, os);
    const int w = tab.w[l];
    const int ix = discrete_pixel<A>(x, w), iy = discrete_pixel<A>(y, tab.h[l]);
    return mad24(mad24((uint32_t)iy, (uint32_t)w, (uint32_t)tab.start[l]) + (uint32_t)ix, (uint32_t)p.v_row, 0u);
}

// ---- the reference module's rule (msda_*_fused_discrete_<suffix>; frontend.py:253-282, as the bilinear fused kernels keep
// it): `ref` is [B, Q, ref_dim], the kernarg ModuleDiscreteParams ----
//   2-d   x = ref_x + ox / h_l                 y = ref_y + oy / w_l          (img_shapes in its stored (h, w) order)
//   4-d   x = ref_x + ox * ref_w / (2 P_l)     y = ref_y + oy * ref_h / (2 P_l)   (P_l: the count of the sample's own level)
// a rounded multiply (4-d only), a correctly rounded TRUE division — not a multiplication by a reciprocal, which differs
// for P_l = 3 —, a rounded add.  The division sits between the other two, so -ffp-contract=fast finds nothing to fuse.
// The reference point of a unit's query: (x, y), and the box size for 4-d (zeros for 2-d: never read)
template <typename T>
__device__ __forceinline__ UnitBox<typename Traits<T>::acc> load_unit_box(const ModuleDiscreteParams &p, int b, int q)
{
    using TR = Traits<T>;
    using A = typename TR::acc;
    const T *r = static_cast<const T *>(p.ref) + ((size_t)b * p.Q + q) * p.ref_dim;
    const bool box = p.ref_dim == 4;  // (uniform)
    return {TR::to_acc(r[0]), TR::to_acc(r[1]), box ? TR::to_acc(r[2]) : (A)0, box ? TR::to_acc(r[3]) : (A)0};
}
template <typename A, typename TS>
__device__ __forceinline__ uint32_t fused_discrete_sample(const ModuleDiscreteParams &p, const LevelTab &tab, const TS *proj3, int s,
                                                         const UnitBox<A> &box, A &x, A &y, A &logit)
{
    using SR = Traits<TS>;
    const A ox = SR::to_acc(proj3[3 * s]), oy = SR::to_acc(proj3[3 * s + 1]);
    logit = SR::to_acc(proj3[3 * s + 2]);
    int npts;
    const int l = lvl_of(p, s, npts);
    const int w = tab.w[l], h = tab.h[l];
    // one division per axis for both rules: numerator and denominator are selected on the uniform ref_dim
    const bool box4 = p.ref_dim == 4;
    const A den = (A)(2 * npts);
    const A nx = box4 ? ox * box.w : ox, ny = box4 ? oy * box.h : oy;
    x = box.x + nx / (box4 ? den : (A)h);
    y = box.y + ny / (box4 ? den : (A)w);
    const int ix = discrete_pixel<A>(x, w), iy = discrete_pixel<A>(y, h);
    return mad24(mad24((uint32_t)iy, (uint32_t)w, (uint32_t)tab.start[l]) + (uint32_t)ix, (uint32_t)p.v_row, 0u);
}

// The forward of either rule: PP = HfBoxDiscreteParams or ModuleDiscreteParams picks fused_discrete_sample's and
// load_unit_box's overload, nothing else differs.
// T: arithmetic and box type, TV: value rows, TS: projection and out
template <typename T, int VEC, int G, typename TV, typename TS, typename PP>
__global__ __launch_bounds__(kBlock) void msda_fwd_hfbox_discrete_kernel(const PP p)
{
    using A = typename Traits<T>::acc;
    using SR = Traits<TS>;
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
    const TS *proj3 = static_cast<const TS *>(p.loc) + 3 * unit * S;
    const UnitBox<A> box = load_unit_box<T>(p, b, live ? q : 0);
    const UnitSoftmax<A, G> sm(proj3, S, live, j);
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
            A x, y, logit;
            off = fused_discrete_sample<A>(p, tab, proj3, s, box, x, y, logit);
            a = sm.weight(logit);
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
        Pack<TS, VEC> o;
#pragma unroll
        for (int i = 0; i < VEC; ++i) o.v[i] = SR::from_acc(acc[i]);
        store_stream(static_cast<TS *>(p.out) + unit * p.D + c0, o);
    }
    }
}

// g_s waits in the sample's grad_proj triple for the unit's sum: in the logit slot where the slot holds the arithmetic
// type, else (16-bit storage, float arithmetic) as two halves in the offset slots.  Read back by the lane that wrote it.
template <typename A, typename TS> struct GradTriple {
    static constexpr bool kSplit = sizeof(TS) != sizeof(A);
    using Word = std::conditional_t<kSplit, uint16_t, TS>;
    Word *w;
    __device__ __forceinline__ GradTriple(void *grad_proj, size_t sample) : w(static_cast<Word *>(grad_proj) + 3 * sample)
    {
        static_assert(kSplit ? (sizeof(TS) == 2 && sizeof(A) == 4) : std::is_same<TS, A>::value, "unexpected storage type");
    }
    __device__ __forceinline__ void stash(A g) const
    {
        if constexpr (kSplit) {
            const uint32_t bits = __builtin_bit_cast(uint32_t, g);
            w[0] = (uint16_t)bits;
            w[1] = (uint16_t)(bits >> 16);
        } else {
            w[2] = g;
        }
    }
    __device__ __forceinline__ A stashed() const
    {
        if constexpr (kSplit) return __builtin_bit_cast(A, (uint32_t)w[0] | ((uint32_t)w[1] << 16));
        else return w[2];
    }
    // the finished triple: the offsets have no gradient in this mode
    __device__ __forceinline__ void finish(A grad_logit) const
    {
        if constexpr (kSplit) {
            w[0] = w[1] = 0;
            w[2] = __builtin_bit_cast(uint16_t, Traits<TS>::from_acc(grad_logit));
        } else {
            w[0] = w[1] = (TS)0;
            w[2] = grad_logit;
        }
    }
};

// (PP: as the forward's)
template <typename T, int VEC, int G, typename TV, typename TS, typename PP>
__global__ __launch_bounds__(kBlock) void msda_bwd_hfbox_discrete_kernel(const PP p)
{
    using A = typename Traits<T>::acc;
    using SR = Traits<TS>;
    using MT = ParkType<T>;
    using MR = Traits<MT>;
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
    const TS *proj3 = static_cast<const TS *>(p.loc) + 3 * unit * S;
    const UnitBox<A> box = load_unit_box<T>(p, b, live ? q : 0);
    // (the channel chunks are the inner loop of a sample, as in msda_bwd_discrete_attn_kernel)
    const int nchunk = (p.D + G * VEC - 1) / (G * VEC);
    const TS *go_row = static_cast<const TS *>(p.grad_out) + unit * p.D;
    const int c00 = j * VEC;
    const bool lane_on = c00 < p.D;
    const uint32_t lane_off = (uint32_t)(c00 * (int)sizeof(TV));
    A g[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) g[i] = (A)0;
    if (live && lane_on) {
        const Pack<TS, VEC> gp = *reinterpret_cast<const Pack<TS, VEC> *>(go_row + c00);
#pragma unroll
        for (int i = 0; i < VEC; ++i) g[i] = SR::to_acc(gp.v[i]);
    }
    const UnitSoftmax<A, G> sm(proj3, S, live, j);
    A wsum = (A)0;  // this lane's share of sum_t a_t g_t
    for (int s0 = 0; s0 < S; s0 += G) {
        const int s = s0 + j;
        uint32_t off = kMaskedOffset;
        A a = (A)0;
        if (live && s < S) {
            A x, y, logit;
            off = fused_discrete_sample<A>(p, tab, proj3, s, box, x, y, logit);
            a = sm.weight(logit);
            if (p.mat_loc != nullptr) {  // for the grad_value passes: the point the forward sampled and its weight
                Pack<MT, 2> m;
                m.v[0] = MR::from_acc(x);
                m.v[1] = MR::from_acc(y);
                *reinterpret_cast<Pack<MT, 2> *>(static_cast<MT *>(p.mat_loc) + 2 * (unit * S + s)) = m;
                static_cast<MT *>(p.mat_attn)[unit * S + s] = MR::from_acc(a);
            }
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
                    const Pack<TS, VEC> gp = *reinterpret_cast<const Pack<TS, VEC> *>(go_row + c0);
#pragma unroll
                    for (int i = 0; i < VEC; ++i) dot = fma_t(row[i], SR::to_acc(gp.v[i]), dot);
                }
            }
            dot = group_sum<G>(dot);
            if (j == k) mine = dot;
        }
        if (live && s < S) {
            wsum = fma_t(a, mine, wsum);
            GradTriple<A, TS>(p.grad_loc, unit * S + s).stash(mine);
        }
    }
    wsum = group_sum<G>(wsum);
    for (int s = j; s < S; s += G) {
        if (!live) break;
        const GradTriple<A, TS> t(p.grad_loc, unit * S + s);
        const A a = sm.weight(SR::to_acc(proj3[3 * s + 2]));
        t.finish(a * (t.stashed() - wsum));
    }
}

}  // namespace msda
