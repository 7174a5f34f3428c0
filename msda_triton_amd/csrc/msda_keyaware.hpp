// msda_keyaware.hpp — key-aware deformable attention: the weights of a unit's samples are a softmax over what was SAMPLED.
//
//   K_s = bilinear(key_h, p_s)              V_s = bilinear(value_h, p_s)
//   z_s = scale * <query[b, q, h, :], K_s>  a = softmax_s(z)              out[b, q, h, :] = sum_s a_s * V_s
//
// (Lite-DETR's key-aware deformable attention, the sampled-key attention of the DAT family.)  `key` is a second pyramid of
// `value`'s shape and row stride, sampled at the same points: one tap record — four byte offsets, four bilinear weights —
// serves both through two buffer descriptors.  The softmax cannot be hoisted out of the gather, so the family has kernels
// of its own; no other kernel or template knows about it.
//
//   forward           msda_keyaware_fwd_kernel         one pass over the rows, online softmax, second output `attn`
//   sample gradients  msda_keyaware_bwd_sample_kernel  grad_query, grad_loc and the key weights scale * dz, one pass
//   pyramid gradients the grad_value pipelines as they are (msda_value_sorted.hpp, msda_value_small.hpp), run twice:
//                     weights `attn` on the rows of grad_out -> grad_value, weights scale * dz on the rows of query -> grad_key
//
// Both kernels use the bilinear forward's decomposition and addressing: a workgroup serves ONE (b, head) plane
// (decode_block), a unit (b, q, head) is served by G lanes x VEC channels, the planes are buffer descriptors over 64-bit
// bases with 32-bit in-plane offsets, rows are Params::v_row bytes apart, the level table is read in-kernel, and a corner
// dropped by "zeros" padding carries the out-of-range offset the hardware answers with 0 — in either pyramid.
//   phase 1 (per wave, one sample per lane and trip): make_taps ONCE per sample, parked in the wave's LDS slice
//   phase 2 (per unit, G lanes): the head rows of query (and grad_out) stay in registers; per sample 4 key rows and 4
//           value rows are requested together, two samples' rows (16 loads) in flight per lane
//   phase 3 (per wave): coalesced write-out of the per-sample results, one sample per lane and trip
// A wave reads only its own records: no block barrier behind the level table.  A unit with more samples than the record
// area holds makes several trips; what carries across them is said at each kernel.
#pragma once

#include "msda_kernels.hpp"

namespace msda {

// The kernarg: Params (value, shapes, loc, sizes, modes) and, BEHIND it, what only this family has.
//   forward   out, mat_attn = the attention weights [B, Q, H, L, P] it writes
//   backward  grad_out, attn (the forward's), out = grad_query, grad_loc, mat_attn = scale * dz [B, Q, H, L, P] for the
//             grad_key passes (ParkType: float32 for the 16-bit operators, which also park the points and weights in
//             float32 at mat_loc / grad_attn for the float grad_value passes; NULL: both pyramids frozen)
struct KeyAwareParams : Params {
    const void *query;  // [B, Q, H, D]
    const void *key;    // [B, I, H, D], rows Params::v_row bytes apart like value's
    double scale;       // cast once to the accumulate type
};

template <typename T> __device__ __forceinline__ const unsigned char *keyaware_plane(const void *base, const Params &p, int b, int h)
{
    return static_cast<const unsigned char *>(base) + (size_t)b * p.I * (size_t)p.v_row + (size_t)h * p.D * sizeof(T);
}

// the four corner rows of one sample, requested together and kept packed until they are consumed
template <typename T, int VEC> __device__ __forceinline__ void request_rows(rsrc_t rs, const uint4 &o, uint32_t lo, Pack<T, VEC> (&r)[4])
{
    using RL = RawLoad<sizeof(T) * VEC>;
    r[0] = __builtin_bit_cast(Pack<T, VEC>, RL::load(rs, o.x + lo));
    r[1] = __builtin_bit_cast(Pack<T, VEC>, RL::load(rs, o.y + lo));
    r[2] = __builtin_bit_cast(Pack<T, VEC>, RL::load(rs, o.z + lo));
    r[3] = __builtin_bit_cast(Pack<T, VEC>, RL::load(rs, o.w + lo));
}
// the lane's slice of a unit's head row, widened (zeros on a lane beyond the row: it joins the group sums with nothing)
template <typename T, int VEC> __device__ __forceinline__ void head_row(const T *row, bool on, typename Traits<T>::acc (&dst)[VEC])
{
    Pack<T, VEC> pk;
#pragma unroll
    for (int i = 0; i < VEC; ++i) pk.v[i] = Traits<T>::from_acc(0);
    if (on) pk = *reinterpret_cast<const Pack<T, VEC> *>(row);
#pragma unroll
    for (int i = 0; i < VEC; ++i) dst[i] = Traits<T>::to_acc(pk.v[i]);
}
// sum_k w[k] * r[k][i]: the bilinear blend of the lane's slice
template <typename T, int VEC> __device__ __forceinline__ void blend_rows(const typename Traits<T>::acc (&w)[4], const Pack<T, VEC> (&r)[4],
                                                                          typename Traits<T>::acc (&dst)[VEC])
{
    using TR = Traits<T>;
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
        typename TR::acc s = w[0] * TR::to_acc(r[0].v[i]);
        s = fma_t(w[1], TR::to_acc(r[1].v[i]), s);
        s = fma_t(w[2], TR::to_acc(r[2].v[i]), s);
        dst[i] = fma_t(w[3], TR::to_acc(r[3].v[i]), s);
    }
}
template <typename A> __device__ __forceinline__ A minus_infinity() { return -(A)__builtin_huge_valf(); }

// ==========================================================================================
// forward.  Per unit and lane: the query slice, a running maximum m, a running sum l and the D-wide accumulator, all in
// the accumulate type; a sample's score is one group_sum, and when the maximum moves the sum and the accumulator are
// rescaled by exp(m_old - m_new) (the fused prologues' exp_t).  A sample's score replaces its first bilinear weight in
// the LDS record once its rows are blended; at the end of a trip the wave writes attn = exp(z - m) / l coalesced.
// Several trips: m, l and the accumulator carry in registers.  The attention rows of earlier trips are written as
// exp(z - m) with the running maximum of THEIR trip; a later trip that moves a unit's maximum rescales those scalars by
// exp(m_old - m_new), and the last trip also divides them by l — passes over the S scalars, never over the rows.
// ==========================================================================================
template <typename T, int VEC, int G>
__global__ __launch_bounds__(kBlock) void msda_keyaware_fwd_kernel(const KeyAwareParams p)
{
    using A = typename Traits<T>::acc;
    using TR = Traits<T>;
    constexpr int NU = kBlock / G, UPW = kWave / G;
    int pair, slot;
    if (!decode_block(p.grid3d, p.B * p.H, p.nqc, p.xcd_map, pair, slot)) return;
    const int b = (int)fast_div((uint32_t)pair, p.div_h), h = pair - b * p.H;
    const int scp = p.sc + 1;  // +1 slot per unit: its (m, 1 / l, rescale factor) at the end of a trip
    const GatherLds<A> lds(NU, scp);
    LevelTab *tab = lds.tab;
    load_level_table(tab, p.shapes, p.L);
    __syncthreads();

    const uint32_t row_bytes = (uint32_t)p.v_row;
    const rsrc_t rs_v = make_rsrc(keyaware_plane<T>(p.value, p, b, h), plane_span<T>(p, h));
    const rsrc_t rs_k = make_rsrc(keyaware_plane<T>(p.key, p, b, h), plane_span<T>(p, h));
    const int tid = threadIdx.x, wave = tid / kWave, lane = tid % kWave;
    const int wunit = lane / G, j = lane % G;
    uint4 *w_off = lds.s_off + wave * UPW * scp;
    Rec4<A> *w_rec = lds.s_rec + wave * UPW * scp;
    const size_t plane_s0 = ((size_t)b * p.Q * p.H + h) * p.LP;
    const T *loc = static_cast<const T *>(p.loc) + 2 * plane_s0;
    T *attn = static_cast<T *>(p.mat_attn) + plane_s0;
    const int HLP = p.H * p.LP, S = p.LP;
    const float inv_P = 1.0f / (float)p.P;
    const A scale = (A)p.scale;

    const int wq0 = slot * NU + wave * UPW;  // first query of this wave (wave-uniform)
    if (wq0 >= p.Q) return;
    const int q = wq0 + wunit;
    const bool unit_ok = q < p.Q;
    const int c0 = j * VEC;
    const bool lane_on = c0 < p.D;
    const uint32_t lo = lane_on ? (uint32_t)c0 * (uint32_t)sizeof(T) : 0u;
    const size_t urow = ((size_t)(b * (size_t)p.Q + (unit_ok ? q : 0)) * p.H + h) * p.D;
    A qv[VEC], acc[VEC];
    head_row<T, VEC>(static_cast<const T *>(p.query) + urow + c0, unit_ok && lane_on, qv);
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc[i] = (A)0;
    A m = minus_infinity<A>(), l = (A)0;

    for (int s0 = 0; s0 < S; s0 += p.sc) {
        const int sc = min(p.sc, S - s0);
        const float inv_sc = 1.0f / (float)sc;
        const bool last = s0 + sc >= S;
        wave_lds_sync();  // previous records consumed
        // ---- phase 1: the wave's UPW * sc samples, one per lane and trip ----
        for (int f = lane; f < UPW * sc; f += kWave) {
            const int fu = div_small(f, sc, inv_sc);
            const int sl = s0 + (f - imul24(fu, sc));
            const int fq = wq0 + fu;
            if (fq < p.Q) {
                const int l_ = lvl_of(p, sl, inv_P);
                const Pack<T, 2> xy = *reinterpret_cast<const Pack<T, 2> *>(loc + 2 * (imul24(fq, HLP) + sl));
                Taps<A> t;
                make_taps<A>(TR::to_acc(xy.v[0]), TR::to_acc(xy.v[1]), tab->h[l_], tab->w[l_], tab->start[l_], p.zeros, p.align, row_bytes, t);
                const A wy0 = (A)1 - t.dy, wx0 = (A)1 - t.dx;
                Rec4<A> w;
                w.v[0] = wy0 * wx0;
                w.v[1] = wy0 * t.dx;
                w.v[2] = t.dy * wx0;
                w.v[3] = t.dy * t.dx;
                const int rslot = imul24(fu, scp) + (sl - s0);
                w_off[rslot] = make_uint4(t.off[0], t.off[1], t.off[2], t.off[3]);
                w_rec[rslot] = w;
            }
        }
        wave_lds_sync();
        // ---- phase 2: two samples' key and value rows in flight, scores, online softmax ----
        const A m_start = m;
        if (unit_ok) {  // (idle lanes of a live unit join the group sums)
            const uint4 *uo = w_off + imul24(wunit, scp);
            Rec4<A> *uw = w_rec + imul24(wunit, scp);
            for (int s = 0; s < sc; s += 2) {
                const bool two = s + 1 < sc;  // (uniform)
                const uint4 oa = uo[s], ob = uo[two ? s + 1 : s];
                const Rec4<A> wa = uw[s], wb = uw[two ? s + 1 : s];
                Pack<T, VEC> ka[4], va[4], kb[4], vb[4];
                request_rows<T, VEC>(rs_k, oa, lo, ka);
                request_rows<T, VEC>(rs_v, oa, lo, va);
                request_rows<T, VEC>(rs_k, ob, lo, kb);
                request_rows<T, VEC>(rs_v, ob, lo, vb);
                auto take = [&](int si, const Rec4<A> &w, const Pack<T, VEC> (&kr)[4], const Pack<T, VEC> (&vr)[4]) {
                    A ks[VEC], vs[VEC];
                    blend_rows<T, VEC>(w.v, kr, ks);
                    A dot = (A)0;
#pragma unroll
                    for (int i = 0; i < VEC; ++i) dot = fma_t(qv[i], ks[i], dot);
                    const A z = scale * group_sum<G>(dot);
                    blend_rows<T, VEC>(w.v, vr, vs);
                    const A m_new = fmax_t(m, z);
                    const A corr = exp_t(m - m_new), e = exp_t(z - m_new);
                    l = fma_t(l, corr, e);
#pragma unroll
                    for (int i = 0; i < VEC; ++i) acc[i] = fma_t(e, vs[i], acc[i] * corr);
                    m = m_new;
                    if (j == 0) uw[si].v[0] = z;  // (its weights are consumed: the score takes the first one's place)
                };
                take(s, wa, ka, va);
                if (two) take(s + 1, wb, kb, vb);
            }
            if (j == 0) {
                Rec4<A> st;
                st.v[0] = m;
                st.v[1] = last ? (A)1 / l : (A)1;
                st.v[2] = exp_t(m_start - m);  // what the rows of earlier trips are rescaled by
                st.v[3] = (A)0;
                uw[p.sc] = st;
            }
        }
        wave_lds_sync();
        // ---- phase 3: the trip's attention weights, coalesced ----
        for (int f = lane; f < UPW * sc; f += kWave) {
            const int fu = div_small(f, sc, inv_sc);
            const int sl = f - imul24(fu, sc);
            const int fq = wq0 + fu;
            if (fq < p.Q) {
                const Rec4<A> st = w_rec[imul24(fu, scp) + p.sc];
                attn[imul24(fq, HLP) + s0 + sl] = TR::from_acc(exp_t(w_rec[imul24(fu, scp) + sl].v[0] - st.v[0]) * st.v[1]);
            }
        }
        // ... and the rows of earlier trips: exp(z - m_then) -> exp(z - m_now), over 1 / l in the last trip.  Only when a
        // unit of the wave moved its maximum, or at the end (a wave reads back what its own lanes stored: fenced)
        if (s0 > 0) {
            const bool moved = unit_ok && m != m_start;
            if (last || __any(moved)) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                for (int f = lane; f < UPW * s0; f += kWave) {
                    const int fu = f / s0, sl = f - fu * s0;
                    const int fq = wq0 + fu;
                    if (fq < p.Q) {
                        const Rec4<A> st = w_rec[imul24(fu, scp) + p.sc];
                        T *dst = attn + imul24(fq, HLP) + sl;
                        *dst = TR::from_acc(TR::to_acc(*dst) * (st.v[2] * st.v[1]));
                    }
                }
            }
        }
    }
    if (unit_ok && lane_on) {
        const A inv_l = (A)1 / l;
        Pack<T, VEC> o;
#pragma unroll
        for (int i = 0; i < VEC; ++i) o.v[i] = TR::from_acc(acc[i] * inv_l);
        store_stream(static_cast<T *>(p.out) + urow + c0, o);
    }
}

// ==========================================================================================
// backward, the sample half.  The rows of grad_out (g) and query (q) stay in registers.  Per sample, one pass over its 8 rows:
//   value rows   dp = <g, V_s> and the directional dots <g, dV_s/dx>, <g, dV_s/dy>
//   key rows     K_s (the lane's slice) and <q, dK_s/dx>, <q, dK_s/dy>
// five group sums; A1 += a dp K_s and A2 += a K_s are D-wide register accumulators, c = sum_s a_s dp_s a scalar.  The five
// scalars and a go to the sample's LDS record; with c known, phase 3 writes per sample
//   dz = a (dp - c)      grad_loc = a d<g, V> + scale dz d<q, K>  (un-normalised as the bilinear grad_loc)      scale dz
// and the unit ends with grad_query = scale (A1 - c A2).  No atomics: every output element has one writer.
// Several trips: c is complete only behind the last one, and the records of earlier trips are gone by then — such a unit
// runs the trips TWICE, the first time for c alone (the same arithmetic in the same order, so c is the same bits).
// ==========================================================================================
template <typename T, int VEC, int G>
__global__ __launch_bounds__(kBlock) void msda_keyaware_bwd_sample_kernel(const KeyAwareParams p)
{
    using A = typename Traits<T>::acc;
    using TR = Traits<T>;
    using MT = ParkType<T>;
    using MR = Traits<MT>;
    constexpr int NU = kBlock / G, UPW = kWave / G;
    int pair, slot;
    if (!decode_block(p.grid3d, p.B * p.H, p.nqc, p.xcd_map, pair, slot)) return;
    const int b = (int)fast_div((uint32_t)pair, p.div_h), h = pair - b * p.H;
    const int scp = p.sc + 1;  // +1 slot per unit: its c
    // record in : {dx, dy, sx * gx_on, sy * gy_on}, aux a;  out (same slot): {dp, d<g,V>/dx, d<g,V>/dy, -}, aux d<q,K>/dx, /dy
    const GatherLds<A> lds(NU, scp, true);
    LevelTab *tab = lds.tab;
    load_level_table(tab, p.shapes, p.L);
    __syncthreads();

    const uint32_t row_bytes = (uint32_t)p.v_row;
    const rsrc_t rs_v = make_rsrc(keyaware_plane<T>(p.value, p, b, h), plane_span<T>(p, h));
    const rsrc_t rs_k = make_rsrc(keyaware_plane<T>(p.key, p, b, h), plane_span<T>(p, h));
    const int tid = threadIdx.x, wave = tid / kWave, lane = tid % kWave;
    const int wunit = lane / G, j = lane % G;
    uint4 *w_off = lds.s_off + wave * UPW * scp;
    Rec4<A> *w_rec = lds.s_rec + wave * UPW * scp;
    A *w_a = lds.s_aux + wave * UPW * scp * 3, *w_kx = w_a + UPW * scp, *w_ky = w_a + 2 * UPW * scp;
    const size_t plane_s0 = ((size_t)b * p.Q * p.H + h) * p.LP;
    const T *loc = static_cast<const T *>(p.loc) + 2 * plane_s0;
    const T *attn = static_cast<const T *>(p.attn) + plane_s0;
    const int HLP = p.H * p.LP, S = p.LP;
    const float inv_P = 1.0f / (float)p.P;
    const A scale = (A)p.scale;

    const int wq0 = slot * NU + wave * UPW;
    if (wq0 >= p.Q) return;
    const int q = wq0 + wunit;
    const bool unit_ok = q < p.Q;
    const int c0 = j * VEC;
    const bool lane_on = c0 < p.D;
    const uint32_t lo = lane_on ? (uint32_t)c0 * (uint32_t)sizeof(T) : 0u;
    const size_t urow = ((size_t)(b * (size_t)p.Q + (unit_ok ? q : 0)) * p.H + h) * p.D;
    A g[VEC], qv[VEC], a1[VEC], a2[VEC];
    head_row<T, VEC>(static_cast<const T *>(p.grad_out) + urow + c0, unit_ok && lane_on, g);
    head_row<T, VEC>(static_cast<const T *>(p.query) + urow + c0, unit_ok && lane_on, qv);

    const bool multi = S > p.sc;
    A c = (A)0;
    for (int pass = multi ? 0 : 1; pass < 2; ++pass) {
        A cc = (A)0;
#pragma unroll
        for (int i = 0; i < VEC; ++i) a1[i] = a2[i] = (A)0;
        for (int s0 = 0; s0 < S; s0 += p.sc) {
            const int sc = min(p.sc, S - s0);
            const float inv_sc = 1.0f / (float)sc;
            wave_lds_sync();
            // ---- phase 1 ----
            for (int f = lane; f < UPW * sc; f += kWave) {
                const int fu = div_small(f, sc, inv_sc);
                const int sl = s0 + (f - imul24(fu, sc));
                const int fq = wq0 + fu;
                if (fq < p.Q) {
                    const int l_ = lvl_of(p, sl, inv_P);
                    const int sidx = imul24(fq, HLP) + sl;
                    const Pack<T, 2> xy = *reinterpret_cast<const Pack<T, 2> *>(loc + 2 * sidx);
                    const int lh = tab->h[l_], lw = tab->w[l_];
                    Taps<A> t;
                    make_taps<A>(TR::to_acc(xy.v[0]), TR::to_acc(xy.v[1]), lh, lw, tab->start[l_], p.zeros, p.align, row_bytes, t);
                    Rec4<A> r;
                    r.v[0] = t.dx;
                    r.v[1] = t.dy;
                    r.v[2] = t.gx_on ? (p.align ? (A)(lw - 1) : (A)lw) : (A)0;
                    r.v[3] = t.gy_on ? (p.align ? (A)(lh - 1) : (A)lh) : (A)0;
                    const int rslot = imul24(fu, scp) + (sl - s0);
                    w_off[rslot] = make_uint4(t.off[0], t.off[1], t.off[2], t.off[3]);
                    w_rec[rslot] = r;
                    w_a[rslot] = TR::to_acc(attn[sidx]);
                }
            }
            wave_lds_sync();
            // ---- phase 2: two samples' 16 rows in flight ----
            if (unit_ok) {
                const int u0 = imul24(wunit, scp);
                for (int s = 0; s < sc; s += 2) {
                    const bool two = s + 1 < sc;  // (uniform)
                    const int sb = two ? s + 1 : s;
                    const uint4 oa = w_off[u0 + s], ob = w_off[u0 + sb];
                    Pack<T, VEC> ka[4], va[4], kb[4], vb[4];
                    request_rows<T, VEC>(rs_v, oa, lo, va);
                    request_rows<T, VEC>(rs_k, oa, lo, ka);
                    request_rows<T, VEC>(rs_v, ob, lo, vb);
                    request_rows<T, VEC>(rs_k, ob, lo, kb);
                    auto take = [&](int si, const Pack<T, VEC> (&kr)[4], const Pack<T, VEC> (&vr)[4]) {
                        const Rec4<A> r = w_rec[u0 + si];
                        const A a = w_a[u0 + si];
                        const A dx = r.v[0], dy = r.v[1], wy0 = (A)1 - dy, wx0 = (A)1 - dx;
                        A w[4] = {wy0 * wx0, wy0 * dx, dy * wx0, dy * dx};
                        A ks[VEC];
                        blend_rows<T, VEC>(w, kr, ks);
                        A d[4] = {0, 0, 0, 0}, e[4] = {0, 0, 0, 0};
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
#pragma unroll
                            for (int i = 0; i < VEC; ++i) {
                                d[k] = fma_t(g[i], TR::to_acc(vr[k].v[i]), d[k]);
                                e[k] = fma_t(qv[i], TR::to_acc(kr[k].v[i]), e[k]);
                            }
                        }
                        A dp = w[0] * d[0] + w[1] * d[1] + w[2] * d[2] + w[3] * d[3];
                        A vx = wy0 * (d[1] - d[0]) + dy * (d[3] - d[2]), vy = wx0 * (d[2] - d[0]) + dx * (d[3] - d[1]);
                        A kx = wy0 * (e[1] - e[0]) + dy * (e[3] - e[2]), ky = wx0 * (e[2] - e[0]) + dx * (e[3] - e[1]);
                        dp = group_sum<G>(dp);
                        vx = group_sum<G>(vx);
                        vy = group_sum<G>(vy);
                        kx = group_sum<G>(kx);
                        ky = group_sum<G>(ky);
                        const A adp = a * dp;
                        cc += adp;
#pragma unroll
                        for (int i = 0; i < VEC; ++i) {
                            a1[i] = fma_t(adp, ks[i], a1[i]);
                            a2[i] = fma_t(a, ks[i], a2[i]);
                        }
                        if (j == 0) {
                            Rec4<A> res;
                            res.v[0] = dp;
                            res.v[1] = r.v[2] * vx;
                            res.v[2] = r.v[3] * vy;
                            res.v[3] = (A)0;
                            w_rec[u0 + si] = res;
                            w_kx[u0 + si] = r.v[2] * kx;
                            w_ky[u0 + si] = r.v[3] * ky;
                        }
                    };
                    take(s, ka, va);
                    if (two) take(sb, kb, vb);
                }
            }
            if (pass == 0) continue;  // (the first of two runs: c alone)
            if (!multi) c = cc;
            if (unit_ok && j == 0) w_rec[imul24(wunit, scp) + p.sc].v[0] = c;
            wave_lds_sync();
            // ---- phase 3: coalesced write-out, one sample per lane and trip ----
            for (int f = lane; f < UPW * sc; f += kWave) {
                const int fu = div_small(f, sc, inv_sc);
                const int sl = f - imul24(fu, sc);
                const int fq = wq0 + fu;
                if (fq < p.Q) {
                    const int rslot = imul24(fu, scp) + sl;
                    const size_t sidx = plane_s0 + (size_t)(imul24(fq, HLP) + s0 + sl);
                    const Rec4<A> res = w_rec[rslot];
                    const A a = w_a[rslot], sdz = scale * (a * (res.v[0] - w_rec[imul24(fu, scp) + p.sc].v[0]));
                    if (p.grad_loc != nullptr) {  // (NULL with grad_query: a call for the pyramid gradients alone)
                        Pack<T, 2> gl;
                        gl.v[0] = TR::from_acc(fma_t(sdz, w_kx[rslot], a * res.v[1]));
                        gl.v[1] = TR::from_acc(fma_t(sdz, w_ky[rslot], a * res.v[2]));
                        store_stream(static_cast<T *>(p.grad_loc) + 2 * sidx, gl);
                    }
                    if (p.mat_attn != nullptr) static_cast<MT *>(p.mat_attn)[sidx] = MR::from_acc(sdz);
                    if constexpr (sizeof(MT) != sizeof(T)) {
                        // the 16-bit operators: points and weights once more in float32, for the float grad_value passes
                        if (p.mat_loc != nullptr) {
                            const Pack<T, 2> xy = *reinterpret_cast<const Pack<T, 2> *>(static_cast<const T *>(p.loc) + 2 * sidx);
                            Pack<MT, 2> m;
                            m.v[0] = TR::to_acc(xy.v[0]);
                            m.v[1] = TR::to_acc(xy.v[1]);
                            *reinterpret_cast<Pack<MT, 2> *>(static_cast<MT *>(p.mat_loc) + 2 * sidx) = m;
                            static_cast<MT *>(p.grad_attn)[sidx] = a;
                        }
                    }
                }
            }
        }
        if (pass == 0) c = cc;
    }
    if (unit_ok && lane_on && p.out != nullptr) {
        Pack<T, VEC> o;
#pragma unroll
        for (int i = 0; i < VEC; ++i) o.v[i] = TR::from_acc(scale * (a1[i] - c * a2[i]));
        store_stream(static_cast<T *>(p.out) + urow + c0, o);
    }
}

}  // namespace msda
