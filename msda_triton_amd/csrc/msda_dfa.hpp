// msda_dfa.hpp — deformable feature aggregation (Sparse4D v2 / v3, SparseDrive): every anchor's P key points are projected
// into every camera, each camera's pyramid is sampled at that ONE location on every level, and the samples are summed
// with a weight per (point, camera, level, channel group).
//
//   out[b, a, g, :] = sum_{p, c, l} valid(b, a, p, c) * weights[b, a, p, c, l, g]
//                                    * bilinear(feature_maps[b, map(c, l), g, :], x * w_cl - 0.5, y * h_cl - 0.5)
//   valid = 0 < x < 1 and 0 < y < 1     (strict; a dropped pair contributes nothing on any level)
//
// feature_maps [B, I, G, D] IS value [B, I, H, D] with H = G and the cams * levels maps as its levels (camera-major), so the
// grad_value pipelines serve grad_feature_maps as they are.  What differs from every other gather here, and why the family
// has kernels of its own (no other kernel, template or kernarg type knows about it):
//   * a unit is an anchor (b, a) with ALL C = G D channels: its lanes hold VEC channels each of the whole pixel row, which
//     a wave reads as one coalesced run (1 KB at C = 256 in fp32).  UL lanes serve a unit (the power of two that holds
//     C / VEC, at most the wave), 64 / UL units share a wave.  A row wider than one wave's chunk (C > 64 VEC) is served
//     in CHANNEL CHUNKS by the same wave: the forward runs its trips once per chunk (the accumulator of one chunk in
//     registers), the backward runs the chunks inside a trip and sums their partial results in the wave's LDS records.
//   * the location is shared by the levels and the groups: cell and fractions are made once per (point, camera, level)
//     and serve every group; the G weights of a record are contiguous, a lane reads the one of its group.
//   * a point is in view of one or two cameras of six: phase 1 COMPACTS the surviving (point, camera) pairs of a unit with
//     a ballot and a prefix count before any record is made, so a dropped pair costs no record, no loop trip and no
//     memory request.
//
//   phase 1a (per wave and unit, one pair per lane)    location, valid, ballot / prefix count -> the unit's list of survivors
//   phase 1b (per wave and unit, one record per lane)  survivor x level -> {4 byte offsets, 4 bilinear weights | fractions,
//                                                      the index of its G weights}
//   phase 2  (per unit, UL lanes)                      two records' eight rows in flight; accumulate (forward) or the dots
//                                                      with the grad_out row (backward)
//   phase 3  (backward, per wave)                      coalesced write-out of grad_weights and grad_sampling_locations — zeros
//                                                      for dropped pairs — and of the parked points and weights
// A wave reads only its own records: no block barrier behind the level table.  P * cams * levels records beyond the LDS area:
// trips over whole points, `pt` of them at a time (DfaParams::pt, msda_dfa_trip_records), the accumulator carried.
//
// ONE definition of a sample's cell: dfa_taps derives cell and fractions from the normalised location with sample_cell's
// own expression (the explicit fma, floor, px - floor; msda_value_sorted.hpp), and the backward parks exactly that location
// (ParkType), so forward, sample gradients and the pipeline agree bit for bit.  A dropped pair is parked as the point
// (-2, -2) with weight 0: every corner of its cell is outside every map, sample_cell gives it no cell.
#pragma once

#include "msda_kernels.hpp"

namespace msda {

// The kernarg: Params (value = feature_maps, shapes, loc = sampling_locations, attn = weights, out, grad_out, grad_loc,
// grad_attn = grad_weights, mat_loc / mat_attn = the parked points / weights; B, I, H = G, D, Q = A, L = cams * levels, P)
// and, BEHIND it, what only this family has.
struct DfaParams : Params {
    int cams, levels;
    int C;        // G * D
    int nch;      // channel chunks of UL * VEC channels per row
    int pt;       // points of a unit per trip
    int npc, rc;  // pairs (pt * cams) and records (npc * levels) a unit's LDS slice holds
};

// the workgroup's LDS: level table, then per unit slices of NU * {rc records, npc survivors}
template <typename A> struct DfaLds {
    LevelTab *tab;
    uint4 *off;       // [NU rc]   byte offsets of the four corner rows
    Rec4<A> *rec;     // [NU rc]   forward: the bilinear weights; backward: {dx, dy, w_cl, h_cl}
    A *ent;           // [NU npc 2] the survivors' locations
    A *res;           // [NU rc 2] backward: the record's d out / d (x, y), summed over channels and groups
    A *dp;            // [NU rc G] backward: <grad_out, bilinear> per group
    uint32_t *widx;   // [NU rc]   index of the record's G weights inside the unit's block
    int *epair;       // [NU npc]  the survivors' pair (p_local * cams + cam)
    int *pmap;        // [NU npc]  backward: pair -> its place among the survivors, -1: dropped
    int *cnt;         // [NU]      survivors of the unit in this trip
    __device__ __forceinline__ DfaLds(int NU, int npc, int rc, int G, bool bwd)
    {
        unsigned char *p = msda_smem;
        tab = reinterpret_cast<LevelTab *>(p);
        p += kGatherLdsFixedBytes;
        off = reinterpret_cast<uint4 *>(p);
        p += (size_t)NU * rc * sizeof(uint4);
        rec = reinterpret_cast<Rec4<A> *>(p);
        p += (size_t)NU * rc * sizeof(Rec4<A>);
        ent = reinterpret_cast<A *>(p);
        p += (size_t)NU * npc * 2 * sizeof(A);
        res = reinterpret_cast<A *>(p);
        if (bwd) p += (size_t)NU * rc * 2 * sizeof(A);
        dp = reinterpret_cast<A *>(p);
        if (bwd) p += (size_t)NU * rc * G * sizeof(A);
        widx = reinterpret_cast<uint32_t *>(p);
        p += (size_t)NU * rc * sizeof(uint32_t);
        epair = reinterpret_cast<int *>(p);
        p += (size_t)NU * npc * sizeof(int);
        pmap = reinterpret_cast<int *>(p);
        if (bwd) p += (size_t)NU * npc * sizeof(int);
        cnt = reinterpret_cast<int *>(p);
    }
};

// sample_cell's arithmetic on a location inside (0, 1)^2: the cell's corner 00 lies in [-1, n - 1], so no clamp is needed
// before the conversion; a corner outside the map carries the offset the descriptor answers with zeros.
template <typename A>
__device__ __forceinline__ void dfa_taps(A x, A y, int h, int w, int start, uint32_t row_bytes, uint32_t (&off)[4], A &dx, A &dy)
{
    const A px = fma_t(x, (A)w, (A)-0.5), py = fma_t(y, (A)h, (A)-0.5);
    const A x0 = floor_t(px), y0 = floor_t(py);
    dx = px - x0;
    dy = py - y0;
    const int ix = (int)x0, iy = (int)y0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int cx = ix + (k & 1), cy = iy + (k >> 1);
        off[k] = cx >= 0 && cx < w && cy >= 0 && cy < h ? mul24((uint32_t)(start + imul24(cy, w) + cx), row_bytes) : kMaskedOffset;
    }
}

// Phase 1 of both kernels for unit `fu` of the wave (anchor `a`): compaction, then the records of the survivors.
// kBwd: the records carry the fractions and the map's size instead of the four weights, and the pair map is kept.
template <typename T, bool kBwd, typename A>
__device__ __forceinline__ void dfa_phase1(const DfaParams &p, const DfaLds<A> &lds, int unit, int lane, const T *loc_u, int p0, int np,
                                           uint32_t row_bytes, float inv_lv, float inv_cams)
{
    using TR = Traits<T>;
    A *ent = lds.ent + (size_t)unit * p.npc * 2;
    int *epair = lds.epair + unit * p.npc, *pmap = lds.pmap + unit * p.npc;
    int cnt = 0;
    for (int pp0 = 0; pp0 < np; pp0 += kWave) {
        const int pp = pp0 + lane;
        const bool in = pp < np;
        A x = (A)0, y = (A)0;
        if (in) {
            const Pack<T, 2> xy = *reinterpret_cast<const Pack<T, 2> *>(loc_u + 2 * (imul24(p0, p.cams) + pp));
            x = TR::to_acc(xy.v[0]);
            y = TR::to_acc(xy.v[1]);
        }
        const bool valid = in && x > (A)0 && x < (A)1 && y > (A)0 && y < (A)1;  // (NaN: dropped)
        const uint64_t mask = __ballot(valid);
        const int pos = cnt + __popcll(mask & ((1ull << lane) - 1ull));
        if (valid) {
            ent[2 * pos] = x;
            ent[2 * pos + 1] = y;
            epair[pos] = pp;
        }
        if (kBwd && in) pmap[pp] = valid ? pos : -1;
        cnt += __popcll(mask);
    }
    if (lane == 0) lds.cnt[unit] = cnt;
    wave_lds_sync();
    const int nrec = imul24(cnt, p.levels);
    uint4 *w_off = lds.off + (size_t)unit * p.rc;
    Rec4<A> *w_rec = lds.rec + (size_t)unit * p.rc;
    uint32_t *w_idx = lds.widx + (size_t)unit * p.rc;
    for (int f = lane; f < nrec; f += kWave) {
        const int cp = div_small(f, p.levels, inv_lv), l = f - imul24(cp, p.levels);
        const int pp = epair[cp];
        const int cam = pp - imul24(div_small(pp, p.cams, inv_cams), p.cams);
        const int m = imul24(cam, p.levels) + l;
        const int h = lds.tab->h[m], w = lds.tab->w[m];
        uint32_t off[4];
        Rec4<A> r;
        A dx, dy;
        dfa_taps<A>(ent[2 * cp], ent[2 * cp + 1], h, w, lds.tab->start[m], row_bytes, off, dx, dy);
        if (kBwd) {
            r.v[0] = dx;
            r.v[1] = dy;
            r.v[2] = (A)w;
            r.v[3] = (A)h;
        } else {
            const A wy0 = (A)1 - dy, wx0 = (A)1 - dx;
            r.v[0] = wy0 * wx0;
            r.v[1] = wy0 * dx;
            r.v[2] = dy * wx0;
            r.v[3] = dy * dx;
        }
        w_off[f] = make_uint4(off[0], off[1], off[2], off[3]);
        w_rec[f] = r;
        w_idx[f] = (uint32_t)imul24(imul24(imul24(p0, p.cams) + pp, p.levels) + l, p.H);
    }
}

// the four corner rows of one record, requested together and kept packed until they are consumed
template <typename T, int VEC> __device__ __forceinline__ void dfa_rows(rsrc_t rs, const uint4 &o, uint32_t lo, Pack<T, VEC> (&r)[4])
{
    using RL = RawLoad<sizeof(T) * VEC>;
    r[0] = __builtin_bit_cast(Pack<T, VEC>, RL::load(rs, o.x + lo));
    r[1] = __builtin_bit_cast(Pack<T, VEC>, RL::load(rs, o.y + lo));
    r[2] = __builtin_bit_cast(Pack<T, VEC>, RL::load(rs, o.z + lo));
    r[3] = __builtin_bit_cast(Pack<T, VEC>, RL::load(rs, o.w + lo));
}

// ==========================================================================================
// forward
// ==========================================================================================
template <typename T, int VEC, int UL>
__global__ __launch_bounds__(kBlock) void msda_dfa_fwd_kernel(const DfaParams p)
{
    using A = typename Traits<T>::acc;
    using TR = Traits<T>;
    constexpr int NU = kBlock / UL, UPW = kWave / UL;
    int b, slot;
    if (!decode_block(p.grid3d, p.B, p.nqc, p.xcd_map, b, slot)) return;
    const DfaLds<A> lds(NU, p.npc, p.rc, p.H, false);
    load_level_table(lds.tab, p.shapes, p.L);
    __syncthreads();

    const uint32_t row_bytes = (uint32_t)p.v_row;
    const rsrc_t rs = make_rsrc(static_cast<const unsigned char *>(p.value) + (size_t)b * p.I * (size_t)p.v_row, plane_span<T>(p, 0));
    const int tid = threadIdx.x, wave = tid / kWave, lane = tid % kWave;
    const int wunit = lane / UL, j = lane % UL;
    const int wa0 = slot * NU + wave * UPW;  // first anchor of this wave (wave-uniform)
    if (wa0 >= p.Q) return;
    const int a = wa0 + wunit;
    const bool unit_ok = a < p.Q;
    const int pairs = imul24(p.P, p.cams);
    const size_t unit0 = (size_t)b * p.Q + wa0;  // the wave's first unit
    const T *loc = static_cast<const T *>(p.loc) + unit0 * pairs * 2;
    const T *wts = static_cast<const T *>(p.attn) + (unit0 + (unit_ok ? wunit : 0)) * ((size_t)pairs * p.levels * p.H);
    const float inv_lv = 1.0f / (float)p.levels, inv_cams = 1.0f / (float)p.cams;
    const int u0 = imul24(wave * UPW + wunit, p.rc);

    for (int ch = 0; ch < p.nch; ++ch) {  // (uniform; one chunk unless C > 64 VEC)
        const int c0 = (ch * UL + j) * VEC;
        const bool lane_on = c0 < p.C;
        const uint32_t lo = lane_on ? (uint32_t)c0 * (uint32_t)sizeof(T) : 0u;
        const int gl = lane_on ? c0 / p.D : 0;  // the lane's group
        A acc[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] = (A)0;
        for (int p0 = 0; p0 < p.P; p0 += p.pt) {
            const int np = imul24(min(p.pt, p.P - p0), p.cams);
            wave_lds_sync();  // previous records consumed
            for (int fu = 0; fu < UPW && wa0 + fu < p.Q; ++fu)
                dfa_phase1<T, false, A>(p, lds, wave * UPW + fu, lane, loc + (size_t)fu * pairs * 2, p0, np, row_bytes, inv_lv, inv_cams);
            wave_lds_sync();
            if (unit_ok) {
                // ---- phase 2: two records' rows in flight ----
                const int nrec = imul24(lds.cnt[wave * UPW + wunit], p.levels);
                for (int s = 0; s < nrec; s += 2) {
                    const bool two = s + 1 < nrec;
                    const int sb = two ? s + 1 : s;
                    const uint4 oa = lds.off[u0 + s], ob = lds.off[u0 + sb];
                    Pack<T, VEC> ra[4], rb[4];
                    dfa_rows<T, VEC>(rs, oa, lo, ra);
                    dfa_rows<T, VEC>(rs, ob, lo, rb);
                    const T wa = wts[lds.widx[u0 + s] + gl], wb = wts[lds.widx[u0 + sb] + gl];
                    auto take = [&](int si, const Pack<T, VEC> (&r)[4], T wt) {
                        const Rec4<A> w = lds.rec[u0 + si];
                        const A m = TR::to_acc(wt);
    #pragma unroll
                        for (int i = 0; i < VEC; ++i) {
                            A v = w.v[0] * TR::to_acc(r[0].v[i]);
                            v = fma_t(w.v[1], TR::to_acc(r[1].v[i]), v);
                            v = fma_t(w.v[2], TR::to_acc(r[2].v[i]), v);
                            v = fma_t(w.v[3], TR::to_acc(r[3].v[i]), v);
                            acc[i] = fma_t(m, v, acc[i]);
                        }
                    };
                    take(s, ra, wa);
                    if (two) take(sb, rb, wb);
                }
            }
        }
        if (unit_ok && lane_on) {
            Pack<T, VEC> o;
#pragma unroll
            for (int i = 0; i < VEC; ++i) o.v[i] = TR::from_acc(acc[i]);
            store_stream(static_cast<T *>(p.out) + ((size_t)b * p.Q + a) * p.C + c0, o);
        }
    }
}

// ==========================================================================================
// backward, the sample half.  Per record, from its four rows and the lane's slice g of the unit's grad_out row:
//   dp = <g, bilinear>      vx = <g, d bilinear / dx>      vy = <g, d bilinear / dy>
//   grad_weights[.., l, g]          = dp summed over the D / VEC lanes of group g (a segmented scan: the groups' lanes are
//                                     contiguous runs, of any length, and a group may continue in the next chunk)
//   grad_sampling_locations[.., c]  = sum_l (w_cl, h_cl) * sum over ALL lanes of weight_g(lane) * (vx, vy)
// The sums land in the wave's LDS records (one writer lane per element; the chunks of a wide row add to them in order),
// and phase 3 writes every element of the trip once, zeros for the dropped pairs.  No atomics.
// Frozen weights and locations (grad_loc NULL): phases 1 and 3 alone, for the parked points and weights.
// ==========================================================================================
template <typename T, int VEC, int UL>
__global__ __launch_bounds__(kBlock) void msda_dfa_bwd_sample_kernel(const DfaParams p)
{
    using A = typename Traits<T>::acc;
    using TR = Traits<T>;
    using MT = ParkType<T>;
    constexpr int NU = kBlock / UL, UPW = kWave / UL;
    int b, slot;
    if (!decode_block(p.grid3d, p.B, p.nqc, p.xcd_map, b, slot)) return;
    const DfaLds<A> lds(NU, p.npc, p.rc, p.H, true);
    load_level_table(lds.tab, p.shapes, p.L);
    __syncthreads();

    const uint32_t row_bytes = (uint32_t)p.v_row;
    const rsrc_t rs = make_rsrc(static_cast<const unsigned char *>(p.value) + (size_t)b * p.I * (size_t)p.v_row, plane_span<T>(p, 0));
    const int tid = threadIdx.x, wave = tid / kWave, lane = tid % kWave;
    const int wunit = lane / UL, j = lane % UL;
    const int wa0 = slot * NU + wave * UPW;
    if (wa0 >= p.Q) return;
    const int a = wa0 + wunit;
    const bool unit_ok = a < p.Q;
    const int pairs = imul24(p.P, p.cams), G = p.H, LG = imul24(p.levels, G);
    const size_t unit0 = (size_t)b * p.Q + wa0;
    const size_t wblock = (size_t)pairs * LG;  // a unit's weights
    const T *loc = static_cast<const T *>(p.loc) + unit0 * pairs * 2;
    const T *wts0 = static_cast<const T *>(p.attn) + unit0 * wblock;
    const T *wts = wts0 + (unit_ok ? wunit : 0) * wblock;
    const float inv_lv = 1.0f / (float)p.levels, inv_cams = 1.0f / (float)p.cams;
    const int u0 = imul24(wave * UPW + wunit, p.rc);
    const int dl = min(p.D / VEC, UL);  // lanes of a group inside a chunk, at most
    const bool sample = p.grad_loc != nullptr;

    for (int p0 = 0; p0 < p.P; p0 += p.pt) {
        const int npt = min(p.pt, p.P - p0), np = imul24(npt, p.cams);
        wave_lds_sync();
        for (int fu = 0; fu < UPW && wa0 + fu < p.Q; ++fu)
            dfa_phase1<T, true, A>(p, lds, wave * UPW + fu, lane, loc + (size_t)fu * pairs * 2, p0, np, row_bytes, inv_lv, inv_cams);
        wave_lds_sync();
        // ---- phase 2 ----
        for (int ch = 0; sample && ch < p.nch; ++ch) {  // (uniform)
            if (unit_ok) {  // (idle lanes of a live unit join the sums with zeros)
                const int cbase = ch * UL * VEC, c0 = cbase + j * VEC;
                const bool lane_on = c0 < p.C;
                const uint32_t lo = lane_on ? (uint32_t)c0 * (uint32_t)sizeof(T) : 0u;
                const int gl = lane_on ? c0 / p.D : 0;
                // the run of lanes that holds group gl in this chunk: [seg_lo, seg_hi]
                const int gc0 = imul24(gl, p.D), gc1 = min(min(gc0 + p.D, p.C), cbase + UL * VEC);
                const int seg_lo = max(gc0 - cbase, 0) / VEC, seg_hi = (gc1 - cbase) / VEC - 1;
                const bool writer = lane_on && j == seg_hi, fresh = gc0 >= cbase;
                A g[VEC];
                {
                    Pack<T, VEC> pk;
#pragma unroll
                    for (int i = 0; i < VEC; ++i) pk.v[i] = TR::from_acc(0);
                    if (lane_on) pk = *reinterpret_cast<const Pack<T, VEC> *>(static_cast<const T *>(p.grad_out) + ((size_t)b * p.Q + a) * p.C + c0);
#pragma unroll
                    for (int i = 0; i < VEC; ++i) g[i] = TR::to_acc(pk.v[i]);
                }
                const int nrec = imul24(lds.cnt[wave * UPW + wunit], p.levels);
                for (int s = 0; s < nrec; s += 2) {
                    const bool two = s + 1 < nrec;
                    const int sb = two ? s + 1 : s;
                    const uint4 oa = lds.off[u0 + s], ob = lds.off[u0 + sb];
                    Pack<T, VEC> ra[4], rb[4];
                    dfa_rows<T, VEC>(rs, oa, lo, ra);
                    dfa_rows<T, VEC>(rs, ob, lo, rb);
                    const T wa = wts[lds.widx[u0 + s] + gl], wb = wts[lds.widx[u0 + sb] + gl];
                    auto take = [&](int si, const Pack<T, VEC> (&r)[4], T wt) {
                        const Rec4<A> rc = lds.rec[u0 + si];
                        const A dx = rc.v[0], dy = rc.v[1], wy0 = (A)1 - dy, wx0 = (A)1 - dx;
                        A d[4] = {0, 0, 0, 0};
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
#pragma unroll
                            for (int i = 0; i < VEC; ++i) d[k] = fma_t(g[i], TR::to_acc(r[k].v[i]), d[k]);
                        }
                        if (!lane_on) d[0] = d[1] = d[2] = d[3] = (A)0;
                        A dpv = (wy0 * wx0) * d[0] + (wy0 * dx) * d[1] + (dy * wx0) * d[2] + (dy * dx) * d[3];
                        const A m = TR::to_acc(wt);
                        const A gx = group_sum<UL>(m * (wy0 * (d[1] - d[0]) + dy * (d[3] - d[2])));
                        const A gy = group_sum<UL>(m * (wx0 * (d[2] - d[0]) + dx * (d[3] - d[1])));
                        for (int st = 1; st < dl; st <<= 1) {  // inclusive scan inside the group's run of lanes
                            const A up = __shfl_up(dpv, st, UL);
                            if (j - st >= seg_lo) dpv += up;
                        }
                        if (writer) {
                            A *dst = lds.dp + (size_t)(u0 + si) * G + gl;
                            *dst = fresh ? dpv : *dst + dpv;
                        }
                        if (j == 0) {
                            A *dst = lds.res + 2 * (size_t)(u0 + si);
                            dst[0] = ch == 0 ? rc.v[2] * gx : fma_t(rc.v[2], gx, dst[0]);
                            dst[1] = ch == 0 ? rc.v[3] * gy : fma_t(rc.v[3], gy, dst[1]);
                        }
                    };
                    take(s, ra, wa);
                    if (two) take(sb, rb, wb);
                }
            }
            wave_lds_sync();  // (the next chunk's writer lanes add to what these left)
        }
        // ---- phase 3: coalesced write-out, the wave's units one after another ----
        for (int fu = 0; fu < UPW && wa0 + fu < p.Q; ++fu) {
            const int unit = wave * UPW + fu, r0 = imul24(unit, p.rc);
            const int *pmap = lds.pmap + unit * p.npc;
            const size_t ua = unit0 + fu;
            if (sample) {
                // grad_weights: the trip's np * levels * G elements of the unit are one contiguous run
                T *gw = static_cast<T *>(p.grad_attn) + ua * wblock + (size_t)imul24(p0, p.cams) * LG;
                const float inv_LG = 1.0f / (float)LG;
                for (int f = lane; f < imul24(np, LG); f += kWave) {
                    const int pp = div_small(f, LG, inv_LG), r = f - imul24(pp, LG);
                    const int cp = pmap[pp];
                    gw[f] = TR::from_acc(cp >= 0 ? lds.dp[(size_t)(r0 + imul24(cp, p.levels)) * G + r] : (A)0);
                }
                // grad_sampling_locations: the pair's records summed over its levels, in level order
                T *gl_ = static_cast<T *>(p.grad_loc) + (ua * pairs + imul24(p0, p.cams)) * 2;
                for (int pp = lane; pp < np; pp += kWave) {
                    const int cp = pmap[pp];
                    A gx = (A)0, gy = (A)0;
                    if (cp >= 0) {
                        const A *rr = lds.res + 2 * (size_t)(r0 + imul24(cp, p.levels));
                        for (int l = 0; l < p.levels; ++l) {
                            gx += rr[2 * l];
                            gy += rr[2 * l + 1];
                        }
                    }
                    Pack<T, 2> o;
                    o.v[0] = TR::from_acc(gx);
                    o.v[1] = TR::from_acc(gy);
                    store_stream(gl_ + 2 * pp, o);
                }
            }
            if (p.mat_loc != nullptr) {
                // the pipeline's points [B, A, G, L, P, 2] and weights [B, A, G, L, P]: runs of the trip's points
                const A *ent = lds.ent + (size_t)unit * p.npc * 2;
                const T *wu = wts0 + (size_t)fu * wblock;
                const float inv_npt = 1.0f / (float)npt, inv_L = 1.0f / (float)p.L;
                for (int f = lane; f < imul24(imul24(G, p.L), npt); f += kWave) {
                    const int t = div_small(f, npt, inv_npt), pl = f - imul24(t, npt);
                    const int gq = div_small(t, p.L, inv_L), m = t - imul24(gq, p.L);
                    const int cam = div_small(m, p.levels, inv_lv), l = m - imul24(cam, p.levels);
                    const int pp = imul24(pl, p.cams) + cam;
                    const int cp = pmap[pp];
                    Pack<MT, 2> xy;
                    xy.v[0] = xy.v[1] = (MT)-2;
                    MT wv = (MT)0;
                    if (cp >= 0) {
                        xy.v[0] = ent[2 * cp];
                        xy.v[1] = ent[2 * cp + 1];
                        wv = TR::to_acc(wu[(size_t)imul24(imul24(imul24(p0, p.cams) + pp, p.levels) + l, G) + gq]);
                    }
                    const size_t sidx = ((ua * G + gq) * p.L + m) * p.P + (p0 + pl);
                    *reinterpret_cast<Pack<MT, 2> *>(static_cast<MT *>(p.mat_loc) + 2 * sidx) = xy;
                    static_cast<MT *>(p.mat_attn)[sidx] = wv;
                }
            }
        }
    }
}

}  // namespace msda
