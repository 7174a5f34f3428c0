// msda_dcn.hpp — the deformable convolution core of DCNv3 / DCNv4: the gather of the attention kernels with the pixel
// lattice as its queries.
//
//   lx = wo sw - pw + cx + s (i dw - cx + ox_k)      ly = ho sh - ph + cy + s (j dh - cy + oy_k)       k = i kh + j
//   m = softmax_k(mask) | mask                       out[n, ho, wo, g, :] = sum_k m_k bilinear(input[n, :, :, g, :], lx, ly)
//
// input [N, Hi, Wi, G, D] IS value [B, I, H, D] (one level, I = Hi Wi, H = G), a query is an output pixel (Q = Ho Wo), the
// K = kh kw taps are its samples, zero padding outside the image.  What the lattice changes, and why the family has kernels
// of its own (no other kernel, template or kernarg type knows about it):
//   * no point tensor and no level table: a sample's point follows from the unit's position, the tap and (ox, oy)
//   * offsets and mask are read in place through (row stride, group stride) pairs — DCNv3's two dense tensors and
//     DCNv4's packed offset_mask alike — and their gradients are written through the same strides
//   * a workgroup serves an 8 x 8 TILE of output pixels of one image and a block of `gblk` groups.  Square, because the
//     input window under a tile grows with its perimeter; 64 pixels, because with the 4-lane units of a D = 16 stage one
//     trip of the 256 threads is then one group of the whole tile, and a tile row of 8 pixels x gblk groups x 64 bytes is
//     the run a wave reads or writes contiguously.  Neighbouring slots are the group blocks of ONE tile, then the next
//     tile of the row: what is resident together shares input rows in L2.
//   * the tile's taps at zero offsets cover a known window of the input — (8 - 1) stride + dilation (k - 1) + 1 pixels,
//     plus the second corner, plus a halo of kDcnHalo on every side.  With Params-side `win` the workgroup stages that
//     window of its group block in LDS once, and every bilinear corner inside it is served from there; every other corner
//     goes through the buffer descriptor.  Both paths deliver the pixel's stored bits, a corner dropped by zero padding
//     reads 0 on either (it is never marked as in the window), and the arithmetic behind the rows is the same code: the
//     results are the same bits with the window on or off.
//
//   forward           msda_dcn_fwd_kernel         out; the softmax over K in the accumulate type
//   sample gradients  msda_dcn_bwd_sample_kernel  grad_offset, grad_mask (through the softmax), and — parked for the passes
//                     below — every sample's normalised point and post-softmax weight, in ParkType
//   input gradient    the grad_value pipelines as they are (msda_value_sorted.hpp / msda_value_small.hpp), L = 1, weights
//                     the parked m, rows grad_out
//
// ONE definition of a sample's cell.  The pipeline finds a sample's cell from a parked NORMALISED point through
// sample_cell: px = fma(x, W, -0.5), floor, fractions px - floor.  `x W - 0.5` does not invert `(lx + 0.5) / W` in floating
// point, so no kernel here derives a cell from lx: dcn_point forms x = (lx + 0.5) (1 / W) ONCE per sample in the accumulate
// type (every operation explicit: one fma, one add, one multiply — nothing for -ffp-contract to fuse differently in two
// inlined copies), dcn_taps derives cell and fractions from that x with sample_cell's own expression, and the sample kernel
// parks exactly that x.  Forward, sample gradients and the pipeline therefore agree bit for bit on cell and fractions.
//
// Phases as the other gather kernels': 1 (per wave, one sample per lane and trip) point, taps and weights into the wave's
// LDS records; 2 (per unit, G lanes x VEC channels) the rows and the arithmetic; 3 (backward, per wave) coalesced
// write-out.  All K samples of a unit are parked at once (the softmax wants them together): K is bounded by the LDS.
#pragma once

#include "msda_kernels.hpp"

namespace msda {

constexpr int kDcnTile = 8;                      // output pixels per tile side
constexpr int kDcnHalo = 1;                      // window pixels beyond the zero-offset taps, every side
constexpr uint32_t kDcnLdsTag = 0xC0000000u;     // a record offset at or above it: window byte offset in the low 30 bits

// The kernarg: Params (value = input, B = N, I = Hi Wi, H = G, Q = Ho Wo, L = 1, P = LP = K, v_row, out, grad_out,
// mat_loc / mat_attn = the parked points / weights) and, BEHIND it, what only this family has.
struct DcnParams : Params {
    const void *off, *msk;  // offsets: element (row r, group g, tap k) at off[r off_row + g off_grp + 2 k (+ 1)]; mask likewise
    void *g_off, *g_msk;    // their gradients, through the same strides (backward; NULL: not asked for)
    int64_t off_row, off_grp, msk_row, msk_grp;
    int64_t *park_shapes;   // backward: (Hi, Wi) for the pipeline's level table, written by the sample kernel
    double s;               // offset_scale, cast once to the accumulate type
    double inv_w, inv_h;    // 1 / Wi, 1 / Hi (dcn_point)
    int Hi, Wi, Ho, Wo, kh, kw, sh, sw, ph, pw, dh, dw;
    int softmax;
    int tiles_x, gblk, ngb;      // tiles per row of tiles, groups per block, group blocks
    int win, win_w, win_h;       // the staged window: on / off, its extent in pixels
    uint32_t win_off, win_row;   // ... its first byte in the dynamic LDS, bytes per window pixel (gblk D sizeof)
};

// what a workgroup serves, from its slot: group block fastest, then the tile along the row
struct DcnTileOf {
    int g0, ho0, wo0;    // first group, first output pixel
    int wx0, wy0;        // input pixel under the window's corner
};
__device__ __forceinline__ DcnTileOf dcn_tile_of(const DcnParams &p, int slot)
{
    DcnTileOf t;
    const int tile = slot / p.ngb, gb = slot - tile * p.ngb;
    const int ty = tile / p.tiles_x, tx = tile - ty * p.tiles_x;
    t.g0 = gb * p.gblk;
    t.ho0 = ty * kDcnTile;
    t.wo0 = tx * kDcnTile;
    t.wx0 = t.wo0 * p.sw - p.pw - kDcnHalo;  // (tap i of pixel wo at zero offset and s = 1: wo sw - pw + i dw)
    t.wy0 = t.ho0 * p.sh - p.ph - kDcnHalo;
    return t;
}
// unit u of the workgroup: pixel-major, the block's groups innermost (their rows are neighbours in memory)
struct DcnUnit {
    int ho, wo, g, gl;
    bool ok;
};
__device__ __forceinline__ DcnUnit dcn_unit(const DcnParams &p, const DcnTileOf &t, int u, float inv_gblk)
{
    DcnUnit n;
    const int pix = div_small(u, p.gblk, inv_gblk);
    n.gl = u - imul24(pix, p.gblk);
    n.g = t.g0 + n.gl;
    n.ho = t.ho0 + pix / kDcnTile;
    n.wo = t.wo0 + pix % kDcnTile;
    n.ok = pix < kDcnTile * kDcnTile && n.ho < p.Ho && n.wo < p.Wo && n.g < p.H;
    return n;
}

// The sample's normalised point — THE value every consumer derives its cell from (header).  t: the tap's place in the
// window minus the centre plus the learned offset; base: the pixel's own term, an integer.
template <typename A> __device__ __forceinline__ A dcn_point(A s, A tap, A o, A base, A inv_n)
{
    const A l = fma_t(s, tap + o, base);
    return (l + (A)0.5) * inv_n;
}

template <typename A> struct DcnTaps {
    uint32_t off[4];  // 00 (y0, x0), 01 (y0, x1), 10 (y1, x0), 11 (y1, x1): byte offset of the pixel's rows in the image,
                      // kMaskedOffset for a corner outside it, kDcnLdsTag | window offset for a staged one
    A dx, dy;
};
// sample_cell's arithmetic (msda_value_sorted.hpp: the explicit fma, floor, px - floor) on the point of dcn_point
template <typename A>
__device__ __forceinline__ void dcn_taps(A x, A y, const DcnParams &p, const DcnTileOf &tl, uint32_t row_bytes, DcnTaps<A> &t)
{
    const A W = (A)p.Wi, Hh = (A)p.Hi;
    const A px = fma_t(x, W, (A)-0.5), py = fma_t(y, Hh, (A)-0.5);
    const A x0 = floor_t(px), y0 = floor_t(py);
    t.dx = px - x0;
    t.dy = py - y0;
    // a cell with a pixel in the image has its corner 00 in [-1, n - 1]; anything else (NaN too) touches nothing
    const bool any = x0 >= (A)-1 && x0 <= W - (A)1 && y0 >= (A)-1 && y0 <= Hh - (A)1;
    const int ix = (int)fmin_t(fmax_t(x0, (A)-1), W), iy = (int)fmin_t(fmax_t(y0, (A)-1), Hh);  // (clamped before the conversion)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int cx = ix + (k & 1), cy = iy + (k >> 1);
        uint32_t o = kMaskedOffset;
        if (any && cx >= 0 && cx < p.Wi && cy >= 0 && cy < p.Hi) {
            o = mul24((uint32_t)imul24(cy, p.Wi) + (uint32_t)cx, row_bytes);
            const int wx = cx - tl.wx0, wy = cy - tl.wy0;
            if (p.win && wx >= 0 && wx < p.win_w && wy >= 0 && wy < p.win_h)
                o = kDcnLdsTag | mul24((uint32_t)imul24(wy, p.win_w) + (uint32_t)wx, p.win_row);
        }
        t.off[k] = o;
    }
}

// One corner's rows for this lane: from the window when the record says so, else through the descriptor (a masked
// corner's offset is out of range there: zeros).  Both loads are issued and one is kept — no divergent branch; the
// descriptor answers the unused one without a memory access, the window read of a corner outside it goes to the window's
// first pixel.  `win` is uniform.
template <typename T, int VEC>
__device__ __forceinline__ Pack<T, VEC> dcn_row(rsrc_t rs, uint32_t off, uint32_t lo_img, uint32_t lo_win, bool win)
{
    using RL = RawLoad<sizeof(T) * VEC>;
    const bool staged = win && off >= kDcnLdsTag;
    Pack<T, VEC> r = __builtin_bit_cast(Pack<T, VEC>, RL::load(rs, staged ? kMaskedOffset : off + lo_img));
    if (win) {
        const Pack<T, VEC> l = *reinterpret_cast<const Pack<T, VEC> *>(msda_smem + ((staged ? (off & ~kDcnLdsTag) : 0u) + lo_win));
        if (staged) r = l;
    }
    return r;
}

// The window of the workgroup's group block, image -> LDS, in pieces of VEC elements; pixels of the window outside the
// image are not staged (no corner refers to them).  Ends with the block barrier: every thread of the workgroup calls it.
template <typename T, int VEC>
__device__ __forceinline__ void dcn_stage_window(const DcnParams &p, const DcnTileOf &tl, rsrc_t rs)
{
    using RL = RawLoad<sizeof(T) * VEC>;
    const int ng = min(p.gblk, p.H - tl.g0);
    const int per = imul24(ng, p.D) / VEC;  // pieces per pixel
    const int total = imul24(imul24(p.win_w, p.win_h), per);
    const float inv_per = 1.0f / (float)per, inv_ww = 1.0f / (float)p.win_w;
    const uint32_t g_bytes = (uint32_t)imul24(tl.g0, p.D) * (uint32_t)sizeof(T);
    for (int f = threadIdx.x; f < total; f += kBlock) {
        const int wp = div_small(f, per, inv_per), c = f - imul24(wp, per);
        const int wy = div_small(wp, p.win_w, inv_ww), wx = wp - imul24(wy, p.win_w);
        const int ix = tl.wx0 + wx, iy = tl.wy0 + wy;
        if (ix >= 0 && ix < p.Wi && iy >= 0 && iy < p.Hi) {
            const uint32_t piece = (uint32_t)c * (uint32_t)(sizeof(T) * VEC);
            const typename RL::type v = RL::load(rs, mul24((uint32_t)imul24(iy, p.Wi) + (uint32_t)ix, (uint32_t)p.v_row) + g_bytes + piece);
            *reinterpret_cast<typename RL::type *>(msda_smem + p.win_off + mul24((uint32_t)wp, p.win_row) + piece) = v;
        }
    }
    __syncthreads();
}

// the records of a workgroup: `slots` = units per trip x K
template <typename A> struct DcnPoint {
    A x, y;
};
template <typename A> struct DcnLds {
    uint4 *off;
    Rec4<A> *rec;
    A *z;             // the raw mask value; backward: + one scalar per unit behind the slots
    DcnPoint<A> *pt;  // backward only
    __device__ __forceinline__ DcnLds(int slots, int units)
    {
        off = reinterpret_cast<uint4 *>(msda_smem);
        rec = reinterpret_cast<Rec4<A> *>(off + slots);
        z = reinterpret_cast<A *>(rec + slots);
        pt = reinterpret_cast<DcnPoint<A> *>(z + slots + units);
    }
};

// the softmax over a unit's K parked mask values, every lane of the unit for itself (the same bits on each): the maximum
// and 1 / sum exp(z - max) in the accumulate type.  m_k = exp(z_k - mx) * inv.
template <typename A> __device__ __forceinline__ void dcn_softmax_stats(const A *z, int K, A &mx, A &inv)
{
    mx = z[0];
    for (int k = 1; k < K; ++k) mx = fmax_t(mx, z[k]);
    A sum = (A)0;
    for (int k = 0; k < K; ++k) sum += exp_t(z[k] - mx);
    inv = (A)1 / sum;
}

// phase 1 of both kernels: sample f of the wave's trip -> its record.  Returns the point through (x, y).
template <typename T, typename A>
__device__ __forceinline__ void dcn_sample(const DcnParams &p, const DcnTileOf &tl, const DcnUnit &un, int n, int k, float inv_kh,
                                           uint32_t row_bytes, DcnTaps<A> &t, A &x, A &y, A &z)
{
    using TR = Traits<T>;
    const size_t row = (size_t)n * p.Q + (size_t)(imul24(un.ho, p.Wo) + un.wo);
    const T *po = static_cast<const T *>(p.off) + (row * p.off_row + (size_t)un.g * p.off_grp + 2 * k);
    const A ox = TR::to_acc(po[0]), oy = TR::to_acc(po[1]);
    z = TR::to_acc(static_cast<const T *>(p.msk)[row * p.msk_row + (size_t)un.g * p.msk_grp + k]);
    const int i = div_small(k, p.kh, inv_kh), j = k - imul24(i, p.kh);  // i: the window's column (outer), j: its row
    const int cx = (p.dw * (p.kw - 1)) / 2, cy = (p.dh * (p.kh - 1)) / 2;
    x = dcn_point<A>((A)p.s, (A)(i * p.dw - cx), ox, (A)(un.wo * p.sw - p.pw + cx), (A)p.inv_w);
    y = dcn_point<A>((A)p.s, (A)(j * p.dh - cy), oy, (A)(un.ho * p.sh - p.ph + cy), (A)p.inv_h);
    dcn_taps<A>(x, y, p, tl, row_bytes, t);
}

// ==========================================================================================
// forward
// ==========================================================================================
template <typename T, int VEC, int G>
__global__ __launch_bounds__(kBlock) void msda_dcn_fwd_kernel(const DcnParams p)
{
    using A = typename Traits<T>::acc;
    using TR = Traits<T>;
    constexpr int NU = kBlock / G, UPW = kWave / G;
    int n, slot;
    if (!decode_block(p.grid3d, p.B, p.nqc, p.xcd_map, n, slot)) return;
    const DcnTileOf tl = dcn_tile_of(p, slot);
    const uint32_t row_bytes = (uint32_t)p.v_row;
    const rsrc_t rs = make_rsrc(static_cast<const unsigned char *>(p.value) + (size_t)n * p.I * (size_t)p.v_row, (uint32_t)p.I * row_bytes);
    const bool win = p.win != 0;
    if (win) dcn_stage_window<T, VEC>(p, tl, rs);

    const int K = p.P;
    const DcnLds<A> lds(NU * K, 0);
    const int tid = threadIdx.x, wave = tid / kWave, lane = tid % kWave;
    const int wunit = lane / G, j = lane % G;
    uint4 *w_off = lds.off + wave * UPW * K;
    Rec4<A> *w_rec = lds.rec + wave * UPW * K;
    A *w_z = lds.z + wave * UPW * K;
    const float inv_K = 1.0f / (float)K, inv_kh = 1.0f / (float)p.kh, inv_gblk = 1.0f / (float)p.gblk;
    const int c0 = j * VEC;
    const bool lane_on = c0 < p.D;
    const int units = kDcnTile * kDcnTile * p.gblk;

    for (int wu0 = wave * UPW; wu0 < units; wu0 += NU) {  // (wave-uniform: no block barrier below)
        wave_lds_sync();  // previous records consumed
        // ---- phase 1 ----
        for (int f = lane; f < UPW * K; f += kWave) {
            const int fu = div_small(f, K, inv_K), k = f - imul24(fu, K);
            const DcnUnit un = dcn_unit(p, tl, wu0 + fu, inv_gblk);
            if (un.ok) {
                DcnTaps<A> t;
                A x, y, z;
                dcn_sample<T, A>(p, tl, un, n, k, inv_kh, row_bytes, t, x, y, z);
                const A wy0 = (A)1 - t.dy, wx0 = (A)1 - t.dx;
                Rec4<A> w;
                w.v[0] = wy0 * wx0;
                w.v[1] = wy0 * t.dx;
                w.v[2] = t.dy * wx0;
                w.v[3] = t.dy * t.dx;
                w_off[f] = make_uint4(t.off[0], t.off[1], t.off[2], t.off[3]);
                w_rec[f] = w;
                w_z[f] = z;
            }
        }
        wave_lds_sync();
        // ---- phase 2: two samples' rows in flight ----
        const DcnUnit un = dcn_unit(p, tl, wu0 + wunit, inv_gblk);
        if (un.ok) {
            const int u0 = imul24(wunit, K);
            const uint32_t lo_chan = (uint32_t)(lane_on ? c0 : 0) * (uint32_t)sizeof(T);
            const uint32_t lo_img = (uint32_t)imul24(un.g, p.D) * (uint32_t)sizeof(T) + lo_chan;
            const uint32_t lo_win = p.win_off + (uint32_t)imul24(un.gl, p.D) * (uint32_t)sizeof(T) + lo_chan;
            A mx = (A)0, inv = (A)1;
            if (p.softmax) dcn_softmax_stats<A>(w_z + u0, K, mx, inv);
            A acc[VEC];
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc[i] = (A)0;
            for (int s = 0; s < K; s += 2) {
                const bool two = s + 1 < K;  // (uniform)
                const int sb = two ? s + 1 : s;
                const uint4 oa = w_off[u0 + s], ob = w_off[u0 + sb];
                Pack<T, VEC> ra[4], rb[4];
                ra[0] = dcn_row<T, VEC>(rs, oa.x, lo_img, lo_win, win);
                ra[1] = dcn_row<T, VEC>(rs, oa.y, lo_img, lo_win, win);
                ra[2] = dcn_row<T, VEC>(rs, oa.z, lo_img, lo_win, win);
                ra[3] = dcn_row<T, VEC>(rs, oa.w, lo_img, lo_win, win);
                rb[0] = dcn_row<T, VEC>(rs, ob.x, lo_img, lo_win, win);
                rb[1] = dcn_row<T, VEC>(rs, ob.y, lo_img, lo_win, win);
                rb[2] = dcn_row<T, VEC>(rs, ob.z, lo_img, lo_win, win);
                rb[3] = dcn_row<T, VEC>(rs, ob.w, lo_img, lo_win, win);
                auto take = [&](int si, const Pack<T, VEC> (&r)[4]) {
                    const Rec4<A> w = w_rec[u0 + si];
                    const A zz = w_z[u0 + si];
                    const A m = p.softmax ? exp_t(zz - mx) * inv : zz;
#pragma unroll
                    for (int i = 0; i < VEC; ++i) {
                        A v = w.v[0] * TR::to_acc(r[0].v[i]);
                        v = fma_t(w.v[1], TR::to_acc(r[1].v[i]), v);
                        v = fma_t(w.v[2], TR::to_acc(r[2].v[i]), v);
                        v = fma_t(w.v[3], TR::to_acc(r[3].v[i]), v);
                        acc[i] = fma_t(m, v, acc[i]);
                    }
                };
                take(s, ra);
                if (two) take(sb, rb);
            }
            if (lane_on) {
                Pack<T, VEC> o;
#pragma unroll
                for (int i = 0; i < VEC; ++i) o.v[i] = TR::from_acc(acc[i]);
                const size_t q = (size_t)n * p.Q + (size_t)(imul24(un.ho, p.Wo) + un.wo);
                store_stream(static_cast<T *>(p.out) + (q * p.H + un.g) * p.D + c0, o);
            }
        }
    }
}

// ==========================================================================================
// backward, the sample half.  The unit's row of grad_out (g) stays in registers.  Per sample, from its four rows:
//   dp = <g, bilinear>      vx = <g, d bilinear / dx>      vy = <g, d bilinear / dy>        (three group sums)
// and with c = sum_k m_k dp_k (softmax on):
//   grad_mask_k = m_k (dp_k - c) | dp_k      grad_offset_k = s m_k (vx, vy)    — lx, ly are pixel coordinates: no W, H factor
// Phase 3 writes them through the offsets' and the mask's own strides, one sample per lane, and parks (x, y) and m.
// Every element has one writer; no atomics.
// ==========================================================================================
template <typename T, int VEC, int G>
__global__ __launch_bounds__(kBlock) void msda_dcn_bwd_sample_kernel(const DcnParams p)
{
    using A = typename Traits<T>::acc;
    using TR = Traits<T>;
    using MT = ParkType<T>;
    constexpr int NU = kBlock / G, UPW = kWave / G;
    if (p.park_shapes != nullptr && blockIdx.x + blockIdx.y + blockIdx.z == 0 && threadIdx.x == 0) {
        p.park_shapes[0] = p.Hi;
        p.park_shapes[1] = p.Wi;
    }
    int n, slot;
    if (!decode_block(p.grid3d, p.B, p.nqc, p.xcd_map, n, slot)) return;
    const DcnTileOf tl = dcn_tile_of(p, slot);
    const uint32_t row_bytes = (uint32_t)p.v_row;
    const rsrc_t rs = make_rsrc(static_cast<const unsigned char *>(p.value) + (size_t)n * p.I * (size_t)p.v_row, (uint32_t)p.I * row_bytes);
    const bool win = p.win != 0;
    if (win) dcn_stage_window<T, VEC>(p, tl, rs);

    const int K = p.P;
    const DcnLds<A> lds(NU * K, NU);
    const int tid = threadIdx.x, wave = tid / kWave, lane = tid % kWave;
    const int wunit = lane / G, j = lane % G;
    uint4 *w_off = lds.off + wave * UPW * K;
    Rec4<A> *w_rec = lds.rec + wave * UPW * K;  // in: {dx, dy, -, -}; out: {dp, vx, vy, m}
    A *w_z = lds.z + wave * UPW * K;
    A *w_c = lds.z + NU * K + wave * UPW;
    DcnPoint<A> *w_pt = lds.pt + wave * UPW * K;
    const float inv_K = 1.0f / (float)K, inv_kh = 1.0f / (float)p.kh, inv_gblk = 1.0f / (float)p.gblk;
    const int c0 = j * VEC;
    const bool lane_on = c0 < p.D;
    const int units = kDcnTile * kDcnTile * p.gblk;
    const A sA = (A)p.s;

    for (int wu0 = wave * UPW; wu0 < units; wu0 += NU) {
        wave_lds_sync();
        // ---- phase 1 ----
        for (int f = lane; f < UPW * K; f += kWave) {
            const int fu = div_small(f, K, inv_K), k = f - imul24(fu, K);
            const DcnUnit un = dcn_unit(p, tl, wu0 + fu, inv_gblk);
            if (un.ok) {
                DcnTaps<A> t;
                DcnPoint<A> pt;
                A z;
                dcn_sample<T, A>(p, tl, un, n, k, inv_kh, row_bytes, t, pt.x, pt.y, z);
                Rec4<A> r;
                r.v[0] = t.dx;
                r.v[1] = t.dy;
                r.v[2] = r.v[3] = (A)0;
                w_off[f] = make_uint4(t.off[0], t.off[1], t.off[2], t.off[3]);
                w_rec[f] = r;
                w_z[f] = z;
                w_pt[f] = pt;
            }
        }
        wave_lds_sync();
        // ---- phase 2 ----
        const DcnUnit un = dcn_unit(p, tl, wu0 + wunit, inv_gblk);
        if (un.ok) {  // (idle lanes of a live unit join the group sums with zeros)
            const int u0 = imul24(wunit, K);
            const uint32_t lo_chan = (uint32_t)(lane_on ? c0 : 0) * (uint32_t)sizeof(T);
            const uint32_t lo_img = (uint32_t)imul24(un.g, p.D) * (uint32_t)sizeof(T) + lo_chan;
            const uint32_t lo_win = p.win_off + (uint32_t)imul24(un.gl, p.D) * (uint32_t)sizeof(T) + lo_chan;
            const size_t q = (size_t)n * p.Q + (size_t)(imul24(un.ho, p.Wo) + un.wo);
            A g[VEC];
            {
                Pack<T, VEC> pk;
#pragma unroll
                for (int i = 0; i < VEC; ++i) pk.v[i] = TR::from_acc(0);
                if (lane_on) pk = *reinterpret_cast<const Pack<T, VEC> *>(static_cast<const T *>(p.grad_out) + (q * p.H + un.g) * p.D + c0);
#pragma unroll
                for (int i = 0; i < VEC; ++i) g[i] = TR::to_acc(pk.v[i]);
            }
            A mx = (A)0, inv = (A)1;
            if (p.softmax) dcn_softmax_stats<A>(w_z + u0, K, mx, inv);
            A c = (A)0;
            for (int s = 0; s < K; s += 2) {
                const bool two = s + 1 < K;  // (uniform)
                const int sb = two ? s + 1 : s;
                const uint4 oa = w_off[u0 + s], ob = w_off[u0 + sb];
                Pack<T, VEC> ra[4], rb[4];
                ra[0] = dcn_row<T, VEC>(rs, oa.x, lo_img, lo_win, win);
                ra[1] = dcn_row<T, VEC>(rs, oa.y, lo_img, lo_win, win);
                ra[2] = dcn_row<T, VEC>(rs, oa.z, lo_img, lo_win, win);
                ra[3] = dcn_row<T, VEC>(rs, oa.w, lo_img, lo_win, win);
                rb[0] = dcn_row<T, VEC>(rs, ob.x, lo_img, lo_win, win);
                rb[1] = dcn_row<T, VEC>(rs, ob.y, lo_img, lo_win, win);
                rb[2] = dcn_row<T, VEC>(rs, ob.z, lo_img, lo_win, win);
                rb[3] = dcn_row<T, VEC>(rs, ob.w, lo_img, lo_win, win);
                auto take = [&](int si, const Pack<T, VEC> (&r)[4]) {
                    const Rec4<A> rc = w_rec[u0 + si];
                    const A zz = w_z[u0 + si];
                    const A m = p.softmax ? exp_t(zz - mx) * inv : zz;
                    const A dx = rc.v[0], dy = rc.v[1], wy0 = (A)1 - dy, wx0 = (A)1 - dx;
                    A d[4] = {0, 0, 0, 0};
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
#pragma unroll
                        for (int i = 0; i < VEC; ++i) d[k] = fma_t(g[i], TR::to_acc(r[k].v[i]), d[k]);
                    }
                    if (!lane_on) d[0] = d[1] = d[2] = d[3] = (A)0;
                    A dp = (wy0 * wx0) * d[0] + (wy0 * dx) * d[1] + (dy * wx0) * d[2] + (dy * dx) * d[3];
                    A vx = wy0 * (d[1] - d[0]) + dy * (d[3] - d[2]), vy = wx0 * (d[2] - d[0]) + dx * (d[3] - d[1]);
                    dp = group_sum<G>(dp);
                    vx = group_sum<G>(vx);
                    vy = group_sum<G>(vy);
                    c = fma_t(m, dp, c);
                    if (j == 0) {
                        Rec4<A> res;
                        res.v[0] = dp;
                        res.v[1] = vx;
                        res.v[2] = vy;
                        res.v[3] = m;
                        w_rec[u0 + si] = res;
                    }
                };
                take(s, ra);
                if (two) take(sb, rb);
            }
            if (j == 0) w_c[wunit] = c;
        }
        wave_lds_sync();
        // ---- phase 3: coalesced write-out, one sample per lane and trip ----
        for (int f = lane; f < UPW * K; f += kWave) {
            const int fu = div_small(f, K, inv_K), k = f - imul24(fu, K);
            const DcnUnit un = dcn_unit(p, tl, wu0 + fu, inv_gblk);
            if (un.ok) {
                const Rec4<A> res = w_rec[f];
                const A m = res.v[3];
                const size_t row = (size_t)n * p.Q + (size_t)(imul24(un.ho, p.Wo) + un.wo);
                if (p.g_off != nullptr) {
                    T *go = static_cast<T *>(p.g_off) + (row * p.off_row + (size_t)un.g * p.off_grp + 2 * k);
                    const A sm = sA * m;
                    go[0] = TR::from_acc(sm * res.v[1]);
                    go[1] = TR::from_acc(sm * res.v[2]);
                    static_cast<T *>(p.g_msk)[row * p.msk_row + (size_t)un.g * p.msk_grp + k] =
                        TR::from_acc(p.softmax ? m * (res.v[0] - w_c[fu]) : res.v[0]);
                }
                if (p.mat_loc != nullptr) {  // (the input is not frozen: point and weight for the grad_value passes)
                    const size_t sidx = (row * p.H + un.g) * K + k;
                    const DcnPoint<A> pt = w_pt[f];
                    Pack<MT, 2> xy;
                    xy.v[0] = pt.x;
                    xy.v[1] = pt.y;
                    *reinterpret_cast<Pack<MT, 2> *>(static_cast<MT *>(p.mat_loc) + 2 * sidx) = xy;
                    static_cast<MT *>(p.mat_attn)[sidx] = m;
                }
            }
        }
    }
}

}  // namespace msda
