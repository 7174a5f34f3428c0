// msda_launch.hpp — host side of the C ABI: argument checks, variant selection, launches.
// One translation unit per storage dtype instantiates run_fwd<T> / run_bwd<T> (msda_<dtype>.hip).
#pragma once

#include <stdio.h>

#include <atomic>
#include <initializer_list>

#include "msda_value_sorted.hpp"
#include "msda_value_place.hpp"
#include "msda_value_small.hpp"
#include "msda_discrete.hpp"
#include "msda_hfbox_discrete.hpp"
#include "msda_options.hpp"

namespace msda {

// ---- per-thread error text, side stream and measurement hooks (defined in msda_api.hip; the options: msda_options.hpp) ----
// fork-join helpers around a lazily created per-device side stream (msda_api.hip)
hipStream_t side_stream_fork(hipStream_t user);   // side stream that waits for everything queued on `user`
int side_stream_join(hipStream_t user);            // `user` waits for everything queued on the side stream
void set_error(const char *fmt, ...);
// measurement only (msda_last_launch_info): slot 0-3 forward {variant 0 plain / 1 LDS-served levels / 2 one wave per unit, LDS level
// bytes, planes per workgroup, workgroups}, 4-5 sample gradients {variant, LDS level bytes}, 6 grad_value path (1 single launch,
// 2 sorted pipeline), 7 its passes over the batch
void note_launch(int slot, int value);
// ... and WHICH template instantiation a launch runs: VEC channels per lane, G lanes per unit, ceil(D / (G * VEC)) channel
// chunks — slots 8-10 the forward ("fwd_vec", "fwd_group", "fwd_chunks"), 11-13 the sample gradients, 14-16 grad_value (the
// single-launch kernel or the sorted gather + finish).  For tests: a changed threshold must not turn a G = 64 case into a G = 16 one.
inline void note_instance(int first_slot, int vec, int group, int D)
{
    note_launch(first_slot, vec);
    note_launch(first_slot + 1, group);
    note_launch(first_slot + 2, (D + group * vec - 1) / (group * vec));
}
// ... and how many passes the launch makes over a unit's S samples: ceil(S / sc), sc samples parked per trip (plan_gather, the
// LDS-served-level plan) or taken per trip by a wave's 64 / U lanes (the one-wave-per-unit forward) — slot 23 the forward
// ("fwd_trips"), 24 the sample gradients ("sample_trips"); 1 for the discrete kernels, which park nothing.  For tests: a moved
// cap must not turn a three-trip case into a one-trip one.
inline void note_trips(int slot, int S, int sc) { note_launch(slot, sc > 0 ? (S + sc - 1) / sc : 0); }
// ... and which grid form plane_grid gave a launch: 0 XCD-aware 3-D, 1 linear 2-D, 2 flat 1-D — one process-wide counter per
// form that only ever rises ("grid_xcd3d_launches", "grid_linear2d_launches", "grid_flat_launches"; callers take differences)
void note_grid(int form);
// measurement only (option "profile"): an event pair around a kernel launch, read back by msda_profile_read
void *profile_begin(const char *name, hipStream_t stream);
void profile_end(void *token, hipStream_t stream);
struct ProfileScope {
    void *token;
    hipStream_t stream;
    ProfileScope(const char *name, hipStream_t s) : token(profile_begin(name, s)), stream(s) {}
    ~ProfileScope() { profile_end(token, stream); }
};
constexpr int kRecordLdsBudget = 48 * 1024;                // per workgroup, parked sample records
constexpr int kMaxDynLds = 160 * 1024 - 2048;  // leaves room for small static __shared__ objects

inline bool aligned_to(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }

// Kernels that may ask for more than 64 KiB of dynamic LDS need the attribute raised once per (kernel, DEVICE): a
// process that drives several GPUs must not skip it on the second one.  `done` is the caller's per-kernel bitmask
// of devices already served (idempotent: a lost race only repeats the call).
template <typename K> inline void allow_big_lds(K kernel, std::atomic<uint64_t> &done)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) dev = 0;
    const uint64_t bit = 1ull << (dev & 63);
    if (dev < 64 && (done.load(std::memory_order_relaxed) & bit)) return;
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            kMaxDynLds) != hipSuccess)
        (void)hipGetLastError();  // do not let a refused attribute poison the next launch check
    if (dev < 64) done.fetch_or(bit, std::memory_order_relaxed);
}

struct Dims {
    int64_t B, I, H, D, Q, L, P;
    int64_t cells = 0;  // the caller's max_level_cells argument: no level has more bilinear cells (0: unknown)
    int64_t S = 0;      // samples per (b, q, h) unit with per-level point counts (P is then their maximum); 0: L * P
};
inline int64_t samples(const Dims &d) { return d.S > 0 ? d.S : d.L * d.P; }
// ... or the process-wide promise (msda_set_option("level_cells", n)); 0: unknown
inline int64_t level_cells_bound(const Dims &d) { return d.cells > 0 ? d.cells : (int64_t)option_level_cells(); }

// The size limits behind the 32-bit plane offsets ("Size limits"); `es`: size of the arithmetic / sampling
// type.  One definition for the entry points (check_common) and the workspace queries, which answer 0 where a call
// would be refused.
inline bool common_limits_exceeded(const Dims &d, int64_t es)
{
    const int64_t lim = (int64_t)1 << 31;
    return d.I * d.H * d.D * es >= lim || d.B >= lim || d.Q >= lim || samples(d) >= (1 << 22) || d.B * d.H >= (1 << 28) ||
           d.Q * d.H * samples(d) * 2 >= lim || d.Q * d.H * d.D * es >= lim || d.I >= (1 << 24) || d.Q >= (1 << 24) ||
           d.H * samples(d) >= (1 << 24) || d.H * d.D * es >= (1 << 24);
}
// ... and of the fused entry points' projection [B, Q, H, S, 3]
inline bool fused_limit_exceeded(const Dims &d) { return d.Q * d.H * samples(d) * 3 >= ((int64_t)1 << 31); }

// ---- the shared steps of an entry point, part 1 (part 2: behind fill_params).  Every run_* applies them in its OWN order,
//      and that order is contract (which of two faults a call reports): see the run_* bodies and DESIGN.md 1. ----
// dimensions, padding mode, level count, size limits (`es`: size of the arithmetic / sampling type)
inline int check_common(const Dims &d, int64_t es, int padding_mode)
{
    if (d.B < 0 || d.I < 0 || d.H < 0 || d.D < 0 || d.Q < 0 || d.L < 0 || d.P < 0) {
        set_error("negative dimension");
        return MSDA_ERR_BAD_ARG;
    }
    if (padding_mode != MSDA_PADDING_BORDER && padding_mode != MSDA_PADDING_ZEROS) {
        set_error("unknown padding_mode %d", padding_mode);
        return MSDA_ERR_BAD_ARG;
    }
    if (d.L > MSDA_MAX_LEVELS) {
        set_error("L=%lld exceeds MSDA_MAX_LEVELS=%d", (long long)d.L, MSDA_MAX_LEVELS);
        return MSDA_ERR_TOO_MANY_LEVELS;
    }
    if (common_limits_exceeded(d, es)) {
        set_error("tensor too large for 32-bit plane offsets (I*H*D*sizeof = %lld bytes)", (long long)(d.I * d.H * d.D * es));
        return MSDA_ERR_TOO_LARGE;
    }
    return 0;
}
// buffers a call cannot do without (the index in the message counts within the list)
inline int require_buffers(std::initializer_list<const void *> ptrs)
{
    int i = 0;
    for (const void *ptr : ptrs) {
        if (ptr == nullptr) {
            set_error("null buffer (argument %d)", i);
            return MSDA_ERR_BAD_ARG;
        }
        ++i;
    }
    return 0;
}
// every buffer on a multiple of its element size (a null pointer, an output not asked for, passes)
struct AlignedTo {
    const void *ptr;
    size_t bytes;
};
inline int check_aligned(std::initializer_list<AlignedTo> bufs)
{
    for (const AlignedTo &b : bufs) {
        if (aligned_to(b.ptr, b.bytes)) continue;
        set_error("misaligned buffer");
        return MSDA_ERR_MISALIGNED;
    }
    return 0;
}
// the empty-problem shortcut: zeros into every output that was asked for and has bytes
struct ZeroFill {
    void *ptr;
    size_t bytes;
};
inline int zero_outputs(std::initializer_list<ZeroFill> outs, hipStream_t stream)
{
    hipError_t e = hipSuccess;
    for (const ZeroFill &o : outs)
        if (e == hipSuccess && o.ptr != nullptr && o.bytes != 0) e = hipMemsetAsync(o.ptr, 0, o.bytes, stream);
    return (int)e;
}
// no sample touches anything: all gradients are zero
inline bool nothing_sampled(const Dims &d) { return d.B * d.Q * d.H * d.D == 0 || samples(d) == 0 || d.I == 0; }

// Grid for a (plane, slot) decomposition.  Prefers the 3-D shapes whose linear dispatch order equals
// decode_block's 1-D formula, so the kernel needs no integer division; falls back to 1-D when a
// dimension would exceed the 65535 limit.  Returns false if even the 1-D grid is too large.
// Which workgroups share an XCD (decode_block): by default the planes stay on "their" XCD (xcd_map 1) so that its L2 holds
// few planes.  A launch with HUNDREDS of workgroups per plane walks the planes one after another anyway — the workgroups
// resident at any time belong to a few planes, whose rows every L2 can hold — and then the plain linear order is better:
// all eight XCDs share every plane's work, so a head whose rows gather slower (HISTORY.md 4 item 5) slows everybody a little
// instead of one XCD a lot.  c5 (3 125 workgroups per plane): forward 2.92 -> 2.45 ms, sample gradients 3.44 -> 2.89 ms; its
// shards of 12 500 / 25 000 / 50 000 queries per plane (391 ... 1 563 workgroups): step -8 % each.  The threshold (option
// "linear_slots", default 320) is empirical: c3's sample-gradient kernel (279 workgroups per plane) loses 2 % in linear order.
inline bool plane_grid(Params &p, int npairs, int64_t slots, dim3 &grid)
{
    if (slots < 1) slots = 1;
    p.xcd_map = option_xcd_map();
    // (... where there is an imbalance for it to level: 128-byte rows 1 KB apart — H * D * sizeof = 1024 —, the layout whose
    // head 3 runs on half of the L1's tag RAMs.  Elsewhere the linear order only costs L2 locality: D = 128 / 256 in fp32 with
    // 625 / 500 workgroups per plane lost 10-19 % of their forward to it.)
    const bool skewed_layout = p.vrow_bytes == 128 && p.v_row == 1024;
    if (p.xcd_map == 1 && skewed_layout && slots >= option_linear_slots()) p.xcd_map = 0;
    // ... and so is a launch whose planes do not cover the eight XCDs evenly (the XCD-aware grid gives plane-group x to XCD x
    // and pads the rest: 4 planes would use half the chip — step 0.312 -> 0.204 ms at B = 1, H = 4, Q = 40 000; 12 planes: -11 %)
    if (p.xcd_map == 1 && option_linear_slots() > 0 && (int64_t)npairs * 100 < ((int64_t)npairs + 7) / 8 * 8 * 85) p.xcd_map = 0;
    const int64_t groups = (npairs + 7) / 8;
    if (p.xcd_map && slots <= 65535 && groups <= 65535) {
        p.grid3d = 1;
        grid = dim3(8, (unsigned)slots, (unsigned)groups);
        note_grid(0);
        return true;
    }
    if (!p.xcd_map && npairs <= 65535 && slots < ((int64_t)1 << 31)) {
        p.grid3d = 1;
        grid = dim3((unsigned)slots, (unsigned)npairs);
        note_grid(1);
        return true;
    }
    p.grid3d = 0;
    const int64_t blocks = (p.xcd_map ? groups * 8 : (int64_t)npairs) * slots;
    if (blocks >= ((int64_t)1 << 31)) return false;
    grid = dim3((unsigned)blocks);
    note_grid(2);
    return true;
}

// Params::touch (msda_kernels.hpp, Touch; option "touch": 0 never, 2 always, 1 = this rule): calls whose samples will read
// most rows of the pyramid anyway (4 Q L P taps >= 2 I rows per plane) and that are small enough for a cold start to be what
// they cost.  In-process A/B, B = 4, H = 8, c2 pyramid, caches AND Infinity Cache flushed (tools/small_q_cold.py --flush 1024):
// Q = 500 19.9 -> 19.0 us, 900 26.2 -> 22.8, 1000 26.6 -> 23.2 (2000, two rounds of workgroups: 35.4 -> 32.9, given up for
// touch_settle's rule below).
// (The one-wave-per-unit kernel does not touch: its waves all start together, the touches only queue in front of the rows
// they want — Q = 100 10.7 -> 15.0 us, 300 15.7 -> 17.5.)
inline int touch_plan(const Dims &d)
{
    const int o = option_touch();
    if (o != 1) return o;  // (2: forced)
    return d.Q * samples(d) * 4 >= 2 * d.I && d.B * d.Q * d.H <= 65536;
}
// ... and, known once the grid is: only launches of ONE round of workgroups in which a workgroup touches at most 768 rows.
// The touches go through the texture path in front of the workgroup's first samples (one row per lane: 64 tag look-ups per
// wave instruction), which is free while everything waits for memory and is not when the rows are already in L2: c4 (64
// planes x 4 workgroups, 1 360 rows each) 23.7 -> 26.5 us warm with the touches; c2 @ 1k and c1 (680 rows each) unchanged
// within +-0.5 us (rocprofv3, options alternated on one box).
int device_cu_count();  // CUs of the current device (cached; msda_api.hip)
inline void touch_settle(Params &p, const dim3 &grid, long long slots)
{
    if (p.touch == 1 && ((long long)grid.x * grid.y * grid.z > device_cu_count() || (p.I + slots - 1) / slots > 768)) p.touch = 0;
    if (p.touch == 2) p.touch = 1;
}

inline FastDiv make_fast_div(uint32_t d)
{
    FastDiv fd{0, 0};
    if (d <= 1) return fd;
    uint32_t shift = 0;
    while ((1ull << shift) < d) ++shift;  // ceil(log2 d)
    const uint64_t m = ((1ull << (32 + shift)) / d) - (1ull << 32) + 1;  // fits 32 bits for d > 1
    fd.magic = (uint32_t)m;
    fd.shift = shift;
    return fd;
}

inline int pick_group(int lanes_needed)
{
    if (lanes_needed <= 4) return 4;
    if (lanes_needed <= 8) return 8;
    if (lanes_needed <= 16) return 16;
    if (lanes_needed <= 32) return 32;
    return 64;
}

// samples of a unit parked in LDS at a time (records) and the total dynamic LDS
inline void plan_gather(int NU, int LP, size_t acc_bytes, int &sc, size_t &lds, bool aux = false, size_t budget = kRecordLdsBudget)
{
    const size_t rec = 16 + (aux ? 7 : 4) * acc_bytes;  // aux: the fused backward's (a, ox, oy) per slot
    int cap = (int)(budget / (NU * rec)) - 1;
    if (cap < 1) cap = 1;
    sc = LP < cap ? LP : cap;
    lds = kGatherLdsFixed + (size_t)NU * (sc + 1) * rec;
}

// MODE 0: forward, 1: grad_loc/grad_attn, 2: fused forward, 3: fused backward (sample half)
// ---- the gather kernels with the coarsest levels in LDS (msda_kernels.hpp, LDSL): ONE 1024-thread workgroup per CU,
// every (b, h) plane cut into as many runs of query chunks as fill the chip once ----
// (b, q, h) units up to which the one-wave-per-unit forward is taken: cold-cache forward at B = 4, H = 8 (round 5, in-process
// A/B): Q = 10 10.3 -> 7.5 us, 100 12.8 -> 9.4, 300 ~15 -> 13.2; from Q ~ 500 the general kernel is faster (900: 18-23 against 23.7)
constexpr long long kUnitFwdMaxUnits = 12288;
constexpr size_t kRecordLdsBudgetLds = 72 * 1024;  // the records of 16 waves (the fused backward's larger records: 100 KB)

struct LdsLevelsPlan {
    bool use;
    int nqc, qw, slots, sc;
    size_t lds;
    int lev_bytes;
    int planes;  // 2: a workgroup serves the planes of two neighbouring heads and balances its waves between them
    bool rotate; // one plane per workgroup, but two workgroups per CU and the heads rotated over the XCDs (below)
};
// (G lanes per unit, accumulators of acc_size bytes, rows of D * row_elem_size bytes)
inline LdsLevelsPlan lds_levels_plan_rt(const Params &p, int G, size_t acc_size, size_t row_elem_size, bool aux, bool stage,
                                        bool two_ok = false)
{
    const int NU = kBlockLds / G;
    LdsLevelsPlan pl{};
    size_t rec_lds;
    plan_gather(NU, p.LP, acc_size, pl.sc, rec_lds, aux, aux ? (size_t)100 * 1024 : kRecordLdsBudgetLds);
    if (pl.sc < p.LP && pl.sc > G) {  // several trips: whole exchange batches of the sample-gradient kernel per trip
        pl.sc = pl.sc / G * G;
        rec_lds = kGatherLdsFixed + (size_t)NU * (pl.sc + 1) * (16 + (aux ? 7 : 4) * acc_size);
    }
    // the waves' next-slice staging areas (dma_dword) — not with two planes per workgroup: they do not fit next to two copies
    const size_t lev_base2 = (rec_lds + 127) / 128 * 128;
    if (stage) rec_lds += (size_t)(kBlockLds / kWave) * kStageWaveBytes;
    size_t lev_base = (rec_lds + 127) / 128 * 128;
    const size_t row = (size_t)p.D * row_elem_size;
    const int npairs_all = p.B * p.H, ncu = device_cu_count();
    // the whole plane at most; the kernel takes the longest suffix of the level list that fits
    const long long plane = (long long)p.I * (long long)row;
    auto levels_for = [&](int planes) {
        const long long room = ((long long)kMaxDynLds - (long long)(planes == 2 ? lev_base2 : lev_base)) / planes -
                               (long long)((row + 127) / 128 * 128) - 128;
        long long lb = room < plane ? (room < 0 ? 0 : room) : plane;
        if (option_lds_budget() >= 0 && option_lds_budget() < lb) lb = option_lds_budget();
        return (int)lb;
    };
    auto slots_for = [&](int npairs, int nqc) {
        int sl = npairs >= ncu ? 1 : (ncu + npairs / 2) / npairs;
        sl *= option_lds_over();
        if (sl > nqc) sl = nqc;
        return sl < 1 ? 1 : sl;
    };
    pl.nqc = (p.Q + NU - 1) / NU;
    pl.planes = 1;
    pl.lev_bytes = levels_for(1);
    // TWO planes per workgroup — the neighbouring heads (b, 2k), (b, 2k + 1) — whose waves take slices of whichever plane
    // has more left (next_slice2): the rows of one head can gather 20 % slower than its neighbour's (they use half of the
    // vector L1's tag RAMs, HISTORY.md 4 item 5), and a workgroup that owns one plane cannot give it more waves.  When both planes'
    // levels fit where one plane's did (c2 @ 10k forward 69.3 -> 65.4 us).
    // (... and the pairs still cover the eight XCDs evenly: the XCD-aware grid gives plane-group x to XCD x)
    // (both remedies below exist for layouts whose rows sit an EVEN number of 128-byte lines apart — every row of a head on
    //  the same tag RAMs; a caller that pads the pixels' rows, value_row_stride, has no slow head: one plane per workgroup
    //  and no rotation are then faster — c2 @ 10k with rows 1 152 B apart: forward 64.5 -> 62.8 us, sample gradients 83 -> 78)
    const bool skewed_rows = (p.v_row % 256) == 0;
    if (two_ok && option_lds_planes() != 1 && (p.H % 2) == 0 && npairs_all >= 2 &&
        (option_lds_planes() == 2 || (skewed_rows && (npairs_all / 2) % 8 == 0))) {
        // The level sizes live on the device; the host has I and L.  For a pyramid whose levels shrink four-fold count the
        // levels of the suffix that fits either budget: two planes when halving the budget loses none of them (a wrong guess
        // costs speed, never correctness — the kernel fits its suffix itself).
        const int lb2 = levels_for(2);
        auto fit = [&](long long budget) {
            double total = 0.0, w = 1.0;
            for (int l = 0; l < p.L; ++l, w *= 0.25) total += w;
            double px = (double)p.I / total;
            for (int l = 1; l < p.L; ++l) px *= 0.25;  // pixels of the coarsest level
            double sum = 0.0;
            int n = 0;
            for (int l = p.L - 1; l >= 0; --l, px *= 4.0) {
                if ((sum + px) * (double)row > (double)budget) break;
                sum += px;
                ++n;
            }
            return n;
        };
        // ... and the pairs' workgroups do not come out heavier than single planes' would (the query chunks are dealt out in
        // whole numbers: at c2 @ 5k a pair's workgroup would take 2 x 3 chunks where a plane's takes 5 — 43.5 against 39.2 us;
        // @ 6k / 7.5k / 10k / 20k the loads are equal and two planes win by 4-8 %)
        const int sl1 = slots_for(npairs_all, pl.nqc), sl2 = slots_for(npairs_all / 2, pl.nqc);
        const int qw1 = (pl.nqc + sl1 - 1) / sl1, qw2 = (pl.nqc + sl2 - 1) / sl2;
        if (option_lds_planes() == 2 || (fit(lb2) == fit(pl.lev_bytes) && fit(lb2) > 0 && 2 * qw2 <= qw1 + qw1 / 8 && qw2 >= 2)) {
            pl.planes = 2;
            pl.lev_bytes = lb2;
            lev_base = lev_base2;
        }
    }
    const int npairs = npairs_all / pl.planes;
    int slots = slots_for(npairs, pl.nqc);
    // One plane per workgroup (the plain sample-gradient kernel) and >= 1024 queries per workgroup: cut the launch into two
    // workgroups per CU and rotate the heads over the XCDs, so that the dispatcher hands an XCD's CUs their second workgroup
    // as they come free and a slow head (HISTORY.md 4 item 5) is shared by four XCDs: c2 @ 10k 91 -> 87.4 us; smaller problems pay
    // more for staging the levels twice than they get back (c2 @ 5k: 50.7 -> 55.2), so not there.
    pl.rotate = false;
    if (two_ok == false && pl.planes == 1 && option_lds_planes() != 1 && skewed_rows && option_lds_over() == 1 && npairs_all >= 16 &&
        (long long)((pl.nqc + slots - 1) / slots) * NU >= 1024 && slots * 2 <= pl.nqc) {
        slots *= 2;
        pl.rotate = true;
    }
    pl.qw = (pl.nqc + slots - 1) / slots;
    pl.slots = (pl.nqc + pl.qw - 1) / pl.qw;
    pl.lds = lev_base + (size_t)pl.planes * ((size_t)pl.lev_bytes + (row + 127) / 128 * 128 + 128);
    const long long wgs = (long long)npairs * pl.slots, rounds = (wgs + ncu - 1) / ncu;
    const int opt = option_lds_levels();
    // worth it when the workgroups fill the CUs (one 1024-thread workgroup each) evenly: c2 @ 10k 99 -> 75 us, @ 1k
    // (one chunk per workgroup) still 15.3 -> 14.4, c4 28.5 -> 26.9; the README shape (128 workgroups: half the chip) 10.7 -> 13
    const bool pays = wgs * 10 >= rounds * ncu * 8 && pl.lev_bytes >= (int)(64 * row);
    pl.use = opt == 2 ? pl.lev_bytes >= (int)row : opt == 1 && pays;
    return pl;
}
template <typename T, int G, typename TV> inline LdsLevelsPlan lds_levels_plan(const Params &p, bool aux, bool stage = false)
{
    return lds_levels_plan_rt(p, G, sizeof(typename Traits<T>::acc), sizeof(TV), aux, stage);
}

// what option "profile" calls a gather launch: the kernel's name — the split-projection pair reports its entry points' names
template <int MODE, typename PP> constexpr const char *gather_profile_name()
{
    if constexpr (kSplitProj<PP>) return MODE == 2 ? "msda_fwd_fused_levelref_split" : "msda_bwd_fused_levelref_split";
    else return MODE == 0 || MODE == 2 ? "msda_fwd_kernel" : "msda_bwd_sample_kernel";
}

template <typename T, int VEC, int G, int MODE, typename TV, typename TS = T, typename PP = Params> inline int launch_gather_lds(PP &p, const LdsLevelsPlan &pl, hipStream_t stream)
{
    // MODE as in launch_gather: the forward and sample-gradient kernels, plain (0, 1) and with the module prologue (2, 3)
    p.sc = pl.sc;
    p.nqc = pl.nqc;
    p.qw = pl.qw;
    p.lds_lev_bytes = pl.lev_bytes;
    p.lds_stagger = option_lds_stagger();
    p.lds_planes = pl.planes;
    dim3 grid;
    if (!plane_grid(p, p.B * p.H / pl.planes, pl.slots, grid)) {
        set_error("grid too large");
        return MSDA_ERR_TOO_LARGE;
    }
    if (pl.rotate && p.xcd_map == 1) p.xcd_map = 2;  // (this launch only: plane_grid sets it afresh for the next one)
    touch_settle(p, grid, pl.slots);
    static std::atomic<uint64_t> big_lds_done{0};
    if constexpr (MODE == 0 || MODE == 2) {
        note_launch(0, 1);
        note_launch(1, pl.lev_bytes);
        note_launch(2, pl.planes);
        note_launch(3, (int)(grid.x * grid.y * grid.z));
        note_instance(8, VEC, G, p.D);
        note_trips(23, p.LP, pl.sc);
    } else {
        note_launch(4, 1);
        note_launch(5, pl.lev_bytes);
        note_instance(11, VEC, G, p.D);
        note_trips(24, p.LP, pl.sc);
    }
    const ProfileScope prof(gather_profile_name<MODE, PP>(), stream);
    if constexpr (MODE == 0 || MODE == 2) {
        auto kernel = msda_fwd_kernel<T, VEC, G, MODE == 2, TV, kBlockLds, true, std::conditional_t<MODE == 2, TS, T>, PP>;
        allow_big_lds(kernel, big_lds_done);
        hipLaunchKernelGGL(kernel, grid, dim3(kBlockLds), pl.lds, stream, p);
    } else {
        auto kernel = msda_bwd_sample_kernel<T, VEC, G, MODE == 3, TV, kBlockLds, true, std::conditional_t<MODE == 3, TS, T>, PP>;
        allow_big_lds(kernel, big_lds_done);
        hipLaunchKernelGGL(kernel, grid, dim3(kBlockLds), pl.lds, stream, p);
    }
    return (int)hipGetLastError();
}

// does this call carry a query mask (MaskedParams::qmask)?
template <typename PP> inline bool has_query_mask(const PP &p)
{
    if constexpr (kValueMask<PP>) return p.qmask != nullptr;
    else return false;
}

template <typename T, int VEC, int G, int MODE, typename TV = T, typename TS = T, typename PP = Params> inline int launch_gather(PP &p, hipStream_t stream)
{
    using A = typename Traits<T>::acc;
    constexpr int NU = kBlock / G;
    // (the sample-gradient kernel has the variant for its reduce-scatter units: float accumulation, 4 or 8 lanes)
    // fp32 operators only: measured at c3 (bf16, 64-byte rows: forward 88 against 86 us) and c5 (fp16, D = 64, L * P = 40 in
    // three trips: 3.17 against 2.93 ms) the 16-bit operators do not gain
    if constexpr ((MODE == 2 || MODE == 3) && kRagged<PP>) {
        // (the fused kernels' level scan is bounded, msda_kernels.hpp; before anything is launched)
        if (p.L > kFusedRaggedMaxLevels) {
            set_error("the fused prologue with per-level point counts serves at most %d levels, got %d", kFusedRaggedMaxLevels, p.L);
            return MSDA_ERR_UNSUPPORTED;
        }
    }
    // small problems (decoder calls): the forward with one wave per unit (msda_fwd_unit_kernel)
    // (never for a value-mask call: the one-wave-per-unit kernel has no mask hook — fwd_variant says 0 or 1 there)
    if constexpr (MODE == 0 && VEC * sizeof(T) == 16 && sizeof(A) == 4 && !kValueMask<PP>) {
        const long long units = (long long)p.B * p.Q * p.H;
        const int gl = p.D / VEC;
        const int uopt = option_unit_fwd();
        if (uopt != 0 && (p.D % VEC) == 0 && gl >= 1 && gl <= kWave && (gl & (gl - 1)) == 0 && p.LP <= 1024 &&
            units <= (uopt == 2 ? (1ll << 30) : kUnitFwdMaxUnits) && units < (1ll << 31)) {
            const ProfileScope prof("msda_fwd_unit_kernel", stream);
            note_launch(0, 2);
            note_launch(1, 0);
            note_launch(2, 1);
            note_launch(3, (int)units);
            note_instance(8, VEC, gl, p.D);  // (D / VEC lanes hold the row: one chunk)
            static std::atomic<uint64_t> big_lds_unit{0}, big_lds_unit2{0};
            // two units per wave (option "unit_waves" 2; msda_kernels.hpp): faster with the rows in HBM, slower with them
            // cached — which is the usual case, so one unit per wave is the default.  In-process A/B at B = 4, H = 8, one / two
            // units per wave: rows in the Infinity Cache Q = 100 7.96 / 8.32 us, 200 9.60 / 9.68, 300 11.28 / 11.92; rows in
            // HBM 100 10.4 / 10.4, 200 13.5 / 12.6, 300 16.7 / 15.4 (tools/small_q_cold.py --flush 256 / 1024).
            const bool pairs_ok = gl <= kWave / 2 && (size_t)p.B * p.I * (size_t)p.v_row < ((size_t)1 << 31);
            const bool pairs = pairs_ok && option_unit_waves() == 2;
            note_trips(23, p.LP, kWave / (pairs ? 2 : 1));  // (a unit's 64 / U lanes take one sample each per trip)
            if (pairs) {
                p.div_win = make_fast_div((uint32_t)p.Q);  // (the forward has no other use for this field)
                auto kernel = msda_fwd_unit_kernel<T, VEC, TV, 2, PP>;
                allow_big_lds(kernel, big_lds_unit2);
                const size_t ulds = kGatherLdsFixed + (size_t)2 * 8 * p.LP * 4;
                hipLaunchKernelGGL(kernel, dim3((unsigned)((units + 1) / 2)), dim3(kWave), ulds, stream, p.loc, p.attn, p.shapes, p.LP, p.L,
                                   (int)units, p);
            } else {
                auto kernel = msda_fwd_unit_kernel<T, VEC, TV, 1, PP>;
                allow_big_lds(kernel, big_lds_unit);
                const size_t ulds = kGatherLdsFixed + (size_t)8 * p.LP * 4;
                hipLaunchKernelGGL(kernel, dim3((unsigned)units), dim3(kWave), ulds, stream, p.loc, p.attn, p.shapes, p.LP, p.L, (int)units, p);
            }
            return (int)hipGetLastError();
        }
    }
    // ... and the module's kernels (fused prologue).  (An early version of the variant had lost over a bf16 pyramid — the
    // module's step 1.09 -> 1.31 ms; with the waves' dynamic slices it wins there as well: fused forward 116-126 -> 75-79 us,
    // fused sample gradients 124-135 -> 115-123 at the c2 shape.)
    // (the module's uniform masked pair, msda_bwd_fused_masked_<suffix>, with fp32 rows and 8-lane units: the fused
    // sample-gradient kernel with LDS-served levels sits at the 128-VGPR cap of its 1024-thread workgroup, and mask_taps'
    // four pixel indices and mask bytes cost that one instantiation 2 vector registers of scratch — it is not instantiated,
    // and such a call takes the 256-thread kernel below, which has the hook; "sample_variant" says 0.  The 4-lane units, the
    // 16-bit rows and the per-level-count / per-level-reference kernargs fit.)
    constexpr bool kNoLdsMaskHook = MODE == 3 && G == 8 && sizeof(TV) == 4 && std::is_same<PP, MaskedParams>::value;
    if constexpr (VEC == 4 && sizeof(A) == 4 && (sizeof(T) == 4 || MODE == 0) && !kNoLdsMaskHook &&
                  (((MODE == 0 || MODE == 2) && G <= 16) || ((MODE == 1 || MODE == 3) && (G == 4 || G == 8)))) {
        // (fp32 arithmetic; the rows may be 16-bit — the mixed-storage and module-storage kernels: 8-byte pieces, half the LDS)
        const LdsLevelsPlan pl = lds_levels_plan_rt(p, G, sizeof(A), sizeof(TV), MODE == 3, MODE == 1, /*two planes*/ MODE != 1);
        // (not the plain sample-gradient kernel: it would give up its LDS-DMA prefetch for them — 92.9 against 92.7 us, a draw)
        // (a query mask: the fused sample-gradient kernel with LDS-served levels has no hook for it — at its register cap,
        // msda_kernels.hpp — so such a call takes the 256-thread kernel below)
        if (pl.use && (MODE < 2 || pl.sc == p.LP) && !(MODE == 3 && has_query_mask(p)))
            return launch_gather_lds<T, VEC, G, MODE, TV, TS, PP>(p, pl, stream);
    }
    size_t lds;
    plan_gather(NU, p.LP, sizeof(A), p.sc, lds, MODE == 3);
    p.nqc = (p.Q + NU - 1) / NU;
    const int npairs = p.B * p.H;
    // query chunks per workgroup (1 unless the wg_target experiment knob says otherwise)
    long long qw = ((long long)p.nqc * npairs) / option_wg_target();
    p.qw = (int)(qw < 1 ? 1 : qw > 64 ? 64 : qw);
    const int slots = (p.nqc + p.qw - 1) / p.qw;
    dim3 grid;
    if (!plane_grid(p, npairs, slots, grid)) {
        set_error("grid too large");
        return MSDA_ERR_TOO_LARGE;
    }
    if ((MODE == 2 || MODE == 3) && p.sc != p.LP) {
        set_error("fused prologue needs all L*P=%d samples of a unit in LDS at once (limit %d)", p.LP, p.sc);
        return MSDA_ERR_UNSUPPORTED;
    }
    // Many workgroups per plane and at least two planes per XCD: rotate the heads over the XCDs (decode_block, xcd_map 2), so
    // that an XCD's planes belong to different heads and the dispatcher, which hands its CUs the next workgroup as they come
    // free, levels a head whose rows gather slower (HISTORY.md 4 item 5).  c3: sample gradients 84.7 -> 81.0 us, forward 76.2 -> 75.1.
    if (p.xcd_map == 1 && npairs >= 16 && slots >= 32) p.xcd_map = 2;
    touch_settle(p, grid, slots);
    if constexpr (MODE == 0 || MODE == 2) {
        note_launch(0, 0);
        note_launch(1, 0);
        note_launch(2, 1);
        note_launch(3, (int)(grid.x * grid.y * grid.z));
        note_instance(8, VEC, G, p.D);
        note_trips(23, p.LP, p.sc);
    } else {
        note_launch(4, 0);
        note_launch(5, 0);
        note_instance(11, VEC, G, p.D);
        note_trips(24, p.LP, p.sc);
    }
    static std::atomic<uint64_t> big_lds_done{0};  // one per template instantiation
    const ProfileScope prof(gather_profile_name<MODE, PP>(), stream);
    if constexpr (MODE == 3) {
        auto kernel = msda_bwd_sample_kernel<T, VEC, G, true, TV, kBlock, false, TS, PP>;
        allow_big_lds(kernel, big_lds_done);
        hipLaunchKernelGGL(kernel, grid, dim3(kBlock), lds, stream, p);
    } else if constexpr (MODE == 1) {
        auto kernel = msda_bwd_sample_kernel<T, VEC, G, false, TV, kBlock, false, T, PP>;
        allow_big_lds(kernel, big_lds_done);
        hipLaunchKernelGGL(kernel, grid, dim3(kBlock), lds, stream, p);
    } else if constexpr (MODE == 2) {
        auto kernel = msda_fwd_kernel<T, VEC, G, true, TV, kBlock, false, TS, PP>;
        allow_big_lds(kernel, big_lds_done);
        hipLaunchKernelGGL(kernel, grid, dim3(kBlock), lds, stream, p);
    } else {
        auto kernel = msda_fwd_kernel<T, VEC, G, false, TV, kBlock, false, T, PP>;
        allow_big_lds(kernel, big_lds_done);
        hipLaunchKernelGGL(kernel, grid, dim3(kBlock), lds, stream, p);
    }
    return (int)hipGetLastError();
}

template <typename T, int VEC, int MODE, typename TV = T, typename TS = T, typename PP = Params> inline int dispatch_group(PP &p, hipStream_t stream)
{
    const int lanes = (p.D + VEC - 1) / VEC;
    switch (pick_group(lanes)) {
    case 4: return launch_gather<T, VEC, 4, MODE, TV, TS>(p, stream);
    case 8: return launch_gather<T, VEC, 8, MODE, TV, TS>(p, stream);
    case 16: return launch_gather<T, VEC, 16, MODE, TV, TS>(p, stream);
    case 32: return launch_gather<T, VEC, 32, MODE, TV, TS>(p, stream);
    default: return launch_gather<T, VEC, 64, MODE, TV, TS>(p, stream);
    }
}

template <typename T, int MODE, typename TV = T, typename TS = T, typename PP = Params> inline int dispatch_gather(PP &p, bool vec_ok, hipStream_t stream)
{
    constexpr int VECF = 16 / sizeof(T);  // channels per lane (mixed storage: the 16-bit value rows load as 8-byte pieces)
    // the 16-bit operators' forward: when the LDS-served-level variant would be taken, as units of 8-byte pieces (twice the
    // lanes per row — 128 units per 1024-thread workgroup, whose records leave room for the levels; bit-identical results:
    // a channel's sum does not depend on the lane that holds it): c3 forward 81 -> 75.5 us, encoder-local points 72 -> 66
    if constexpr (MODE == 0 && sizeof(T) == 2 && sizeof(TV) == 2 && sizeof(typename Traits<T>::acc) == 4) {
        // (64-byte rows, all samples of a unit in one trip: at c5 — 128-byte rows, L * P = 40 — the variant loses, 2.92 -> 3.21 ms)
        if (vec_ok && (p.D % 4) == 0 && p.D <= 32) {
            const int g = pick_group((p.D + 3) / 4);
            const long long units = (long long)p.B * p.Q * p.H;
            if (units > kUnitFwdMaxUnits) {
                const LdsLevelsPlan pl = lds_levels_plan_rt(p, g, 4, sizeof(TV), false, false);
                if (pl.use && pl.sc == p.LP) return dispatch_group<T, 4, MODE, TV, TS>(p, stream);
            }
        }
    }
    if (vec_ok && (p.D % VECF) == 0) return dispatch_group<T, VECF, MODE, TV, TS>(p, stream);
    return dispatch_group<T, 1, MODE, TV, TS>(p, stream);
}

// ---- sorted (gather-formulated) grad_value: K1..K5 of msda_value_sorted.hpp ----
// PP = MaskedParams: the finish pass is the value-mask twin (the gather itself knows no mask)
// PP = RaggedMaskedParams: the same twin — the finish pass works per pixel and reads no level start, so it takes the call's
// Params part and its two mask pointers as a MaskedParams (no finish kernels of its own for per-level counts)
inline const MaskedParams &finish_kernarg(const MaskedParams &p) { return p; }
inline MaskedParams finish_kernarg(const RaggedMaskedParams &p)
{
    MaskedParams m{};
    static_cast<Params &>(m) = p;
    m.vmask = p.vmask;
    m.qmask = p.qmask;
    return m;
}
template <typename T, int VEC, int G, int GB, typename TV = T, typename TS = T, typename PP = Params> inline int launch_value_gather_block(PP &p, hipStream_t stream)
{
    constexpr int NUG = GB / G;
    const int npairs = p.B * p.H;
    dim3 g4, g5;
    if (!plane_grid(p, npairs, (p.win_cap + NUG - 1) / NUG, g4)) {
        set_error("grid too large");
        return MSDA_ERR_TOO_LARGE;
    }
    note_instance(14, VEC, G, p.D);
    {
        const ProfileScope prof("msda_value_gather_kernel", stream);
        // The gather's many small workgroups are handed to an XCD's CUs as they come free, so the planes of an XCD balance
        // each other out — if they are planes of DIFFERENT heads: the grad_out rows of one head can gather 20 % slower than the
        // others' (they use half of the vector L1's tag RAMs, HISTORY.md 4 item 5), and with every plane of an XCD belonging to that
        // head nothing balances.  The rotated mapping mixes the heads (c2 @ 10k: 60.7 -> 56.7 us).
        const int keep = p.xcd_map;
        if (p.xcd_map == 1) p.xcd_map = 2;
        hipLaunchKernelGGL((msda_value_gather_kernel<T, VEC, G, GB, TS>), g4, dim3(GB), 0, stream, static_cast<const Params &>(p));
        p.xcd_map = keep;
    }
    // (4-lane groups: 64 of them per workgroup, so 64 pixels keep them all busy)
    const int fp = kBlock / G > 32 ? 64 : finish_pixels(npairs, p.I);
    if (!plane_grid(p, npairs, (p.I + fp - 1) / fp, g5)) {
        set_error("grid too large");
        return MSDA_ERR_TOO_LARGE;
    }
    const ProfileScope prof("msda_value_finish_kernel", stream);
    if constexpr (kValueMask<PP>) {
        if (fp == 64)
            hipLaunchKernelGGL((msda_value_finish_masked_kernel<T, VEC, G, GB, TV, 64>), g5, dim3(kBlock), 0, stream, finish_kernarg(p));
        else
            hipLaunchKernelGGL((msda_value_finish_masked_kernel<T, VEC, G, GB, TV, 32>), g5, dim3(kBlock), 0, stream, finish_kernarg(p));
    } else {
        if (fp == 64)
            hipLaunchKernelGGL((msda_value_finish_kernel<T, VEC, G, GB, TV, 64>), g5, dim3(kBlock), 0, stream, static_cast<const Params &>(p));
        else
            hipLaunchKernelGGL((msda_value_finish_kernel<T, VEC, G, GB, TV, 32>), g5, dim3(kBlock), 0, stream, static_cast<const Params &>(p));
    }
    return (int)hipGetLastError();
}

template <typename T, int VEC, int G, typename TV = T, typename TS = T, typename PP = Params> inline int launch_value_gather(PP &p, hipStream_t stream)
{
    // (64- and 128-thread gather workgroups were measured too: 71-74 us against 73.6 at c2-10k — no effect, removed)
    return launch_value_gather_block<T, VEC, G, 256, TV, TS>(p, stream);
}

template <typename T, int VEC, typename TV = T, typename TS = T, typename PP = Params> inline int dispatch_value_gather_group(PP &p, hipStream_t stream)
{
    const int lanes = (p.D + VEC - 1) / VEC;
    switch (pick_group(lanes)) {
    case 4: return launch_value_gather<T, VEC, 4, TV, TS>(p, stream);
    case 8: return launch_value_gather<T, VEC, 8, TV, TS>(p, stream);
    case 16: return launch_value_gather<T, VEC, 16, TV, TS>(p, stream);
    case 32: return launch_value_gather<T, VEC, 32, TV, TS>(p, stream);
    default: return launch_value_gather<T, VEC, 64, TV, TS>(p, stream);
    }
}

// can the gather kernels use 16-byte row pieces for this call?
template <typename T> inline bool value_vec_ok(const Params &p)
{
    constexpr int VECF = 16 / sizeof(T);  // (mixed storage: grad_value rows are stored as 8-byte pieces, also fine at 16)
    return aligned_to(p.grad_out, 16) && aligned_to(p.grad_value, 16) && (p.D % VECF) == 0;
}

// KP: the kernarg type the count and place passes are instantiated on (run_value_sorted below picks it)
template <typename T, typename TV, typename TS, typename PP, typename KP> inline int run_value_sorted_on(PP &p, const Dims &d, void *workspace, hipStream_t stream)
{
    using A = typename Traits<T>::acc;
    const bool vec_ok = value_vec_ok<T>(p);
    const SortedWsLayout w = sorted_ws_layout(d.B, d.I, d.H, d.D, d.Q, d.L, samples(d), sizeof(A), sizeof(T), vec_ok, p.ent_alt0 != nullptr, sizeof(TV));
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    p.ws_part = reinterpret_cast<int *>(ws + w.off_part);
    p.ws_blocktot = reinterpret_cast<int *>(ws + w.off_blocktot);
    p.ws_off = reinterpret_cast<int *>(ws + w.off_off);
    p.ws_total = reinterpret_cast<int *>(ws + w.off_total);
    p.ws_meta = reinterpret_cast<int *>(ws + w.off_meta);
    p.ws_entries = ws + w.off_entries;
    p.ws_scratch = ws + w.off_scratch;
    p.ws_cont = ws + w.off_cont;
    p.ws_accum = w.rounds > 1 ? ws + w.off_accum : nullptr;
    p.nc_cap = w.nc_cap;
    p.nblk_cap = w.nblk_cap;
    p.win = w.win;
    p.div_win = make_fast_div((uint32_t)w.win);
    p.win_cap = w.win_cap;
    p.cont_cap = w.cont_cap;
    p.nsplit = w.nsplit;
    p.ent_cap = (int)((int64_t)w.q_round * samples(d));
    p.ent_n0 = w.ent_n0;  // (0 / 0 / 0 unless run_bwd offered the caller's gradient buffers: p.ent_alt0 / ent_alt1 / ent_alt2)
    p.ent_n1 = w.ent_n1;
    p.ent_n2 = w.ent_n2;
    // cells a count / place workgroup keeps in LDS at a time: what the LDS holds next to the level table and the
    // per-block totals
    {
        const long long room = ((long long)kMaxDynLds - (long long)sizeof(LevelTab)) / 4 - w.nblk_cap;
        long long cap = room < kCellLdsInts ? room : kCellLdsInts;
        cap = cap / kScanCells * kScanCells;
        if (cap < kScanCells) {
            set_error("plane too large for the sorted grad_value pipeline");
            return MSDA_ERR_TOO_LARGE;
        }
        p.cell_cap = w.nc_cap < cap ? w.nc_cap : (int)cap;
    }
    const int npairs = p.B * p.H;
    dim3 gcell;
    if (!plane_grid(p, npairs, p.nsplit, gcell)) {
        set_error("grid too large");
        return MSDA_ERR_TOO_LARGE;
    }
    // (the count pass keeps its per-block totals behind the cell table)
    const size_t cell_lds = sizeof(LevelTab) + ((size_t)p.cell_cap + (size_t)p.nblk_cap) * sizeof(int);
    static std::atomic<uint64_t> big_lds_count{0}, big_lds_place{0};
    allow_big_lds(msda_cell_pass_kernel<T, false, KP>, big_lds_count);  // (the instantiation that is launched)
    allow_big_lds(msda_cell_pass_kernel<T, true, KP>, big_lds_place);
    const int64_t scan_blocks = (int64_t)p.nblk_cap * npairs;
    if (scan_blocks >= ((int64_t)1 << 31)) {
        set_error("grid too large");
        return MSDA_ERR_TOO_LARGE;
    }
    constexpr int VECF = 16 / sizeof(T);
    // (a grid and the block -> plane mapping it was built for — plane_grid picks it per launch — travel together)
    const int g3_cell = p.grid3d, map_cell = p.xcd_map, cell_cap_pm = p.cell_cap;
    // The level-major place pass (msda_value_place.hpp; reproducible record order) serves every shape it can (P <= its
    // workgroup).  On pyramids much larger than the sample count (a decoder over a real image without the level-size
    // bound: 14 k samples against 36 k cells per plane) every workgroup loads its level's whole table and the
    // plane-major pass would be faster (14 us against 21 of a 147 us group) — but its record order follows LDS atomics,
    // and one rule — grad_value is bitwise reproducible — is worth more than 3 % on that shape.  place_path = 1 keeps
    // the plane-major pass reachable for measurements.
    const bool place_lm = d.P >= 1 && d.P <= kPlaceBlock && option_place_path() != 1;
    if (!place_lm && option_strict() != 0) {  // (no silent fall-back to an order that follows free-running atomics)
        set_error("strict: grad_value would take the plane-major place pass (P = %lld > %d points per level, or place_path = 1), "
                  "whose record order — and so grad_value's last bit — is not reproducible", (long long)d.P, kPlaceBlock);
        return MSDA_ERR_UNSUPPORTED;
    }
    // ... with 256-thread workgroups when one round of them covers a slice's queries (decoder-sized calls: few samples
    // per (level, slice)): the waves' turns are a chain of 4 hand-overs instead of 16, and more workgroups are in flight
    const int64_t q_slice = (w.q_round + p.nsplit - 1) / p.nsplit;
    const bool place_small = place_lm && d.P <= kPlaceBlockSmall &&
                             (option_place_path() == 3 || (option_place_path() == 0 && q_slice <= 6 * (kPlaceBlockSmall / d.P)));
    // Cells of its LDS table: the host knows only the plane's bound (2 I + 2 L) or the caller's promise about the largest
    // level; a table for that can fill the CU's LDS (c3: 142 KB, one workgroup per CU) although the largest level needs
    // 40 % of it.  The kernel walks a level larger than its table in several trips, so the table is capped at what lets
    // TWO workgroups share a CU: c3 66.3 -> 48.6 us, the 800 x 1066 decoder pyramid 29.0 -> 20.7, c5 unchanged (same-box
    // A/B, tools/ab_dbg.sh).
    int place_cells;
    {
        int64_t bound = w.nc_cap;
        const int64_t hint = level_cells_bound(d);
        if (hint > 0 && hint < bound) bound = hint;
        place_cells = place_cell_cap(bound, (size_t)kMaxDynLds);
        if (place_cells > kPlaceCellsTwoPerCu) place_cells = kPlaceCellsTwoPerCu;
    }
    dim3 gplace;
    int g3_place = 0, map_place = p.xcd_map;
    if (place_lm) {
        if (!plane_grid(p, npairs, (int64_t)d.L * p.nsplit, gplace)) {
            set_error("grid too large");
            return MSDA_ERR_TOO_LARGE;
        }
        g3_place = p.grid3d;
        map_place = p.xcd_map;
        static std::atomic<uint64_t> big_lds_lm{0}, big_lds_lm_small{0};
        allow_big_lds(msda_cell_place_lm_kernel<T, kPlaceBlock, KP>, big_lds_lm);
        allow_big_lds(msda_cell_place_lm_kernel<T, kPlaceBlockSmall, KP>, big_lds_lm_small);
    }
    // measurement only: the table sizes, slices, rounds, window and place-pass variant of this launch
    note_launch(17, cell_cap_pm);
    note_launch(18, place_lm ? place_cells : 0);
    note_launch(19, !place_lm ? 0 : place_small ? 2 : 1);
    note_launch(20, p.nsplit);
    note_launch(21, w.rounds);
    note_launch(22, p.win);
    for (int r = 0; r < w.rounds; ++r) {  // one round unless Q is so large that a plane's grad_out rows leave L2
        p.q_begin = r * w.q_round;
        p.q_end = p.q_begin + w.q_round < p.Q ? p.q_begin + w.q_round : p.Q;
        p.finish_mode = w.rounds == 1 ? 0 : r == 0 ? 1 : r == w.rounds - 1 ? 3 : 2;
        p.grid3d = g3_cell;
        p.xcd_map = map_cell;
        p.cell_cap = cell_cap_pm;
        {
            const ProfileScope prof("msda_cell_pass_kernel<count>", stream);
            hipLaunchKernelGGL((msda_cell_pass_kernel<T, false, KP>), gcell, dim3(kCellBlock), cell_lds, stream, static_cast<const KP &>(p));
        }
        {
            const ProfileScope prof("msda_cell_scan_kernel", stream);
            hipLaunchKernelGGL((msda_cell_scan_kernel<T>), dim3((unsigned)scan_blocks), dim3(kScanCells), 0, stream, static_cast<const Params &>(p));
        }
        {
        const ProfileScope prof_place(place_lm ? "msda_cell_place_lm_kernel" : "msda_cell_pass_kernel<place>", stream);
        if (place_lm) {
            p.grid3d = g3_place;
            p.xcd_map = map_place;
            p.cell_cap = place_cells;
            if (place_small)
                hipLaunchKernelGGL((msda_cell_place_lm_kernel<T, kPlaceBlockSmall, KP>), gplace, dim3(kPlaceBlockSmall), (size_t)place_cells * 4, stream, static_cast<const KP &>(p));
            else
                hipLaunchKernelGGL((msda_cell_place_lm_kernel<T, kPlaceBlock, KP>), gplace, dim3(kPlaceBlock), (size_t)place_cells * 4, stream, static_cast<const KP &>(p));
        } else {
            hipLaunchKernelGGL((msda_cell_pass_kernel<T, true, KP>), gcell, dim3(kCellBlock), cell_lds, stream, static_cast<const KP &>(p));
        }
        }
        int rc = (int)hipGetLastError();
        if (rc) return rc;
        rc = vec_ok ? dispatch_value_gather_group<T, VECF, TV, TS>(p, stream) : dispatch_value_gather_group<T, 1, TV, TS>(p, stream);
        if (rc) return rc;
    }
    return 0;
}

// The scan / gather passes know no mask, and neither do the count / place passes of a value-mask call: it runs the unmasked
// kernels on its Params part.  A QUERY mask (MaskedParams::qmask, msda_*_qmasked_*) is the count and place passes' business —
// they drop the masked queries' samples — so such a call, and only such a call, launches their MaskedParams instantiations.
template <typename T, typename TV = T, typename TS = T, typename PP = Params> inline int run_value_sorted(PP &p, const Dims &d, void *workspace, hipStream_t stream)
{
    if constexpr (kValueMask<PP>) {
        // (per-level counts: the ragged masked kernarg, else the ragged passes on its RaggedParams part)
        using Plain = std::conditional_t<kRagged<PP>, RaggedParams, Params>;
        using Masked = std::conditional_t<kRagged<PP>, RaggedMaskedParams, MaskedParams>;
        if (p.qmask != nullptr) return run_value_sorted_on<T, TV, TS, PP, Masked>(p, d, workspace, stream);
        return run_value_sorted_on<T, TV, TS, PP, Plain>(p, d, workspace, stream);
    } else {
        return run_value_sorted_on<T, TV, TS, PP, PP>(p, d, workspace, stream);
    }
}

// Params::v_row: bytes between consecutive pixels' rows of `value` — the caller's `value_row_stride` argument, 0 = dense
// (H * D * sizeof).  A caller that owns the layout pads every pixel's rows by one 128-byte line (HISTORY.md 4 item 5: the vector
// L1 picks its tag RAM from the low bits of the line index; rows exactly 1 KB apart leave one head on half of them).
// Read-only kernels — forward, sample gradients — follow it; grad_value is always written dense.
template <typename TV> inline int set_value_rows(Params &p, const Dims &d, int64_t value_row_stride)
{
    const int64_t dense = d.H * d.D * (int64_t)sizeof(TV);
    const int64_t row = value_row_stride > 0 ? value_row_stride : dense;
    if (value_row_stride < 0 || row < dense || row % (int64_t)sizeof(TV) != 0 || d.I * row >= ((int64_t)1 << 31) ||
        row >= (1 << 24)) {
        set_error("value_row_stride %lld: must be 0 (dense) or a multiple of the element size >= H*D*sizeof = %lld with "
                  "I * stride < 2^31", (long long)value_row_stride, (long long)dense);
        return row < dense || value_row_stride < 0 || row % (int64_t)sizeof(TV) != 0 ? MSDA_ERR_BAD_ARG : MSDA_ERR_TOO_LARGE;
    }
    p.v_row = (int)row;
    return 0;
}

inline void fill_params(Params &p, const Dims &d, int padding_mode, int align_corners)
{
    p.B = (int)d.B;
    p.I = (int)d.I;
    p.H = (int)d.H;
    p.D = (int)d.D;
    p.Q = (int)d.Q;
    p.L = (int)d.L;
    p.P = (int)d.P;
    p.LP = (int)samples(d);
    p.zeros = padding_mode == MSDA_PADDING_ZEROS;
    p.align = align_corners != 0;
    p.xcd_map = option_xcd_map();
    p.nqc = p.sc = 0;
    p.qw = 1;
    p.grid3d = 0;
    p.ref = nullptr;
    p.ref_dim = 0;
    p.debug = option_debug();
    p.div_h = make_fast_div((uint32_t)d.H);
}

// Per-level point counts (msda_*_ragged_<dtype>): the host array `ppl` of L counts, each >= 1.  Checks it and returns the
// largest count (the kernels' Params::P) and the sum S; a negative MSDA_ERR_* when it is unusable.
inline int ragged_counts(const int32_t *ppl, int64_t L, int64_t &pmax, int64_t &S)
{
    pmax = S = 0;
    if (L < 0 || (L > 0 && ppl == nullptr)) {
        set_error("points_per_level: null pointer or negative L");
        return MSDA_ERR_BAD_ARG;
    }
    if (L > MSDA_MAX_LEVELS) {
        set_error("L = %lld > %d levels", (long long)L, MSDA_MAX_LEVELS);
        return MSDA_ERR_TOO_MANY_LEVELS;
    }
    for (int64_t l = 0; l < L; ++l) {
        if (ppl[l] < 1) {
            set_error("points_per_level[%lld] = %d: every level needs at least one point", (long long)l, (int)ppl[l]);
            return MSDA_ERR_BAD_ARG;
        }
        pmax = ppl[l] > pmax ? ppl[l] : pmax;
        S += ppl[l];
    }
    return 0;
}
// the arguments msda_*_fused_hfbox_<dtype> have beyond the per-level-count pair's
inline int box_rule_args(const float *level_scale, int64_t L, int ref_dim)
{
    if (ref_dim != 4) {
        set_error("the Hugging Face box rule takes boxes: ref_dim must be 4, got %d", ref_dim);
        return MSDA_ERR_BAD_ARG;
    }
    if (level_scale == nullptr && L > 0) {
        set_error("level_scale: null pointer");
        return MSDA_ERR_BAD_ARG;
    }
    return 0;
}
inline void fill_level_starts(RaggedParams &p, const int32_t *ppl, int64_t L)
{
    p.pst[0] = 0;
    for (int64_t l = 0; l < L; ++l) p.pst[l + 1] = p.pst[l] + ppl[l];
    for (int64_t l = L + 1; l <= kMaxLevels; ++l) p.pst[l] = p.pst[L];
}
inline void fill_level_starts(Params &, const int32_t *, int64_t) {}
// Hugging Face's box rule (msda_*_fused_hfbox_<dtype>): the caller's fp32 scale per level and offset_scale, behind the
// level starts.  (L beyond the fused kernels' bound is refused before anything is launched; only the table is filled here.)
inline void fill_box_scales(HfBoxParams &p, const float *lscale, double off_scale, int64_t L)
{
    for (int64_t l = 0; l < kFusedRaggedMaxLevels; ++l) p.lscale[l] = l < L ? lscale[l] : 0.0f;
    p.off_scale = off_scale;
}
inline void fill_box_scales(HfBoxDiscreteParams &p, const float *lscale, double off_scale, int64_t L)
{
    for (int64_t l = 0; l < kFusedRaggedMaxLevels; ++l) p.lscale[l] = l < L ? lscale[l] : 0.0f;
    p.off_scale = off_scale;
}
inline void fill_box_scales(Params &, const float *, double, int64_t) {}
// the value padding mask (msda_*_masked_<dtype>): [B, I] bytes behind the kernarg; advanced with every other batch-indexed
// pointer when the grad_value pipeline runs once per group of batch elements
// ... and the query padding mask behind it (msda_*_qmasked_<dtype>): [B, Q] bytes, NULL from the _masked_ entry points
// (one definition for every kernarg that carries the pair — kValueMask — and a no-op for the others)
// the logits of a split projection and their gradient, behind the kernarg (a no-op for every other kernarg)
template <typename PP> inline void set_split_logits(PP &p, const void *logits, void *grad_logits)
{
    if constexpr (kSplitProj<PP>) {
        p.logits = logits;
        p.grad_logits = grad_logits;
    }
}
template <typename PP> inline void set_value_mask(PP &p, const uint8_t *vmask, const uint8_t *qmask)
{
    if constexpr (kValueMask<PP>) {
        p.vmask = vmask;
        p.qmask = qmask;
    }
}
template <typename PP> inline void advance_value_mask(PP &pg, const PP &p, size_t pixels, size_t queries)
{
    if constexpr (kValueMask<PP>) {
        pg.vmask = p.vmask + pixels;
        pg.qmask = p.qmask != nullptr ? p.qmask + queries : nullptr;
    }
}

// ---- discrete (nearest-pixel) sampling: msda_{fwd,bwd}_discrete_<dtype>, kernels in msda_discrete.hpp ----
// MODE 0: the forward, 1: the attention-weight gradient.  G lanes per unit from D as everywhere (pick_group); the
// workgroups are cut per (b, head) plane, kBlock / G units each.
template <typename T, int VEC, int G, int MODE, typename TV> inline int launch_discrete(DiscreteParams &p, hipStream_t stream)
{
    constexpr int NU = kBlock / G;
    p.nqc = (p.Q + NU - 1) / NU;
    dim3 grid;
    if (!plane_grid(p, p.B * p.H, p.nqc, grid)) {
        set_error("grid too large");
        return MSDA_ERR_TOO_LARGE;
    }
    if (MODE == 0) {
        note_launch(0, 3);
        note_launch(1, 0);
        note_launch(2, 1);
        note_launch(3, (int)(grid.x * grid.y * grid.z));
        note_instance(8, VEC, G, p.D);
        note_launch(23, 1);
        const ProfileScope prof("msda_fwd_discrete_kernel", stream);
        hipLaunchKernelGGL((msda_fwd_discrete_kernel<T, VEC, G, TV>), grid, dim3(kBlock), 0, stream, p);
    } else {
        note_launch(4, 2);
        note_launch(5, 0);
        note_instance(11, VEC, G, p.D);
        note_launch(24, 1);
        const ProfileScope prof("msda_bwd_discrete_attn_kernel", stream);
        hipLaunchKernelGGL((msda_bwd_discrete_attn_kernel<T, VEC, G, TV>), grid, dim3(kBlock), 0, stream, p);
    }
    return (int)hipGetLastError();
}
template <typename T, int VEC, int MODE, typename TV> inline int dispatch_discrete_group(DiscreteParams &p, hipStream_t stream)
{
    switch (pick_group((p.D + VEC - 1) / VEC)) {
    case 4: return launch_discrete<T, VEC, 4, MODE, TV>(p, stream);
    case 8: return launch_discrete<T, VEC, 8, MODE, TV>(p, stream);
    case 16: return launch_discrete<T, VEC, 16, MODE, TV>(p, stream);
    case 32: return launch_discrete<T, VEC, 32, MODE, TV>(p, stream);
    default: return launch_discrete<T, VEC, 64, MODE, TV>(p, stream);
    }
}
template <typename T, int MODE, typename TV> inline int dispatch_discrete(DiscreteParams &p, bool vec_ok, hipStream_t stream)
{
    constexpr int VECF = 16 / sizeof(T);
    if (vec_ok && (p.D % VECF) == 0) return dispatch_discrete_group<T, VECF, MODE, TV>(p, stream);
    return dispatch_discrete_group<T, 1, MODE, TV>(p, stream);
}

// ---- the box rule in front of discrete sampling: msda_{fwd,bwd}_fused_hfbox_discrete_<suffix>, kernels in
//      msda_hfbox_discrete.hpp ----
// MODE 0: the forward, 1: the backward (grad_proj; the points and weights for the grad_value passes).  The geometry is
// launch_discrete's; the kernels' level scan is the fused kernels' (at most kFusedRaggedMaxLevels scales in the kernarg),
// refused here, before anything is launched.
// PP = ModuleDiscreteParams (msda_{fwd,bwd}_fused_discrete_<suffix>): the same bodies behind the reference module's rule —
// the same variants, the same bound on L (lvl_of's count scan).
template <typename T, int VEC, int G, int MODE, typename TV, typename TS, typename PP>
inline int launch_hfbox_discrete(PP &p, hipStream_t stream)
{
    constexpr int NU = kBlock / G;
    p.nqc = (p.Q + NU - 1) / NU;
    dim3 grid;
    if (!plane_grid(p, p.B * p.H, p.nqc, grid)) {
        set_error("grid too large");
        return MSDA_ERR_TOO_LARGE;
    }
    if (MODE == 0) {
        note_launch(0, 4);
        note_launch(1, 0);
        note_launch(2, 1);
        note_launch(3, (int)(grid.x * grid.y * grid.z));
        note_instance(8, VEC, G, p.D);
        note_launch(23, 1);
        const ProfileScope prof(kModuleDiscrete<PP> ? "msda_fwd_module_discrete_kernel" : "msda_fwd_hfbox_discrete_kernel", stream);
        hipLaunchKernelGGL((msda_fwd_hfbox_discrete_kernel<T, VEC, G, TV, TS, PP>), grid, dim3(kBlock), 0, stream, p);
    } else {
        note_launch(4, 3);
        note_launch(5, 0);
        note_instance(11, VEC, G, p.D);
        note_launch(24, 1);
        const ProfileScope prof(kModuleDiscrete<PP> ? "msda_bwd_module_discrete_kernel" : "msda_bwd_hfbox_discrete_kernel", stream);
        hipLaunchKernelGGL((msda_bwd_hfbox_discrete_kernel<T, VEC, G, TV, TS, PP>), grid, dim3(kBlock), 0, stream, p);
    }
    return (int)hipGetLastError();
}
template <typename T, int VEC, int MODE, typename TV, typename TS, typename PP>
inline int dispatch_hfbox_discrete_group(PP &p, hipStream_t stream)
{
    switch (pick_group((p.D + VEC - 1) / VEC)) {
    case 4: return launch_hfbox_discrete<T, VEC, 4, MODE, TV, TS>(p, stream);
    case 8: return launch_hfbox_discrete<T, VEC, 8, MODE, TV, TS>(p, stream);
    case 16: return launch_hfbox_discrete<T, VEC, 16, MODE, TV, TS>(p, stream);
    case 32: return launch_hfbox_discrete<T, VEC, 32, MODE, TV, TS>(p, stream);
    default: return launch_hfbox_discrete<T, VEC, 64, MODE, TV, TS>(p, stream);
    }
}
template <typename T, int MODE, typename TV, typename TS, typename PP>
inline int dispatch_hfbox_discrete(PP &p, bool vec_ok, hipStream_t stream)
{
    constexpr int VECF = 16 / sizeof(T);
    if (p.L > kFusedRaggedMaxLevels) {
        set_error("the fused %s prologue serves at most %d levels, got %d", kModuleDiscrete<PP> ? "module" : "box", kFusedRaggedMaxLevels, p.L);
        return MSDA_ERR_UNSUPPORTED;
    }
    if (vec_ok && (p.D % VECF) == 0) return dispatch_hfbox_discrete_group<T, VECF, MODE, TV, TS>(p, stream);
    return dispatch_hfbox_discrete_group<T, 1, MODE, TV, TS>(p, stream);
}

// ---- one call of an entry point, by name.  The extern "C" functions (MSDA_DEFINE_* below) fill one and hand it to their
//      run_*; members a family does not have stay zero. ----
struct Call {
    // device buffers: the sampling operators' loc / attn and their gradients, the fused operators' proj / ref and theirs
    const void *grad_out = nullptr, *value = nullptr;
    const uint8_t *value_mask = nullptr;  // the masked twins: [B, I] bytes
    const uint8_t *query_mask = nullptr;  // ... and their query-mask entry points: [B, Q] bytes
    const int64_t *shapes = nullptr;
    const void *loc = nullptr, *attn = nullptr, *proj = nullptr, *ref = nullptr;
    void *out = nullptr, *grad_value = nullptr, *grad_loc = nullptr, *grad_attn = nullptr, *grad_proj = nullptr,
         *grad_ref_partial = nullptr;
    // split projections (msda_*_fused_levelref_split_<dtype>): `proj` / `grad_proj` then hold the offsets [.., 2] and their
    // gradient, and the logits [..] and theirs sit here
    const void *logits = nullptr;
    void *grad_logits = nullptr;
    int64_t B = 0, I = 0, H = 0, D = 0, Q = 0, L = 0;
    int64_t P = 0, S = 0;  // per-level counts: their maximum and sum (take_counts); else the uniform P and 0
    const int32_t *points_per_level = nullptr;  // host, L counts
    const float *level_scale = nullptr;         // host, L scales, and the config's offset_scale: Hugging Face's box rule
    double offset_scale = 0.0;
    int ref_dim = 0;
    int padding_mode = MSDA_PADDING_BORDER, align_corners = 0;  // (what discrete sampling, which has neither, runs with)
    int64_t max_level_cells = 0, value_row_stride = 0;
    void *workspace = nullptr;
    int64_t workspace_bytes = 0;
    void *stream = nullptr;
};
// checks points_per_level and notes its maximum and sum: once per call, in front of everything but the mask test
inline int take_counts(Call &c) { return ragged_counts(c.points_per_level, c.L, c.P, c.S); }
inline Dims make_dims(const Call &c)
{
    Dims d{c.B, c.I, c.H, c.D, c.Q, c.L, c.P, c.max_level_cells > 0 ? c.max_level_cells : 0};
    d.S = c.S;
    return d;
}
inline int check_ref_dim(int ref_dim)
{
    if (ref_dim == 2 || ref_dim == 4) return 0;
    set_error("ref_dim must be 2 or 4, got %d", ref_dim);
    return MSDA_ERR_BAD_ARG;
}
template <typename PP> constexpr bool kDiscrete = std::is_same<PP, DiscreteParams>::value;

// ---- the shared steps, part 2 ----
// The kernarg of a call whose buffers passed their checks: the sampling operators' pointers as they are (the fused run_*
// then put proj / grad_proj / the partials where their kernels read them), sizes and modes, the family's extras (level
// starts, box scales, mask: no-ops on a kernarg without them) and the row stride — the one argument checked this late.
template <typename TV, typename PP> inline int fill_kernarg(PP &p, const Call &c, const Dims &d)
{
    p.value = c.value;
    p.shapes = c.shapes;
    p.loc = c.loc;
    p.attn = c.attn;
    p.out = c.out;
    p.grad_out = c.grad_out;
    p.grad_value = c.grad_value;
    p.grad_loc = c.grad_loc;
    p.grad_attn = c.grad_attn;
    fill_params(p, d, c.padding_mode, c.align_corners);
    fill_level_starts(p, c.points_per_level, d.L);
    fill_box_scales(p, c.level_scale, c.offset_scale, d.L);
    set_value_mask(p, c.value_mask, c.query_mask);
    set_split_logits(p, c.logits, c.grad_logits);
    p.ref = c.ref;
    p.ref_dim = c.ref_dim;
    p.vrow_bytes = (int)(d.D * (int64_t)sizeof(TV));
    return set_value_rows<TV>(p, d, c.value_row_stride);
}
// can the gather kernels use 16-byte pieces of the value rows and of the rows they read or write next to them?
inline bool rows_vec_ok(const Params &p, const void *rows) { return aligned_to(p.value, 16) && aligned_to(rows, 16) && p.v_row % 16 == 0; }
// a launch's own failure (positive: a hipError_t; a negative status has its message already)
inline int launched(int rc, const char *what)
{
    if (rc > 0) set_error("%s launch failed: %s", what, hipGetErrorString((hipError_t)rc));
    return rc;
}

// PP = RaggedParams: per-level point counts; MaskedParams: the value-mask twin; DiscreteParams: nearest-pixel sampling
// (msda_fwd_discrete_<dtype>: per-level counts, no padding mode — border —, its own kernels)
template <typename T, typename TV = T, typename PP = Params> int run_fwd(const Call &c)
{
    const Dims d = make_dims(c);
    hipStream_t stream = static_cast<hipStream_t>(c.stream);
    const size_t out_bytes = (size_t)(d.B * d.Q * d.H * d.D) * sizeof(T);
    if (out_bytes == 0) return 0;  // nothing to produce
    int rc = check_common(d, sizeof(T), c.padding_mode);
    if (rc == 0) rc = require_buffers({c.out});
    if (rc) return rc;
    if (samples(d) == 0 || d.I == 0) return zero_outputs({{c.out, out_bytes}}, stream);  // empty sum
    if ((rc = require_buffers({c.value, c.shapes, c.loc, c.attn})) != 0) return rc;
    if ((rc = check_aligned({{c.value, sizeof(TV)}, {c.out, sizeof(T)}, {c.loc, 2 * sizeof(T)}, {c.attn, sizeof(T)}, {c.shapes, 8}})) != 0)
        return rc;
    PP p{};
    if ((rc = fill_kernarg<TV>(p, c, d)) != 0) return rc;
    if constexpr (kDiscrete<PP>) {
        return launched(dispatch_discrete<T, 0, TV>(p, rows_vec_ok(p, c.out), stream), "discrete forward");
    } else {
        p.touch = touch_plan(d);
        return launched(dispatch_gather<T, 0, TV>(p, rows_vec_ok(p, c.out), stream), "forward");
    }
}

// Module forward with the prologue fused in: `proj` is the raw query projection
// [B, Q, H, L, P, 3] = (x offset, y offset, attention logit), `ref` the reference points [B, Q, ref_dim].
// TS: storage type of `proj` and `out` (T unless the module keeps them in 16 bits next to fp32 reference points)
// PP = RaggedParams (msda_fwd_fused_ragged_<dtype>): per-level point counts, `proj` [B, Q, H, S, 3]
// PP = LevelRefParams (msda_fwd_fused_levelref_<dtype>): `ref` is [B, Q, L, ref_dim] and the points follow transformers'
// rule (msda_kernels.hpp)
// PP = HfBoxParams (msda_fwd_fused_hfbox_<dtype>): the per-level-count layout with transformers' box rule — `level_scale`
// holds L fp32 scales on the host, `offset_scale` the config's (the entry point checked ref_dim == 4)
// PP = HfBoxDiscreteParams (msda_fwd_fused_hfbox_discrete_<dtype>): the same rule in front of discrete sampling, on the
// kernels of msda_hfbox_discrete.hpp (no padding mode — border —, no 32-bit limit on the projection)
// PP = ModuleDiscreteParams (msda_fwd_fused_discrete_<dtype>): the module's own rule (ref_dim 2 or 4) on the same kernel bodies
// PP = MaskedParams (msda_fwd_fused_masked_<dtype>) / RaggedMaskedParams (msda_fwd_fused_ragged_masked_<dtype>): the module's
// own rule, uniform / per-level counts, with the value mask and (unless NULL) the query mask in the kernels
template <typename T, typename TV = T, typename TS = T, typename PP = Params> int run_fwd_fused(const Call &c)
{
    const Dims d = make_dims(c);
    hipStream_t stream = static_cast<hipStream_t>(c.stream);
    const size_t out_bytes = (size_t)(d.B * d.Q * d.H * d.D) * sizeof(TS);
    if (out_bytes == 0) return 0;
    int rc = check_ref_dim(c.ref_dim);
    if (rc == 0) rc = check_common(d, sizeof(T), c.padding_mode);
    if (rc == 0) rc = require_buffers({c.out});
    if (rc) return rc;
    if (samples(d) == 0 || d.I == 0) return zero_outputs({{c.out, out_bytes}}, stream);
    if ((rc = require_buffers({c.value, c.shapes, c.proj, c.ref})) != 0) return rc;
    if (kSplitProj<PP> && (rc = require_buffers({c.logits})) != 0) return rc;
    if (!kFusedDiscrete<PP> && fused_limit_exceeded(d)) {  // (the discrete kernels index the projection in 64 bits)
        set_error("projection too large for 32-bit sample offsets");
        return MSDA_ERR_TOO_LARGE;
    }
    if ((rc = check_aligned({{c.value, sizeof(TV)}, {c.out, sizeof(TS)}, {c.proj, sizeof(TS)}, {c.ref, sizeof(T)}, {c.shapes, 8}})) != 0)
        return rc;
    if (kSplitProj<PP> && (rc = check_aligned({{c.logits, sizeof(TS)}})) != 0) return rc;
    PP p{};
    if ((rc = fill_kernarg<TV>(p, c, d)) != 0) return rc;
    p.loc = c.proj;
    if constexpr (kFusedDiscrete<PP>)
        return launched(dispatch_hfbox_discrete<T, 0, TV, TS>(p, rows_vec_ok(p, c.out), stream), "fused discrete forward");
    else
        return launched(dispatch_gather<T, 2, TV, TS>(p, rows_vec_ok(p, c.out), stream), "fused forward");
}

// ---- single-launch grad_value for small problems (msda_value_small.hpp) ----
// Cells the kernel's LDS table must hold: the largest level's (h + 1)(w + 1).  The level sizes live on the device, so
// without a promise from the caller the bound is what I pixels can make of one level: 2 I + 2 L.
inline int64_t small_cell_cap(const Dims &d)
{
    const int64_t bound = 2 * d.I + 2 * d.L, hint = level_cells_bound(d);
    return hint > 0 && hint < bound ? hint : bound;
}
template <typename T> inline size_t small_need_bytes(const Dims &d, bool vec)
{
    using A = typename Traits<T>::acc;
    const size_t vecw = vec ? 16 / sizeof(T) : 1;
    return small_lds_bytes((size_t)small_cell_cap(d), (size_t)(d.Q * d.P), sizeof(A), vecw);
}

template <typename T, int VEC, int G, typename TV = T, typename TS = T, typename PP = Params> inline int launch_value_small(PP &p, size_t lds, hipStream_t stream)
{
    dim3 grid;
    if (!plane_grid(p, p.B * p.H, (int64_t)p.L * p.small_ns, grid)) {
        set_error("grid too large");
        return MSDA_ERR_TOO_LARGE;
    }
    note_instance(14, VEC, G, p.D);
    static std::atomic<uint64_t> big_lds_done{0};
    allow_big_lds(msda_value_small_kernel<T, VEC, G, TV, TS, PP>, big_lds_done);
    const ProfileScope prof("msda_value_small_kernel", stream);
    hipLaunchKernelGGL((msda_value_small_kernel<T, VEC, G, TV, TS, PP>), grid, dim3(kSmallBlock), lds, stream, p);
    return (int)hipGetLastError();
}

template <typename T, int VEC, typename TV = T, typename TS = T, typename PP = Params> inline int dispatch_value_small_group(PP &p, size_t lds, hipStream_t stream)
{
    const int lanes = (p.D + VEC - 1) / VEC;
    switch (pick_group(lanes)) {
    case 4: return launch_value_small<T, VEC, 4, TV, TS>(p, lds, stream);
    case 8: return launch_value_small<T, VEC, 8, TV, TS>(p, lds, stream);
    case 16: return launch_value_small<T, VEC, 16, TV, TS>(p, lds, stream);
    case 32: return launch_value_small<T, VEC, 32, TV, TS>(p, lds, stream);
    default: return launch_value_small<T, VEC, 64, TV, TS>(p, lds, stream);
    }
}

template <typename T, typename TV = T, typename TS = T, typename PP = Params> inline int run_value_small(PP &p, const Dims &d, hipStream_t stream)
{
    constexpr int VECF = 16 / sizeof(T);
    const bool vec_ok = value_vec_ok<T>(p);
    p.small_cells = (int)small_cell_cap(d);
    p.small_hinted = p.small_cells < 2 * d.I + 2 * d.L;
    // workgroups per (plane, level): fill the 256 CUs when there are few planes; two when the planes just fill them
    // (a level's workgroups then finish at different times and the busiest level no longer sets the pace)
    const int64_t wgs = d.B * d.H * d.L;
    // (also measured: one more workgroup for the level with the most pixels only — c4 55 -> 62 us, dropped)
    p.small_ns = option_small_ns() > 0 ? option_small_ns() : wgs <= 64 ? 4 : wgs <= 128 ? 2 : 1;
    const size_t lds = small_need_bytes<T>(d, vec_ok);
    return vec_ok ? dispatch_value_small_group<T, VECF, TV, TS>(p, lds, stream) : dispatch_value_small_group<T, 1, TV, TS>(p, lds, stream);
}

// the sorted pipeline's record format: 5 level bits, 23-bit biased pixel index, 32-bit slot offsets
template <typename T> inline bool sorted_fits(const Dims &d)
{
    using A = typename Traits<T>::acc;
    return d.L <= kSortedMaxLevels && d.I < (int64_t)kPixBias && 16 * d.D * (int64_t)sizeof(A) < ((int64_t)1 << 24) &&
           d.I * 4 * d.D * (int64_t)sizeof(A) < ((int64_t)1 << 31);
}

// Small problems: when all samples of a (plane, level) and the level's cell table fit one workgroup's LDS, the
// single-launch kernel does the whole job without workspace.  Measured on MI355X (grad_value alone): c4 (B=8, Q=900)
// 91 -> 55 us, c1 35 -> 26 us, c2 at Q=1000 66 -> 36 us.  It serves one (plane, level) per workgroup on one CU, so it is
// chosen only while a level holds at most 4096 samples.
template <typename T> inline bool small_fits(const Dims &d)
{
    return d.L >= 1 && 2 * d.I + 2 * d.L < ((int64_t)1 << 24) && d.Q < ((int64_t)1 << 24) &&
           small_need_bytes<T>(d, true) <= (size_t)kMaxDynLds;
}
template <typename T> inline bool small_path_chosen(const Dims &d)
{
    return small_fits<T>(d) && (option_value_path() == 3 || (option_value_path() == 0 && d.Q * d.P <= 4096));
}

// grad_value: the single-launch kernel for small problems (no workspace), else the sorted-gather pipeline in the
// caller's workspace.  There is no third path: a large problem without (enough) workspace is an argument error, and
// shapes beyond the sorted pipeline's record format (I >= 2^22 pixels per plane, D beyond 32-bit slot offsets) are
// unsupported for grad_value when they are also too large for the single-launch kernel.
// Passes over the batch (round 6): the workspace the CALLER gives decides.  The sorted pipeline's workspace is one set of
// tables and partial rows per (batch, head) plane of the call (c2 @ 10k: 107 MB); a workspace too small for the whole
// batch but large enough for half, a quarter ... of it makes the pipeline run once per group of batch elements —
// the same kernels on a sub-batch, every batch-indexed pointer advanced — in the same memory.  msda_bwd_workspace_bytes
// (..., flags | MSDA_WS_PASSES(n)) is the size for n passes.  Returns the batch elements per pass (0: nothing fits).
template <typename T, typename TV> inline int64_t value_batch_per_pass(const Params &p, const Dims &d, const void *workspace,
                                                                     int64_t workspace_bytes)
{
    using A = typename Traits<T>::acc;
    if (workspace == nullptr || !aligned_to(workspace, 256) || workspace_bytes < 0) return 0;
    for (int64_t passes = 1;; passes *= 2) {  // (until one batch element per pass)
        const int64_t per = (d.B + passes - 1) / passes;
        const bool rg = p.ent_alt0 != nullptr;
        size_t need = sorted_ws_layout(per, d.I, d.H, d.D, d.Q, d.L, samples(d), sizeof(A), sizeof(T), value_vec_ok<T>(p), rg, sizeof(TV)).total;
        if (passes > 1) {  // (a later group's pointers may be aligned differently: the larger of the two layouts, as the size query)
            const size_t other = sorted_ws_layout(per, d.I, d.H, d.D, d.Q, d.L, samples(d), sizeof(A), sizeof(T), !value_vec_ok<T>(p), rg, sizeof(TV)).total;
            if (other > need) need = other;
        }
        if ((uint64_t)workspace_bytes >= need) return per;
        if (per == 1) break;
    }
    return 0;
}

// MSDA_WS_RECORDS_IN_GRADS with `per` batch elements per pass: every group's share of grad_loc / grad_attn must start on a
// 16-byte boundary.  One pass: always.  Several: required of ONE batch element's share, so that the answer does not
// depend on which group size the call ends up with — the workspace query sizes for ceil(B / n) with any n, the call
// takes the fewest power-of-two passes that fit the workspace it is given, and both must agree.
inline bool records_fit_grads(const Dims &d, int64_t per, size_t elem)
{
    return per >= d.B || ((size_t)(d.Q * d.H * samples(d)) * elem) % 16 == 0;
}

// the size query that belongs to the entry point family of this kernarg type (for the error text below)
inline const char *ws_query_name(const Params &) { return "msda_bwd_workspace_bytes"; }
inline const char *ws_query_name(const RaggedParams &) { return "msda_bwd_ragged_workspace_bytes"; }
inline const char *ws_query_name(const DiscreteParams &) { return "msda_bwd_discrete_workspace_bytes"; }

// Would run_value find a route for this call?  0, or the status it would return — for a caller that must refuse before
// its own first launch (run_bwd_fused on the box rule's discrete kernels); nothing is launched or written here.
template <typename T, typename TV> inline int value_route_status(const Params &p, const Dims &d, const void *workspace, int64_t workspace_bytes)
{
    if (small_path_chosen<T>(d)) return 0;
    const bool fits = sorted_fits<T>(d);
    if (fits && value_batch_per_pass<T, TV>(p, d, workspace, workspace_bytes) > 0) return 0;
    if (option_value_path() != 2 && small_fits<T>(d)) return 0;
    if (!fits) {
        set_error("grad_value: this shape is beyond the sorted pipeline's record format and too large for the single-launch kernel");
        return MSDA_ERR_UNSUPPORTED;
    }
    set_error("grad_value needs a larger 256-byte aligned workspace (got %lld bytes behind the parked points): see the "
              "family's workspace query", (long long)(workspace ? workspace_bytes : 0));
    return MSDA_ERR_BAD_ARG;
}

template <typename T, typename TV = T, typename TS = T, typename PP = Params>
inline int run_value(PP &p, const Dims &d, void *workspace, int64_t workspace_bytes, hipStream_t stream)
{
    using A = typename Traits<T>::acc;
    const int64_t B = d.B, I = d.I, H = d.H, D = d.D, Q = d.Q, L = d.L, P = d.P;
    const bool fits = sorted_fits<T>(d);
    const int64_t per = fits ? value_batch_per_pass<T, TV>(p, d, workspace, workspace_bytes) : 0;
    const bool sorted = per > 0;
    const bool small_path = small_path_chosen<T>(d) ||
                            (option_value_path() != 2 && !sorted && small_fits<T>(d));
    // (no workspace: the single-launch kernel serves whatever fits its LDS)
    int rc = 0;
    if (small_path) {
        note_launch(6, 1);
        note_launch(7, 1);
        for (int slot = 17; slot <= 22; ++slot) note_launch(slot, 0);  // (the sorted pipeline's counters: none of it ran)
        rc = run_value_small<T, TV, TS>(p, d, stream);
    } else if (sorted) {
        note_launch(6, 2);
        note_launch(7, (int)((B + per - 1) / per));
        for (int64_t b0 = 0; b0 < B && rc == 0; b0 += per) {
            const int64_t nb = per < B - b0 ? per : B - b0;
            PP pg = p;
            Dims dg = d;
            dg.B = nb;
            pg.B = (int)nb;
            const size_t ns0 = (size_t)(b0 * Q * H * samples(d));
            pg.loc = static_cast<const unsigned char *>(p.loc) + ns0 * 2 * sizeof(T);
            pg.attn = static_cast<const unsigned char *>(p.attn) + ns0 * sizeof(T);
            pg.grad_out = static_cast<const unsigned char *>(p.grad_out) + (size_t)(b0 * Q * H * D) * sizeof(TS);
            pg.grad_value = static_cast<unsigned char *>(p.grad_value) + (size_t)(b0 * I * H * D) * sizeof(TV);
            advance_value_mask(pg, p, (size_t)(b0 * I), (size_t)(b0 * Q));
            if (p.ent_alt0 != nullptr) {  // this group's own share of the caller's gradient buffers (run_bwd)
                pg.ent_alt0 = static_cast<unsigned char *>(p.ent_alt0) + ns0 * 2 * sizeof(T);
                pg.ent_alt1 = static_cast<unsigned char *>(p.ent_alt1) + ns0 * sizeof(T);
                pg.ent_alt2 = pg.grad_value;
            }
            rc = run_value_sorted<T, TV, TS>(pg, dg, workspace, stream);
        }
    } else if (!fits) {
        set_error("grad_value: this shape is beyond the sorted pipeline's record format (L <= %d, I < 2^22, "
                  "16*D*sizeof(acc) < 2^24, I*4*D*sizeof(acc) < 2^31) and too large for the single-launch kernel",
                  kSortedMaxLevels);
        return MSDA_ERR_UNSUPPORTED;
    } else {
        // (the size msda_bwd_workspace_bytes reports: the larger of the vector and the scalar layout)
        const size_t v1 = sorted_ws_layout(B, I, H, D, Q, L, samples(d), sizeof(A), sizeof(T), true).total;
        const size_t v0 = sorted_ws_layout(B, I, H, D, Q, L, samples(d), sizeof(A), sizeof(T), false).total;
        const size_t m1 = sorted_ws_layout(1, I, H, D, Q, L, samples(d), sizeof(A), sizeof(T), true).total;
        const size_t m0 = sorted_ws_layout(1, I, H, D, Q, L, samples(d), sizeof(A), sizeof(T), false).total;
        set_error("grad_value needs a 256-byte aligned workspace of %s(...) = %zu bytes (at least %zu: one "
                  "batch element per pass); got %lld", ws_query_name(p), v1 > v0 ? v1 : v0, m1 > m0 ? m1 : m0, (long long)(workspace ? workspace_bytes : 0));
        return MSDA_ERR_BAD_ARG;
    }
    if (rc > 0) set_error("backward (grad_value) launch failed: %s", hipGetErrorString((hipError_t)rc));
    return rc;
}

// The float grad_value pipeline on 16-bit rows, for the fused backwards of the 16-bit operators (ParkType).  NOT inline: the
// 16-bit translation units declare their instantiations `extern template` (MSDA_DECLARE_RUN_VALUE_FLOAT) and the
// float-arithmetic 16-bit-storage units, which instantiate these very kernels for themselves anyway and are built with
// their flags, define them (MSDA_DEFINE_RUN_VALUE_FLOAT) — one copy of each kernel in the library.
template <typename TV, typename TS, typename PP>
int run_value_float(PP &p, const Dims &d, void *workspace, int64_t workspace_bytes, hipStream_t stream)
{
    return run_value<float, TV, TS>(p, d, workspace, workspace_bytes, stream);
}
#define MSDA_RUN_VALUE_FLOAT_(KW, TS, PP) \
    KW template int msda::run_value_float<TS, TS, msda::PP>(msda::PP &, const msda::Dims &, void *, int64_t, hipStream_t);
#define MSDA_DECLARE_RUN_VALUE_FLOAT(TS)                                                                                                       \
    MSDA_RUN_VALUE_FLOAT_(extern, TS, Params) MSDA_RUN_VALUE_FLOAT_(extern, TS, RaggedParams) MSDA_RUN_VALUE_FLOAT_(extern, TS, MaskedParams) \
    MSDA_RUN_VALUE_FLOAT_(extern, TS, DiscreteParams) MSDA_RUN_VALUE_FLOAT_(extern, TS, RaggedMaskedParams)
#define MSDA_DEFINE_RUN_VALUE_FLOAT(TS)                                                                                     \
    MSDA_RUN_VALUE_FLOAT_(, TS, Params) MSDA_RUN_VALUE_FLOAT_(, TS, RaggedParams) MSDA_RUN_VALUE_FLOAT_(, TS, MaskedParams) \
    MSDA_RUN_VALUE_FLOAT_(, TS, DiscreteParams) MSDA_RUN_VALUE_FLOAT_(, TS, RaggedMaskedParams)

// PP as run_fwd's.  DiscreteParams (msda_bwd_discrete_<dtype>): grad_value and / or grad_attn — the sampling points have no
// gradient in this mode, so there is no grad_loc buffer, the records always stay in the workspace
// (msda_bwd_discrete_workspace_bytes sizes for that) and nothing is forked
template <typename T, typename TV = T, typename PP = Params> int run_bwd(const Call &c)
{
    const Dims d = make_dims(c);
    hipStream_t stream = static_cast<hipStream_t>(c.stream);
    void *const workspace = c.workspace, *const grad_value = c.grad_value, *const grad_loc = c.grad_loc, *const grad_attn = c.grad_attn;
    const int64_t workspace_bytes = c.workspace_bytes;
    int rc = check_common(d, sizeof(T), c.padding_mode);
    if (rc) return rc;
    const size_t ns = (size_t)(d.B * d.Q * d.H * samples(d));
    if (nothing_sampled(d))
        return zero_outputs({{grad_value, (size_t)(d.B * d.I * d.H * d.D) * sizeof(TV)}, {grad_loc, ns * 2 * sizeof(T)}, {grad_attn, ns * sizeof(T)}}, stream);
    const bool want_value = grad_value != nullptr;
    const bool want_sample = grad_loc != nullptr || grad_attn != nullptr;
    if (!kDiscrete<PP> && want_sample && (grad_loc == nullptr || grad_attn == nullptr)) {
        set_error("grad_loc and grad_attn must be both null or both non-null");
        return MSDA_ERR_BAD_ARG;
    }
    if ((rc = require_buffers({c.grad_out, c.value, c.shapes, c.loc, c.attn})) != 0) return rc;
    if ((rc = check_aligned({{c.value, sizeof(TV)}, {c.grad_out, sizeof(T)}, {grad_value, sizeof(TV)}, {c.loc, 2 * sizeof(T)},
                             {grad_loc, 2 * sizeof(T)}, {c.attn, sizeof(T)}, {grad_attn, sizeof(T)}, {c.shapes, 8}})) != 0)
        return rc;
    PP p{};
    if ((rc = fill_kernarg<TV>(p, c, d)) != 0) return rc;
    // Both halves wanted, one after the other: the sorted records are dead once the gather has run and grad_loc /
    // grad_attn are written only by the sample-gradient kernel, so that kernel goes LAST and the records of as many
    // planes as fit live in those two buffers (three quarters of them in fp32: 61 of 82 MB at c2 @ 10k); the rest go
    // into grad_value itself, which only the finish kernel writes, behind the gather (single-round problems).  The
    // workspace layout shrinks accordingly (msda_bwd_workspace_bytes with MSDA_WS_RECORDS_IN_GRADS); a caller that
    // passes the full size loses nothing.
    bool records_in_grads = !kDiscrete<PP> && want_sample && want_value && option_records_in_grads() != 0 && option_overlap() != 1 &&
                            aligned_to(grad_loc, 16) && aligned_to(grad_attn, 16) && aligned_to(grad_value, 16);
    if (records_in_grads) {
        p.ent_alt0 = grad_loc;
        p.ent_alt1 = grad_attn;
        p.ent_alt2 = grad_value;
        // several passes over the batch: group g's records start g * per * Q * H * S samples into grad_loc / grad_attn,
        // which must be 16-byte aligned too (an odd S makes that common with per-level point counts); otherwise the
        // records stay in the workspace — which msda_bwd_workspace_bytes sizes by the same rule (records_fit_grads)
        const int64_t per = value_batch_per_pass<T, TV>(p, d, workspace, workspace_bytes);
        if (per > 0 && !records_fit_grads(d, per, sizeof(T))) {
            records_in_grads = false;
            p.ent_alt0 = p.ent_alt1 = p.ent_alt2 = nullptr;
        }
    }
    const bool vec_sample = rows_vec_ok(p, c.grad_out);
    // The two halves of the backward are independent: when both are wanted, grad_loc/grad_attn run on a
    // forked side stream next to the grad_value pipeline (fork/join with events: still graph-capturable).
    hipStream_t sample_stream = stream;
    bool forked = false;
    // The fork/join is not free: two event record/wait pairs cost ~14 us of host time and ~19 us of GPU-side
    // latency per backward on this runtime (tools/anyorder_probe.hip; hipExtAnyOrderLaunch, the in-stream
    // alternative, is ignored on gfx9), more under the autograd engine, and the kernels of the two halves lean on the
    // same L2 request path.  Round 3 (plane-major place pass, 59 us of scattered stores) the fork paid from 4M samples
    // with 128-byte rows: c2 @ 10k -3.5 %.  With the level-major place pass (round 4) it no longer does: same-box
    // A/B at c2 @ 10k, fwd+bwd 0.3999-0.4024 ms forked against 0.3912-0.3972 serial (tools/ab_opt.sh - overlap=0).  So
    // the automatic setting never forks; msda_set_option("overlap", 1) still forces it.
    const int ov = option_overlap();
    const bool ov_auto = false;
    if (!kDiscrete<PP> && want_sample && want_value && (ov == 1 || (ov < 0 && ov_auto))) {
        hipStream_t side = side_stream_fork(stream);
        if (side != nullptr) {
            sample_stream = side;
            forked = true;
        }
    }
    auto run_sample = [&]() -> int {
        if constexpr (kDiscrete<PP>)
            return launched(dispatch_discrete<T, 1, TV>(p, vec_sample, sample_stream), "discrete backward (grad_attn)");
        else
            return launched(dispatch_gather<T, 1, TV>(p, vec_sample, sample_stream), "backward (grad_loc/grad_attn)");
    };
    if (want_sample && !records_in_grads) {
        rc = run_sample();
        if (rc) {
            if (forked) (void)side_stream_join(stream);
            return rc;
        }
    }
    if (want_value) rc = run_value<T, TV>(p, d, workspace, workspace_bytes, stream);
    if (rc == 0 && want_sample && records_in_grads) rc = run_sample();  // (its outputs held records until now)
    if (forked) {
        const int jrc = side_stream_join(stream);
        if (rc == 0 && jrc != 0) {
            set_error("joining the side stream failed: %s", hipGetErrorString((hipError_t)jrc));
            rc = jrc;
        }
    }
    return rc;
}

// Module backward with the prologue's chain rule fused in: from grad_out straight to
// grad_value, grad_proj [B,Q,H,L,P,3] and per-head partial sums of grad_reference_points [B,Q,H,ref_dim].
// The first `fused_mat_bytes` of the workspace receive the sampling points / attention weights the kernel
// derives (the grad_value passes read them); the rest is the sorted pipeline's workspace.
// (S: samples of a (b, q, h) unit — L * P, or the sum of the per-level point counts)
inline size_t fused_mat_bytes(int64_t B, int64_t H, int64_t Q, int64_t S, size_t elem)
{
    return align_up((size_t)(B * Q * H * S) * 3 * elem, 256);
}

// The kernarg the grad_value passes behind a fused backward run on.  Per-level reference points change the prologue
// only: grad_value is the UNIFORM pipeline on the parked points (no kernels of its own).
template <typename PP> inline PP &value_pass_params(PP &p) { return p; }
inline Params &value_pass_params(LevelRefParams &p) { return p; }
inline Params &value_pass_params(LevelRefSplitParams &p) { return p; }  // (split projections: the parked points are the pair's)
inline MaskedParams &value_pass_params(LevelRefMaskedParams &p) { return p; }  // (... the plain value-mask pipeline)
// ... and so does Hugging Face's box rule: grad_value is the PER-LEVEL-COUNT pipeline on the parked points.
inline RaggedParams &value_pass_params(HfBoxParams &p) { return p; }
// ... and in front of discrete sampling the DISCRETE pipeline (cell_of's one-corner records)
inline DiscreteParams &value_pass_params(HfBoxDiscreteParams &p) { return p; }
inline DiscreteParams &value_pass_params(ModuleDiscreteParams &p) { return p; }

// PP = RaggedParams (msda_bwd_fused_ragged_<dtype>): per-level point counts, proj / grad_proj [B, Q, H, S, 3]; the
// derived points and weights go to the workspace in the ragged operator's layout and its grad_value pipeline reads them
// PP = LevelRefParams (msda_bwd_fused_levelref_<dtype>): `ref` [B, Q, L, ref_dim], partials [B, Q, H, L, ref_dim]
// PP = HfBoxParams (msda_bwd_fused_hfbox_<dtype>): the per-level-count layout and workspace, transformers' box rule with
// the host's `level_scale` [L] and `offset_scale`
// PP = HfBoxDiscreteParams (msda_bwd_fused_hfbox_discrete_<dtype>): that rule in front of discrete sampling — grad_proj only
// (no partials: c.grad_ref_partial stays null), the same head of the workspace, then the DISCRETE grad_value pipeline
// PP = ModuleDiscreteParams (msda_bwd_fused_discrete_<dtype>): the same with the module's own rule
template <typename T, typename TV = T, typename TS = T, typename PP = Params> int run_bwd_fused(const Call &c)
{
    const Dims d = make_dims(c);
    hipStream_t stream = static_cast<hipStream_t>(c.stream);
    void *const workspace = c.workspace, *const grad_value = c.grad_value;
    const int64_t workspace_bytes = c.workspace_bytes;
    int rc = check_common(d, sizeof(T), c.padding_mode);
    if (rc == 0) rc = check_ref_dim(c.ref_dim);
    if (rc) return rc;
    const size_t ns = (size_t)(d.B * d.Q * d.H * samples(d));
    // (discrete sampling: nothing differentiable reaches the box, there are no partials)
    const size_t nref = kFusedDiscrete<PP> ? 0 : (size_t)(d.B * d.Q * d.H) * (kLevelRef<PP> ? (size_t)d.L : 1) * c.ref_dim;
    // (a buffer of no elements may be null: PyTorch's empty tensors are — a call with Q = 0 has nothing to produce there)
    if ((ns && c.grad_proj == nullptr) || (nref && c.grad_ref_partial == nullptr) || (kSplitProj<PP> && ns && c.grad_logits == nullptr)) {
        set_error("the fused backward always produces grad_proj and the grad_reference_points partials");
        return MSDA_ERR_BAD_ARG;
    }
    if (nothing_sampled(d))  // (split projections: grad_proj is grad_offsets [.., 2], grad_logits apart from it)
        return zero_outputs({{grad_value, (size_t)(d.B * d.I * d.H * d.D) * sizeof(TV)}, {c.grad_proj, ns * (kSplitProj<PP> ? 2 : 3) * sizeof(TS)},
                             {c.grad_logits, kSplitProj<PP> ? ns * sizeof(TS) : 0}, {c.grad_ref_partial, nref * sizeof(T)}}, stream);
    if ((rc = require_buffers({c.grad_out, c.value, c.shapes, c.proj, c.ref})) != 0) return rc;
    if (kSplitProj<PP> && (rc = require_buffers({c.logits})) != 0) return rc;
    if (!kFusedDiscrete<PP> && fused_limit_exceeded(d)) {
        set_error("projection too large for 32-bit sample offsets");
        return MSDA_ERR_TOO_LARGE;
    }
    if ((rc = check_aligned({{c.value, sizeof(TV)}, {c.grad_out, sizeof(TS)}, {grad_value, sizeof(TV)}, {c.proj, sizeof(TS)},
                             {c.grad_proj, sizeof(TS)}, {c.ref, sizeof(T)}, {c.grad_ref_partial, sizeof(T)}, {c.shapes, 8}})) != 0)
        return rc;
    if (kSplitProj<PP> && (rc = check_aligned({{c.logits, sizeof(TS)}, {c.grad_logits, sizeof(TS)}})) != 0) return rc;
    const bool want_value = grad_value != nullptr;
    // the derived points and weights are parked in float by the 16-bit operators too (ParkType), and their grad_value passes
    // are the float pipeline on 16-bit rows — so those calls have the float limits, as the workspace queries say
    using MT = ParkType<T>;
    if (want_value && sizeof(MT) != sizeof(T) && common_limits_exceeded(d, (int64_t)sizeof(MT))) {
        set_error("tensor too large for the fused backward's float32 grad_value passes");
        return MSDA_ERR_TOO_LARGE;
    }
    const size_t mat = fused_mat_bytes(d.B, d.H, d.Q, samples(d), sizeof(MT));
    if (want_value && (workspace == nullptr || !aligned_to(workspace, 256) || (uint64_t)workspace_bytes < mat)) {
        set_error("the fused backward needs a 256-byte aligned workspace of at least %zu bytes for grad_value", mat);
        return MSDA_ERR_BAD_ARG;
    }
    PP p{};
    if ((rc = fill_kernarg<TV>(p, c, d)) != 0) return rc;
    p.loc = c.proj;
    p.grad_loc = c.grad_proj;
    p.grad_attn = c.grad_ref_partial;
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    if (want_value) {
        p.mat_loc = ws;
        p.mat_attn = ws + ns * 2 * sizeof(MT);
    }
    if constexpr (kFusedDiscrete<PP>) {
        // this family refuses a grad_value call it cannot finish BEFORE its first kernel (run_value would say the same
        // behind it)
        if (want_value && (rc = value_route_status<MT, TV>(p, d, ws + mat, workspace_bytes - (int64_t)mat)) != 0) return rc;
        rc = launched(dispatch_hfbox_discrete<T, 1, TV, TS>(p, rows_vec_ok(p, c.grad_out), stream), "fused discrete backward");
    } else {
        rc = launched(dispatch_gather<T, 3, TV, TS>(p, rows_vec_ok(p, c.grad_out), stream), "fused backward");
    }
    if (rc != 0) return rc;
    if (want_value) {
        p.loc = p.mat_loc;
        p.attn = p.mat_attn;
        p.ref = nullptr;
        p.ref_dim = 0;
        if constexpr (sizeof(MT) != sizeof(T))
            rc = run_value_float<TV, TS>(value_pass_params(p), d, ws + mat, workspace_bytes - (int64_t)mat, stream);
        else
            rc = run_value<T, TV, TS>(value_pass_params(p), d, ws + mat, workspace_bytes - (int64_t)mat, stream);
    }
    return rc;
}

}  // namespace msda

// ---- the extern "C" entry points (include/msda_hip.h has the argument lists): each fills a Call by name — the groups
//      below take the arguments that every list of their kind has, under the header's names — and calls its run_* ----
#define MSDA_TAKE_SIZES c.B = B; c.I = I; c.H = H; c.D = D; c.Q = Q; c.L = L; c.value_row_stride = value_row_stride; c.stream = stream;
#define MSDA_TAKE_MODES c.padding_mode = padding_mode; c.align_corners = align_corners;
#define MSDA_TAKE_FWD msda::Call c; c.value = value; c.shapes = shapes; c.loc = loc; c.attn = attn; c.out = out; MSDA_TAKE_SIZES
#define MSDA_TAKE_FWD_FUSED \
    msda::Call c; c.value = value; c.shapes = shapes; c.proj = proj; c.ref = ref; c.out = out; c.ref_dim = ref_dim; MSDA_TAKE_SIZES MSDA_TAKE_MODES
#define MSDA_TAKE_WORKSPACE c.max_level_cells = max_level_cells; c.workspace = workspace; c.workspace_bytes = workspace_bytes;
#define MSDA_TAKE_BWD /* (grad_loc: not in discrete sampling's list) */ \
    msda::Call c; c.grad_out = grad_out; c.value = value; c.shapes = shapes; c.loc = loc; c.attn = attn; c.grad_value = grad_value; \
    c.grad_attn = grad_attn; MSDA_TAKE_SIZES MSDA_TAKE_WORKSPACE
#define MSDA_TAKE_BWD_FUSED \
    msda::Call c; c.grad_out = grad_out; c.value = value; c.shapes = shapes; c.proj = proj; c.ref = ref; c.grad_value = grad_value; \
    c.grad_proj = grad_proj; c.grad_ref_partial = grad_ref_partial; c.ref_dim = ref_dim; MSDA_TAKE_SIZES MSDA_TAKE_MODES MSDA_TAKE_WORKSPACE
// per-level point counts: checked once, here, and their maximum and sum noted in the record
#define MSDA_TAKE_COUNTS c.points_per_level = points_per_level; if (const int rc = msda::take_counts(c)) return rc;
// ... and Hugging Face's box rule behind them
#define MSDA_TAKE_BOX_RULE \
    c.level_scale = level_scale; c.offset_scale = offset_scale; if (const int rc = msda::box_rule_args(level_scale, L, ref_dim)) return rc;

#define MSDA_DEFINE_ENTRY_POINTS2(SUF, T, TV)                                                                        \
    extern "C" int msda_fwd_##SUF(const void *value, const int64_t *shapes, const void *loc, const void *attn,  \
                                  void *out, int64_t B, int64_t I, int64_t H, int64_t D, int64_t Q, int64_t L,  \
                                  int64_t P, int padding_mode, int align_corners, int64_t value_row_stride,     \
                                  void *stream)                                                                  \
    {                                                                                                            \
        MSDA_TAKE_FWD MSDA_TAKE_MODES c.P = P;                                                                   \
        return msda::run_fwd<T, TV>(c);                                                                          \
    }                                                                                                            \
    extern "C" int msda_fwd_fused_##SUF(const void *value, const int64_t *shapes, const void *proj,             \
                                        const void *ref, void *out, int64_t B, int64_t I, int64_t H, int64_t D,  \
                                        int64_t Q, int64_t L, int64_t P, int ref_dim, int padding_mode,          \
                                        int align_corners, int64_t value_row_stride, void *stream)               \
    {                                                                                                            \
        MSDA_TAKE_FWD_FUSED c.P = P;                                                                             \
        return msda::run_fwd_fused<T, TV>(c);                                                                    \
    }                                                                                                            \
    extern "C" int msda_bwd_##SUF(const void *grad_out, const void *value, const int64_t *shapes,               \
                                  const void *loc, const void *attn, void *grad_value, void *grad_loc,          \
                                  void *grad_attn, int64_t B, int64_t I, int64_t H, int64_t D, int64_t Q,       \
                                  int64_t L, int64_t P, int padding_mode, int align_corners,                    \
                                  int64_t max_level_cells, int64_t value_row_stride, void *workspace,           \
                                  int64_t workspace_bytes, void *stream)                                         \
    {                                                                                                            \
        MSDA_TAKE_BWD MSDA_TAKE_MODES c.grad_loc = grad_loc; c.P = P;                                            \
        return msda::run_bwd<T, TV>(c);                                                                          \
    }                                                                                                            \
    extern "C" int msda_bwd_fused_##SUF(const void *grad_out, const void *value, const int64_t *shapes,         \
                                        const void *proj, const void *ref, void *grad_value, void *grad_proj,   \
                                        void *grad_ref_partial, int64_t B, int64_t I, int64_t H, int64_t D,      \
                                        int64_t Q, int64_t L, int64_t P, int ref_dim, int padding_mode,          \
                                        int align_corners, int64_t max_level_cells, int64_t value_row_stride,    \
                                        void *workspace, int64_t workspace_bytes, void *stream)                  \
    {                                                                                                            \
        MSDA_TAKE_BWD_FUSED c.P = P;                                                                             \
        return msda::run_bwd_fused<T, TV>(c);                                                                    \
    }                                                                                                            \
    extern "C" int msda_fwd_ragged_##SUF(const void *value, const int64_t *shapes, const void *loc, const void *attn, \
                                         void *out, int64_t B, int64_t I, int64_t H, int64_t D, int64_t Q, int64_t L, \
                                         const int32_t *points_per_level, int padding_mode, int align_corners,    \
                                         int64_t value_row_stride, void *stream)                                 \
    {                                                                                                            \
        MSDA_TAKE_FWD MSDA_TAKE_MODES MSDA_TAKE_COUNTS                                                           \
        return msda::run_fwd<T, TV, msda::RaggedParams>(c);                                                      \
    }                                                                                                            \
    extern "C" int msda_bwd_ragged_##SUF(const void *grad_out, const void *value, const int64_t *shapes,        \
                                         const void *loc, const void *attn, void *grad_value, void *grad_loc,   \
                                         void *grad_attn, int64_t B, int64_t I, int64_t H, int64_t D, int64_t Q, \
                                         int64_t L, const int32_t *points_per_level, int padding_mode,           \
                                         int align_corners, int64_t max_level_cells, int64_t value_row_stride,   \
                                         void *workspace, int64_t workspace_bytes, void *stream)                 \
    {                                                                                                            \
        MSDA_TAKE_BWD MSDA_TAKE_MODES c.grad_loc = grad_loc; MSDA_TAKE_COUNTS                                    \
        return msda::run_bwd<T, TV, msda::RaggedParams>(c);                                                      \
    }                                                                                                            \
    extern "C" int msda_fwd_discrete_##SUF(const void *value, const int64_t *shapes, const void *loc,           \
                                           const void *attn, void *out, int64_t B, int64_t I, int64_t H,         \
                                           int64_t D, int64_t Q, int64_t L, const int32_t *points_per_level,     \
                                           int64_t value_row_stride, void *stream)                               \
    {                                                                                                            \
        MSDA_TAKE_FWD MSDA_TAKE_COUNTS                                                                           \
        return msda::run_fwd<T, TV, msda::DiscreteParams>(c);                                                    \
    }                                                                                                            \
    extern "C" int msda_bwd_discrete_##SUF(const void *grad_out, const void *value, const int64_t *shapes,      \
                                           const void *loc, const void *attn, void *grad_value, void *grad_attn, \
                                           int64_t B, int64_t I, int64_t H, int64_t D, int64_t Q, int64_t L,     \
                                           const int32_t *points_per_level, int64_t max_level_cells,             \
                                           int64_t value_row_stride, void *workspace, int64_t workspace_bytes,   \
                                           void *stream)                                                         \
    {                                                                                                            \
        MSDA_TAKE_BWD MSDA_TAKE_COUNTS                                                                           \
        return msda::run_bwd<T, TV, msda::DiscreteParams>(c);                                                    \
    }                                                                                                            \
    MSDA_DEFINE_MASKED_ENTRY_POINTS(SUF, T, TV)                                                                   \
    MSDA_DEFINE_QMASKED_ENTRY_POINTS(SUF, T, TV)                                                                  \
    MSDA_DEFINE_FUSED_RAGGED_ENTRY_POINTS(SUF, T, TV, T)                                                          \
    MSDA_DEFINE_FUSED_LEVELREF_ENTRY_POINTS(SUF, T, TV, T)                                                        \
    MSDA_DEFINE_FUSED_LEVELREF_SPLIT_ENTRY_POINTS(SUF, T, TV, T)                                                  \
    MSDA_DEFINE_FUSED_LEVELREF_MASKED_ENTRY_POINTS(SUF, T, TV, T)                                                 \
    MSDA_DEFINE_FUSED_LEVELREF_QMASKED_ENTRY_POINTS(SUF, T, TV, T)                                                \
    MSDA_DEFINE_FUSED_HFBOX_ENTRY_POINTS(SUF, T, TV, T)                                                           \
    MSDA_DEFINE_FUSED_HFBOX_DISCRETE_ENTRY_POINTS(SUF, T, TV, T)                                                  \
    MSDA_DEFINE_FUSED_MODULE_DISCRETE_ENTRY_POINTS(SUF, T, TV, T)                                                 \
    MSDA_DEFINE_MODULE_MASK_ENTRY_POINTS(SUF, T, TV, T)

// the module's kernels with a separate 16-bit STORAGE type TS for value, projection, out and their gradients next to
// fp32 reference points and fp32 arithmetic (msda_fwd_fused_f32_sbf16 / _sf16): fused entry points only
#define MSDA_DEFINE_FUSED_STORAGE_ENTRY_POINTS(SUF, T, TS)                                                        \
    extern "C" int msda_fwd_fused_##SUF(const void *value, const int64_t *shapes, const void *proj,             \
                                        const void *ref, void *out, int64_t B, int64_t I, int64_t H, int64_t D,  \
                                        int64_t Q, int64_t L, int64_t P, int ref_dim, int padding_mode,          \
                                        int align_corners, int64_t value_row_stride, void *stream)               \
    {                                                                                                            \
        MSDA_TAKE_FWD_FUSED c.P = P;                                                                             \
        return msda::run_fwd_fused<T, TS, TS>(c);                                                                \
    }                                                                                                            \
    extern "C" int msda_bwd_fused_##SUF(const void *grad_out, const void *value, const int64_t *shapes,         \
                                        const void *proj, const void *ref, void *grad_value, void *grad_proj,   \
                                        void *grad_ref_partial, int64_t B, int64_t I, int64_t H, int64_t D,      \
                                        int64_t Q, int64_t L, int64_t P, int ref_dim, int padding_mode,          \
                                        int align_corners, int64_t max_level_cells, int64_t value_row_stride,    \
                                        void *workspace, int64_t workspace_bytes, void *stream)                  \
    {                                                                                                            \
        MSDA_TAKE_BWD_FUSED c.P = P;                                                                             \
        return msda::run_bwd_fused<T, TS, TS>(c);                                                                \
    }                                                                                                            \
    MSDA_DEFINE_FUSED_RAGGED_ENTRY_POINTS(SUF, T, TS, TS)                                                         \
    MSDA_DEFINE_FUSED_LEVELREF_ENTRY_POINTS(SUF, T, TS, TS)                                                       \
    MSDA_DEFINE_FUSED_LEVELREF_SPLIT_ENTRY_POINTS(SUF, T, TS, TS)                                                 \
    MSDA_DEFINE_FUSED_LEVELREF_MASKED_ENTRY_POINTS(SUF, T, TS, TS)                                                \
    MSDA_DEFINE_FUSED_LEVELREF_QMASKED_ENTRY_POINTS(SUF, T, TS, TS)                                               \
    MSDA_DEFINE_FUSED_HFBOX_ENTRY_POINTS(SUF, T, TS, TS)                                                          \
    MSDA_DEFINE_FUSED_HFBOX_DISCRETE_ENTRY_POINTS(SUF, T, TS, TS)                                                 \
    MSDA_DEFINE_FUSED_MODULE_DISCRETE_ENTRY_POINTS(SUF, T, TS, TS)                                                \
    MSDA_DEFINE_MODULE_MASK_ENTRY_POINTS(SUF, T, TS, TS)

// the module's fused kernels with per-level point counts: msda_{fwd,bwd}_fused_ragged_<suffix> (T arithmetic and reference
// points, TV value rows, TS projection / out / their gradients)
#define MSDA_DEFINE_FUSED_RAGGED_ENTRY_POINTS(SUF, T, TV, TS)                                                     \
    extern "C" int msda_fwd_fused_ragged_##SUF(const void *value, const int64_t *shapes, const void *proj,       \
                                               const void *ref, void *out, int64_t B, int64_t I, int64_t H,       \
                                               int64_t D, int64_t Q, int64_t L, const int32_t *points_per_level,  \
                                               int ref_dim, int padding_mode, int align_corners,                  \
                                               int64_t value_row_stride, void *stream)                            \
    {                                                                                                            \
        MSDA_TAKE_FWD_FUSED MSDA_TAKE_COUNTS                                                                     \
        return msda::run_fwd_fused<T, TV, TS, msda::RaggedParams>(c);                                            \
    }                                                                                                            \
    extern "C" int msda_bwd_fused_ragged_##SUF(const void *grad_out, const void *value, const int64_t *shapes,   \
                                               const void *proj, const void *ref, void *grad_value,               \
                                               void *grad_proj, void *grad_ref_partial, int64_t B, int64_t I,     \
                                               int64_t H, int64_t D, int64_t Q, int64_t L,                        \
                                               const int32_t *points_per_level, int ref_dim, int padding_mode,    \
                                               int align_corners, int64_t max_level_cells,                        \
                                               int64_t value_row_stride, void *workspace,                         \
                                               int64_t workspace_bytes, void *stream)                             \
    {                                                                                                            \
        MSDA_TAKE_BWD_FUSED MSDA_TAKE_COUNTS                                                                     \
        return msda::run_bwd_fused<T, TV, TS, msda::RaggedParams>(c);                                            \
    }

// the module's fused kernels for per-level reference points and transformers' point rule:
// msda_{fwd,bwd}_fused_levelref_<suffix>, the argument lists of msda_{fwd,bwd}_fused_<suffix> (`ref` [B, Q, L, ref_dim],
// the grad_reference_points partials [B, Q, H, L, ref_dim])
#define MSDA_DEFINE_FUSED_LEVELREF_ENTRY_POINTS(SUF, T, TV, TS)                                                   \
    extern "C" int msda_fwd_fused_levelref_##SUF(const void *value, const int64_t *shapes, const void *proj,     \
                                                 const void *ref, void *out, int64_t B, int64_t I, int64_t H,     \
                                                 int64_t D, int64_t Q, int64_t L, int64_t P, int ref_dim,         \
                                                 int padding_mode, int align_corners, int64_t value_row_stride,   \
                                                 void *stream)                                                    \
    {                                                                                                            \
        MSDA_TAKE_FWD_FUSED c.P = P;                                                                             \
        return msda::run_fwd_fused<T, TV, TS, msda::LevelRefParams>(c);                                          \
    }                                                                                                            \
    extern "C" int msda_bwd_fused_levelref_##SUF(const void *grad_out, const void *value, const int64_t *shapes, \
                                                 const void *proj, const void *ref, void *grad_value,             \
                                                 void *grad_proj, void *grad_ref_partial, int64_t B, int64_t I,   \
                                                 int64_t H, int64_t D, int64_t Q, int64_t L, int64_t P,           \
                                                 int ref_dim, int padding_mode, int align_corners,                \
                                                 int64_t max_level_cells, int64_t value_row_stride,               \
                                                 void *workspace, int64_t workspace_bytes, void *stream)          \
    {                                                                                                            \
        MSDA_TAKE_BWD_FUSED c.P = P;                                                                             \
        return msda::run_bwd_fused<T, TV, TS, msda::LevelRefParams>(c);                                          \
    }

// ... and the same pair on SPLIT projections: msda_{fwd,bwd}_fused_levelref_split_<suffix> — `offsets` [B, Q, H, L, P, 2]
// and `logits` [B, Q, H, L, P] in place of `proj`, `grad_offsets` and `grad_logits` in place of `grad_proj`; every check,
// in the pair's order, and the pair's workspace (msda_bwd_fused_workspace_bytes answers for it)
#define MSDA_DEFINE_FUSED_LEVELREF_SPLIT_ENTRY_POINTS(SUF, T, TV, TS)                                             \
    extern "C" int msda_fwd_fused_levelref_split_##SUF(const void *value, const int64_t *shapes,                 \
                                                       const void *offsets, const void *logits, const void *ref,  \
                                                       void *out, int64_t B, int64_t I, int64_t H, int64_t D,     \
                                                       int64_t Q, int64_t L, int64_t P, int ref_dim,              \
                                                       int padding_mode, int align_corners,                       \
                                                       int64_t value_row_stride, void *stream)                    \
    {                                                                                                            \
        const void *const proj = offsets;                                                                        \
        MSDA_TAKE_FWD_FUSED c.P = P; c.logits = logits;                                                          \
        return msda::run_fwd_fused<T, TV, TS, msda::LevelRefSplitParams>(c);                                     \
    }                                                                                                            \
    extern "C" int msda_bwd_fused_levelref_split_##SUF(const void *grad_out, const void *value,                  \
                                                       const int64_t *shapes, const void *offsets,                \
                                                       const void *logits, const void *ref, void *grad_value,     \
                                                       void *grad_offsets, void *grad_logits,                     \
                                                       void *grad_ref_partial, int64_t B, int64_t I, int64_t H,   \
                                                       int64_t D, int64_t Q, int64_t L, int64_t P, int ref_dim,   \
                                                       int padding_mode, int align_corners,                       \
                                                       int64_t max_level_cells, int64_t value_row_stride,         \
                                                       void *workspace, int64_t workspace_bytes, void *stream)    \
    {                                                                                                            \
        const void *const proj = offsets;                                                                        \
        void *const grad_proj = grad_offsets;                                                                    \
        MSDA_TAKE_BWD_FUSED c.P = P; c.logits = logits; c.grad_logits = grad_logits;                             \
        return msda::run_bwd_fused<T, TV, TS, msda::LevelRefSplitParams>(c);                                     \
    }

// the module's fused kernels for Hugging Face's box rule with per-level point counts (D-FINE, DEIMv2, RT-DETRv2):
// msda_{fwd,bwd}_fused_hfbox_<suffix>, the argument lists of msda_{fwd,bwd}_fused_ragged_<suffix> with the host array
// `level_scale` [L] (fp32) and `offset_scale` behind `points_per_level`; boxes only (`ref` [B, Q, 4])
#define MSDA_DEFINE_FUSED_HFBOX_ENTRY_POINTS(SUF, T, TV, TS)                                                      \
    extern "C" int msda_fwd_fused_hfbox_##SUF(const void *value, const int64_t *shapes, const void *proj,        \
                                              const void *ref, void *out, int64_t B, int64_t I, int64_t H,        \
                                              int64_t D, int64_t Q, int64_t L, const int32_t *points_per_level,   \
                                              const float *level_scale, double offset_scale, int ref_dim,         \
                                              int padding_mode, int align_corners, int64_t value_row_stride,      \
                                              void *stream)                                                       \
    {                                                                                                            \
        MSDA_TAKE_FWD_FUSED MSDA_TAKE_COUNTS MSDA_TAKE_BOX_RULE                                                  \
        return msda::run_fwd_fused<T, TV, TS, msda::HfBoxParams>(c);                                             \
    }                                                                                                            \
    extern "C" int msda_bwd_fused_hfbox_##SUF(const void *grad_out, const void *value, const int64_t *shapes,    \
                                              const void *proj, const void *ref, void *grad_value,                \
                                              void *grad_proj, void *grad_ref_partial, int64_t B, int64_t I,      \
                                              int64_t H, int64_t D, int64_t Q, int64_t L,                         \
                                              const int32_t *points_per_level, const float *level_scale,          \
                                              double offset_scale, int ref_dim, int padding_mode,                 \
                                              int align_corners, int64_t max_level_cells,                         \
                                              int64_t value_row_stride, void *workspace,                          \
                                              int64_t workspace_bytes, void *stream)                              \
    {                                                                                                            \
        MSDA_TAKE_BWD_FUSED MSDA_TAKE_COUNTS MSDA_TAKE_BOX_RULE                                                  \
        return msda::run_bwd_fused<T, TV, TS, msda::HfBoxParams>(c);                                             \
    }

// the box rule in front of DISCRETE sampling (decoder_method = "discrete"): msda_{fwd,bwd}_fused_hfbox_discrete_<suffix>, the
// hfbox pair's lists without ref_dim, padding_mode, align_corners (discrete sampling has none) and grad_ref_partial (nothing
// differentiable reaches the box)
#define MSDA_DEFINE_FUSED_HFBOX_DISCRETE_ENTRY_POINTS(SUF, T, TV, TS)                                             \
    extern "C" int msda_fwd_fused_hfbox_discrete_##SUF(const void *value, const int64_t *shapes, const void *proj, \
                                                       const void *ref, void *out, int64_t B, int64_t I,          \
                                                       int64_t H, int64_t D, int64_t Q, int64_t L,                \
                                                       const int32_t *points_per_level, const float *level_scale, \
                                                       double offset_scale, int64_t value_row_stride,             \
                                                       void *stream)                                              \
    {                                                                                                            \
        const int ref_dim = 4;                                                                                   \
        msda::Call c; c.value = value; c.shapes = shapes; c.proj = proj; c.ref = ref; c.out = out;               \
        c.ref_dim = ref_dim; MSDA_TAKE_SIZES MSDA_TAKE_COUNTS MSDA_TAKE_BOX_RULE                                 \
        return msda::run_fwd_fused<T, TV, TS, msda::HfBoxDiscreteParams>(c);                                     \
    }                                                                                                            \
    extern "C" int msda_bwd_fused_hfbox_discrete_##SUF(const void *grad_out, const void *value,                  \
                                                       const int64_t *shapes, const void *proj, const void *ref,  \
                                                       void *grad_value, void *grad_proj, int64_t B, int64_t I,   \
                                                       int64_t H, int64_t D, int64_t Q, int64_t L,                \
                                                       const int32_t *points_per_level, const float *level_scale, \
                                                       double offset_scale, int64_t max_level_cells,              \
                                                       int64_t value_row_stride, void *workspace,                 \
                                                       int64_t workspace_bytes, void *stream)                     \
    {                                                                                                            \
        const int ref_dim = 4;                                                                                   \
        msda::Call c; c.grad_out = grad_out; c.value = value; c.shapes = shapes; c.proj = proj; c.ref = ref;     \
        c.grad_value = grad_value; c.grad_proj = grad_proj; c.ref_dim = ref_dim;                                 \
        MSDA_TAKE_SIZES MSDA_TAKE_WORKSPACE MSDA_TAKE_COUNTS MSDA_TAKE_BOX_RULE                                  \
        return msda::run_bwd_fused<T, TV, TS, msda::HfBoxDiscreteParams>(c);                                     \
    }

// the reference module's rule in front of DISCRETE sampling (MultiscaleDeformableAttention(sampling_mode="discrete")):
// msda_{fwd,bwd}_fused_discrete_<suffix>, the hfbox-discrete pair's lists with `int ref_dim` (2 or 4) in place of
// `level_scale, offset_scale`
#define MSDA_DEFINE_FUSED_MODULE_DISCRETE_ENTRY_POINTS(SUF, T, TV, TS)                                            \
    extern "C" int msda_fwd_fused_discrete_##SUF(const void *value, const int64_t *shapes, const void *proj,     \
                                                 const void *ref, void *out, int64_t B, int64_t I, int64_t H,     \
                                                 int64_t D, int64_t Q, int64_t L, const int32_t *points_per_level, \
                                                 int ref_dim, int64_t value_row_stride, void *stream)             \
    {                                                                                                            \
        msda::Call c; c.value = value; c.shapes = shapes; c.proj = proj; c.ref = ref; c.out = out;               \
        c.ref_dim = ref_dim; MSDA_TAKE_SIZES MSDA_TAKE_COUNTS                                                    \
        if (const int rc = msda::check_ref_dim(ref_dim)) return rc;                                              \
        return msda::run_fwd_fused<T, TV, TS, msda::ModuleDiscreteParams>(c);                                    \
    }                                                                                                            \
    extern "C" int msda_bwd_fused_discrete_##SUF(const void *grad_out, const void *value, const int64_t *shapes, \
                                                 const void *proj, const void *ref, void *grad_value,             \
                                                 void *grad_proj, int64_t B, int64_t I, int64_t H, int64_t D,     \
                                                 int64_t Q, int64_t L, const int32_t *points_per_level,           \
                                                 int ref_dim, int64_t max_level_cells, int64_t value_row_stride,  \
                                                 void *workspace, int64_t workspace_bytes, void *stream)          \
    {                                                                                                            \
        msda::Call c; c.grad_out = grad_out; c.value = value; c.shapes = shapes; c.proj = proj; c.ref = ref;     \
        c.grad_value = grad_value; c.grad_proj = grad_proj; c.ref_dim = ref_dim;                                 \
        MSDA_TAKE_SIZES MSDA_TAKE_WORKSPACE MSDA_TAKE_COUNTS                                                     \
        if (const int rc = msda::check_ref_dim(ref_dim)) return rc;                                              \
        return msda::run_bwd_fused<T, TV, TS, msda::ModuleDiscreteParams>(c);                                    \
    }

// the value-mask twins: msda_{fwd,bwd}_masked_<suffix> and msda_{fwd,bwd}_fused_levelref_masked_<suffix> — the twins'
// argument lists with `value_mask` ([B, I] bytes, non-zero = real pixel) behind `value`; a null mask is an argument error
// (the caller without a mask calls the twin), refused before any other argument is looked at
#define MSDA_MASK_REQUIRED(NAME)                                                                                 \
    if (value_mask == nullptr) {                                                                                 \
        msda::set_error(NAME ": value_mask is null (call the unmasked entry point instead)");                    \
        return MSDA_ERR_BAD_ARG;                                                                                 \
    }
#define MSDA_DEFINE_MASKED_ENTRY_POINTS(SUF, T, TV)                                                              \
    extern "C" int msda_fwd_masked_##SUF(const void *value, const uint8_t *value_mask, const int64_t *shapes,   \
                                         const void *loc, const void *attn, void *out, int64_t B, int64_t I,    \
                                         int64_t H, int64_t D, int64_t Q, int64_t L, int64_t P, int padding_mode, \
                                         int align_corners, int64_t value_row_stride, void *stream)             \
    {                                                                                                            \
        MSDA_MASK_REQUIRED("msda_fwd_masked")                                                                    \
        MSDA_TAKE_FWD MSDA_TAKE_MODES c.P = P; c.value_mask = value_mask;                                        \
        return msda::run_fwd<T, TV, msda::MaskedParams>(c);                                                      \
    }                                                                                                            \
    extern "C" int msda_bwd_masked_##SUF(const void *grad_out, const void *value, const uint8_t *value_mask,    \
                                         const int64_t *shapes, const void *loc, const void *attn,              \
                                         void *grad_value, void *grad_loc, void *grad_attn, int64_t B, int64_t I, \
                                         int64_t H, int64_t D, int64_t Q, int64_t L, int64_t P, int padding_mode, \
                                         int align_corners, int64_t max_level_cells, int64_t value_row_stride,   \
                                         void *workspace, int64_t workspace_bytes, void *stream)                 \
    {                                                                                                            \
        MSDA_MASK_REQUIRED("msda_bwd_masked")                                                                    \
        MSDA_TAKE_BWD MSDA_TAKE_MODES c.grad_loc = grad_loc; c.P = P; c.value_mask = value_mask;                 \
        return msda::run_bwd<T, TV, msda::MaskedParams>(c);                                                      \
    }
#define MSDA_DEFINE_FUSED_LEVELREF_MASKED_ENTRY_POINTS(SUF, T, TV, TS)                                            \
    extern "C" int msda_fwd_fused_levelref_masked_##SUF(const void *value, const uint8_t *value_mask,           \
                                                        const int64_t *shapes, const void *proj, const void *ref, \
                                                        void *out, int64_t B, int64_t I, int64_t H, int64_t D,   \
                                                        int64_t Q, int64_t L, int64_t P, int ref_dim,            \
                                                        int padding_mode, int align_corners,                     \
                                                        int64_t value_row_stride, void *stream)                  \
    {                                                                                                            \
        MSDA_MASK_REQUIRED("msda_fwd_fused_levelref_masked")                                                     \
        MSDA_TAKE_FWD_FUSED c.P = P; c.value_mask = value_mask;                                                  \
        return msda::run_fwd_fused<T, TV, TS, msda::LevelRefMaskedParams>(c);                                    \
    }                                                                                                            \
    extern "C" int msda_bwd_fused_levelref_masked_##SUF(                                                         \
        const void *grad_out, const void *value, const uint8_t *value_mask, const int64_t *shapes,              \
        const void *proj, const void *ref, void *grad_value, void *grad_proj, void *grad_ref_partial, int64_t B, \
        int64_t I, int64_t H, int64_t D, int64_t Q, int64_t L, int64_t P, int ref_dim, int padding_mode,         \
        int align_corners, int64_t max_level_cells, int64_t value_row_stride, void *workspace,                   \
        int64_t workspace_bytes, void *stream)                                                                   \
    {                                                                                                            \
        MSDA_MASK_REQUIRED("msda_bwd_fused_levelref_masked")                                                     \
        MSDA_TAKE_BWD_FUSED c.P = P; c.value_mask = value_mask;                                                  \
        return msda::run_bwd_fused<T, TV, TS, msda::LevelRefMaskedParams>(c);                                    \
    }

// the query-mask entry points: msda_{fwd,bwd}_qmasked_<suffix> and msda_{fwd,bwd}_fused_levelref_qmasked_<suffix> — the
// _masked_ twins' argument lists with `query_mask` ([B, Q] bytes, non-zero = real query) behind `value_mask`, on the twins'
// kernels (MaskedParams::qmask).  Both masks are required: a null one is an argument error, refused before any other
// argument is looked at (a caller without a value mask passes all ones).
#define MSDA_BOTH_MASKS_REQUIRED(NAME)                                                                           \
    if (value_mask == nullptr || query_mask == nullptr) {                                                        \
        msda::set_error(NAME ": %s is null (both masks are required; all ones for a mask the caller does not have)", \
                        value_mask == nullptr ? "value_mask" : "query_mask");                                    \
        return MSDA_ERR_BAD_ARG;                                                                                 \
    }
#define MSDA_DEFINE_QMASKED_ENTRY_POINTS(SUF, T, TV)                                                             \
    extern "C" int msda_fwd_qmasked_##SUF(const void *value, const uint8_t *value_mask, const uint8_t *query_mask, \
                                          const int64_t *shapes, const void *loc, const void *attn, void *out,   \
                                          int64_t B, int64_t I, int64_t H, int64_t D, int64_t Q, int64_t L,      \
                                          int64_t P, int padding_mode, int align_corners,                        \
                                          int64_t value_row_stride, void *stream)                                \
    {                                                                                                            \
        MSDA_BOTH_MASKS_REQUIRED("msda_fwd_qmasked")                                                             \
        MSDA_TAKE_FWD MSDA_TAKE_MODES c.P = P; c.value_mask = value_mask; c.query_mask = query_mask;             \
        return msda::run_fwd<T, TV, msda::MaskedParams>(c);                                                      \
    }                                                                                                            \
    extern "C" int msda_bwd_qmasked_##SUF(const void *grad_out, const void *value, const uint8_t *value_mask,   \
                                          const uint8_t *query_mask, const int64_t *shapes, const void *loc,     \
                                          const void *attn, void *grad_value, void *grad_loc, void *grad_attn,   \
                                          int64_t B, int64_t I, int64_t H, int64_t D, int64_t Q, int64_t L,      \
                                          int64_t P, int padding_mode, int align_corners,                        \
                                          int64_t max_level_cells, int64_t value_row_stride, void *workspace,    \
                                          int64_t workspace_bytes, void *stream)                                 \
    {                                                                                                            \
        MSDA_BOTH_MASKS_REQUIRED("msda_bwd_qmasked")                                                             \
        MSDA_TAKE_BWD MSDA_TAKE_MODES c.grad_loc = grad_loc; c.P = P; c.value_mask = value_mask;                 \
        c.query_mask = query_mask;                                                                               \
        return msda::run_bwd<T, TV, msda::MaskedParams>(c);                                                      \
    }
#define MSDA_DEFINE_FUSED_LEVELREF_QMASKED_ENTRY_POINTS(SUF, T, TV, TS)                                           \
    extern "C" int msda_fwd_fused_levelref_qmasked_##SUF(const void *value, const uint8_t *value_mask,          \
                                                         const uint8_t *query_mask, const int64_t *shapes,       \
                                                         const void *proj, const void *ref, void *out, int64_t B, \
                                                         int64_t I, int64_t H, int64_t D, int64_t Q, int64_t L,  \
                                                         int64_t P, int ref_dim, int padding_mode,               \
                                                         int align_corners, int64_t value_row_stride,            \
                                                         void *stream)                                           \
    {                                                                                                            \
        MSDA_BOTH_MASKS_REQUIRED("msda_fwd_fused_levelref_qmasked")                                              \
        MSDA_TAKE_FWD_FUSED c.P = P; c.value_mask = value_mask; c.query_mask = query_mask;                       \
        return msda::run_fwd_fused<T, TV, TS, msda::LevelRefMaskedParams>(c);                                    \
    }                                                                                                            \
    extern "C" int msda_bwd_fused_levelref_qmasked_##SUF(                                                        \
        const void *grad_out, const void *value, const uint8_t *value_mask, const uint8_t *query_mask,          \
        const int64_t *shapes, const void *proj, const void *ref, void *grad_value, void *grad_proj,             \
        void *grad_ref_partial, int64_t B, int64_t I, int64_t H, int64_t D, int64_t Q, int64_t L, int64_t P,     \
        int ref_dim, int padding_mode, int align_corners, int64_t max_level_cells, int64_t value_row_stride,     \
        void *workspace, int64_t workspace_bytes, void *stream)                                                  \
    {                                                                                                            \
        MSDA_BOTH_MASKS_REQUIRED("msda_bwd_fused_levelref_qmasked")                                              \
        MSDA_TAKE_BWD_FUSED c.P = P; c.value_mask = value_mask; c.query_mask = query_mask;                       \
        return msda::run_bwd_fused<T, TV, TS, msda::LevelRefMaskedParams>(c);                                    \
    }

// the module's own fused pairs with both padding masks: msda_{fwd,bwd}_fused_masked_<suffix> (one reference point per query,
// uniform point count: MaskedParams) and msda_{fwd,bwd}_fused_ragged_masked_<suffix> (per-level counts: RaggedMaskedParams) —
// the unmasked twins' argument lists with `value_mask`, `query_mask` behind `value`.  A null value_mask is an argument
// error, refused before any other argument is looked at; a null query_mask means "every query is real" (what the kernarg
// means by it: a call that only masks values keeps its prefetches and the LDS-level sample-gradient kernel).
#define MSDA_DEFINE_MODULE_MASK_ENTRY_POINTS(SUF, T, TV, TS)                                                     \
    extern "C" int msda_fwd_fused_masked_##SUF(const void *value, const uint8_t *value_mask,                    \
                                               const uint8_t *query_mask, const int64_t *shapes,                 \
                                               const void *proj, const void *ref, void *out, int64_t B,          \
                                               int64_t I, int64_t H, int64_t D, int64_t Q, int64_t L, int64_t P, \
                                               int ref_dim, int padding_mode, int align_corners,                 \
                                               int64_t value_row_stride, void *stream)                           \
    {                                                                                                            \
        MSDA_MASK_REQUIRED("msda_fwd_fused_masked")                                                              \
        MSDA_TAKE_FWD_FUSED c.P = P; c.value_mask = value_mask; c.query_mask = query_mask;                       \
        return msda::run_fwd_fused<T, TV, TS, msda::MaskedParams>(c);                                            \
    }                                                                                                            \
    extern "C" int msda_bwd_fused_masked_##SUF(                                                                  \
        const void *grad_out, const void *value, const uint8_t *value_mask, const uint8_t *query_mask,          \
        const int64_t *shapes, const void *proj, const void *ref, void *grad_value, void *grad_proj,             \
        void *grad_ref_partial, int64_t B, int64_t I, int64_t H, int64_t D, int64_t Q, int64_t L, int64_t P,     \
        int ref_dim, int padding_mode, int align_corners, int64_t max_level_cells, int64_t value_row_stride,     \
        void *workspace, int64_t workspace_bytes, void *stream)                                                  \
    {                                                                                                            \
        MSDA_MASK_REQUIRED("msda_bwd_fused_masked")                                                              \
        MSDA_TAKE_BWD_FUSED c.P = P; c.value_mask = value_mask; c.query_mask = query_mask;                       \
        return msda::run_bwd_fused<T, TV, TS, msda::MaskedParams>(c);                                            \
    }                                                                                                            \
    extern "C" int msda_fwd_fused_ragged_masked_##SUF(const void *value, const uint8_t *value_mask,             \
                                                      const uint8_t *query_mask, const int64_t *shapes,          \
                                                      const void *proj, const void *ref, void *out, int64_t B,   \
                                                      int64_t I, int64_t H, int64_t D, int64_t Q, int64_t L,     \
                                                      const int32_t *points_per_level, int ref_dim,              \
                                                      int padding_mode, int align_corners,                       \
                                                      int64_t value_row_stride, void *stream)                    \
    {                                                                                                            \
        MSDA_MASK_REQUIRED("msda_fwd_fused_ragged_masked")                                                       \
        MSDA_TAKE_FWD_FUSED MSDA_TAKE_COUNTS c.value_mask = value_mask; c.query_mask = query_mask;               \
        return msda::run_fwd_fused<T, TV, TS, msda::RaggedMaskedParams>(c);                                      \
    }                                                                                                            \
    extern "C" int msda_bwd_fused_ragged_masked_##SUF(                                                           \
        const void *grad_out, const void *value, const uint8_t *value_mask, const uint8_t *query_mask,          \
        const int64_t *shapes, const void *proj, const void *ref, void *grad_value, void *grad_proj,             \
        void *grad_ref_partial, int64_t B, int64_t I, int64_t H, int64_t D, int64_t Q, int64_t L,                \
        const int32_t *points_per_level, int ref_dim, int padding_mode, int align_corners,                       \
        int64_t max_level_cells, int64_t value_row_stride, void *workspace, int64_t workspace_bytes,             \
        void *stream)                                                                                            \
    {                                                                                                            \
        MSDA_MASK_REQUIRED("msda_bwd_fused_ragged_masked")                                                       \
        MSDA_TAKE_BWD_FUSED MSDA_TAKE_COUNTS c.value_mask = value_mask; c.query_mask = query_mask;               \
        return msda::run_bwd_fused<T, TV, TS, msda::RaggedMaskedParams>(c);                                      \
    }

// one storage type for every tensor
#define MSDA_DEFINE_ENTRY_POINTS(SUF, T) MSDA_DEFINE_ENTRY_POINTS2(SUF, T, T)
