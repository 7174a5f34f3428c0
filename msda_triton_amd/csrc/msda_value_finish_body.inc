// msda_value_finish_body.inc — the body of msda_value_finish_kernel (msda_value_sorted.hpp), included once per kernel:
// MSDA_FINISH_MASKED 0 is the kernel as it always was, 1 its value-mask twin (kernarg MaskedParams).  Textual inclusion, not
// a shared function: the unmasked kernel's code must stay what it was, instruction for instruction.
    using A = typename Traits<T>::acc;
    using TR = Traits<TV>;
    constexpr int NU = kBlock / G;
    constexpr int NUG = GB / G;  // windows per gather workgroup
    constexpr int ROUNDS = (kFinishPixels + NU - 1) / NU;  // pixel rows per lane group
    constexpr int RB = ROUNDS < 4 ? ROUNDS : 4;            // ... whose slot loads are in flight together
    const int slots = (p.I + kFinishPixels - 1) / kFinishPixels;
    int pair, slot;
    if (!decode_block(p.grid3d, p.B * p.H, slots, p.xcd_map, pair, slot)) return;
    __shared__ LevelTab tab;
    __shared__ int s_rng[kFinishPixels][6];     // list starts t0 t1 t2 (cell row y-1), u0 u1 u2 (cell row y)
    __shared__ uint32_t s_flags[kFinishPixels];  // bits 0-3: slot k was written; bit 4: continuation rows to add
    load_level_table(&tab, p.shapes, p.L);
    __syncthreads();
    const int b = (int)fast_div((uint32_t)pair, p.div_h), h = pair - b * p.H;
    const int tid = threadIdx.x;
    const int pix_base = slot * kFinishPixels;
    const FastDiv dw = p.div_win;  // record index -> gather window (the window size is chosen per call)
    auto window = [dw](int r) { return fast_div((uint32_t)r, dw); };
    auto carried = [&](int a0, int a1, int a2) { return a1 > a0 && a2 > a1 && window(a0) == window(a1); };
    // continuation row sets: gather-workgroup boundaries strictly inside a cell's window range
    auto nconts = [&](int beg, int end) {
        return end > beg ? (int)(window(end - 1) / (uint32_t)NUG) - (int)(window(beg) / (uint32_t)NUG) : 0;
    };
    // ---- phase 1: record ranges of the cells (x-1,y-1), (x,y-1) | (x-1,y), (x,y) of the thread's pixel: consecutive
    // cell ids, consecutive ranges.  A pixel the shapes tensor does not describe (sum h*w != I), or one whose cells
    // were dropped for lack of workspace, has no cells: all ranges empty, the row is stored as zeros. ----
    if (tid < kFinishPixels) {
        const int pix = pix_base + tid;
        struct Three {
            int v[3];
        };
        Three ta{{0, 0, 0}}, ua{{0, 0, 0}};
#if MSDA_FINISH_MASKED  // a padding pixel (mask byte 0) has no cells either: its row is stored as zeros, its slots never loaded
        if (pix < p.I && p.vmask[(size_t)b * p.I + pix] != 0) {
#else
        if (pix < p.I) {
#endif
            const int *off = p.ws_off + (size_t)pair * (p.nc_cap + 1);
            const int ncells = min(plane_cells(tab, p.L), p.nc_cap);
            int l = 0;
            while (l < p.L - 1 && pix >= tab.start[l + 1]) ++l;
            const int rel = pix - tab.start[l], w = tab.w[l], cw = w + 1;
            const int y = rel / max(w, 1), x = rel - y * w;
            const int c11 = tab.cstart[l] + y * cw + x;  // cell (x-1, y-1)
            if (w > 0 && y < tab.h[l] && c11 + cw + 2 <= ncells) {
                __builtin_memcpy(&ta, off + c11, sizeof(Three));  // three consecutive list starts: one 12-byte load
                __builtin_memcpy(&ua, off + c11 + cw, sizeof(Three));
            }
        }
        const int t0 = ta.v[0], t1 = ta.v[1], t2 = ta.v[2], u0 = ua.v[0], u1 = ua.v[1], u2 = ua.v[2];
        uint32_t flags = (u2 > u1 ? 1u : 0u) | ((u1 > u0 && !carried(u0, u1, u2)) ? 2u : 0u) | (t2 > t1 ? 4u : 0u) |
                         ((t1 > t0 && !carried(t0, t1, t2)) ? 8u : 0u);
        if (nconts(u1, u2) + nconts(u0, u1) + nconts(t1, t2) + nconts(t0, t1) != 0) flags |= 16u;
        s_flags[tid] = flags;
        s_rng[tid][0] = t0, s_rng[tid][1] = t1, s_rng[tid][2] = t2;
        s_rng[tid][3] = u0, s_rng[tid][4] = u1, s_rng[tid][5] = u2;
    }
    __syncthreads();
    // ---- phase 2 ----
    const int unit = tid / G, j = tid % G;
    const A *cont = static_cast<const A *>(p.ws_cont) + (size_t)pair * p.cont_cap * 4 * p.D;
    const size_t plane_slots = (size_t)p.I * 4 * p.D * sizeof(A);  // < 2^31 (host check)
    const rsrc_t rs_sc = make_rsrc(static_cast<const unsigned char *>(p.ws_scratch) + (size_t)pair * plane_slots, (uint32_t)plane_slots);
    const int nchan_chunks = (p.D + G * VEC - 1) / (G * VEC);
    for (int cc = 0; cc < nchan_chunks; ++cc) {
        const int c0 = (cc * G + j) * VEC;
        if (c0 >= p.D) continue;
        for (int r0 = 0; r0 < ROUNDS; r0 += RB) {
            if (pix_base + r0 * NU >= p.I) break;  // block-uniform: nothing left
            // the rows' four slots each: independent range-checked loads through a buffer descriptor; a slot nobody
            // wrote gets an out-of-range offset and reads 0 without touching memory, and an instruction whose lanes
            // are all masked is not issued at all (it would still occupy the vector-memory path)
            uint32_t flags[RB];
            Pack<A, VEC> rr[RB][4];
#pragma unroll
            for (int t = 0; t < RB; ++t) {
                const int pt = (r0 + t) * NU + unit, pix = pix_base + pt;
                const bool live = pt < kFinishPixels && pix < p.I;  // (64 lane groups of 4 lanes, 32 pixels: half the groups idle)
                flags[t] = live ? s_flags[pt] | 32u : 0u;  // bit 5: the row exists
                const uint32_t base = ((uint32_t)(live ? pix : 0) * 4u * (uint32_t)p.D + (uint32_t)c0) * (uint32_t)sizeof(A);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
#pragma unroll
                    for (int v = 0; v < VEC; ++v) rr[t][k].v[v] = (A)0;
                    const bool on = ((flags[t] >> k) & 1u) != 0;
                    if (__builtin_amdgcn_ballot_w64(on) != 0)
                        rr[t][k] = load_acc_pack<A, VEC>(rs_sc, on ? base + (uint32_t)k * (uint32_t)p.D * (uint32_t)sizeof(A) : 0x80000000u);
                }
            }
#pragma unroll
            for (int t = 0; t < RB; ++t) {
                if (!(flags[t] & 32u)) continue;
                const int pt = (r0 + t) * NU + unit, pix = pix_base + pt;
                A acc[VEC];
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc[v] = ((rr[t][0].v[v] + rr[t][1].v[v]) + rr[t][2].v[v]) + rr[t][3].v[v];
                if (flags[t] & 16u) {
                    auto add = [&](int beg, int end, int corner) {
                        if (end <= beg) return;
                        const int g1 = (int)(window(end - 1) / (uint32_t)NUG);
                        for (int g = (int)(window(beg) / (uint32_t)NUG) + 1; g <= g1; ++g) {
                            const Pack<A, VEC> cr =
                                *reinterpret_cast<const Pack<A, VEC> *>(cont + ((size_t)g * 4 + corner) * p.D + c0);
#pragma unroll
                            for (int v = 0; v < VEC; ++v) acc[v] += cr.v[v];
                        }
                    };
                    const int t0 = s_rng[pt][0], t1 = s_rng[pt][1], t2 = s_rng[pt][2];
                    const int u0 = s_rng[pt][3], u1 = s_rng[pt][4], u2 = s_rng[pt][5];
                    add(u1, u2, 0);
                    add(u0, u1, 1);
                    add(t1, t2, 2);
                    add(t0, t1, 3);
                }
                // several rounds over the queries: running sums in the accumulate type between them
                if (p.finish_mode != 0) {
                    A *run = static_cast<A *>(p.ws_accum) + ((size_t)pair * p.I + pix) * p.D + c0;
                    if (p.finish_mode != 1) {
                        const Pack<A, VEC> prev = *reinterpret_cast<const Pack<A, VEC> *>(run);
#pragma unroll
                        for (int v = 0; v < VEC; ++v) acc[v] += prev.v[v];
                    }
                    if (p.finish_mode != 3) {
                        Pack<A, VEC> keep;
#pragma unroll
                        for (int v = 0; v < VEC; ++v) keep.v[v] = acc[v];
                        *reinterpret_cast<Pack<A, VEC> *>(run) = keep;
                        continue;
                    }
                }
                Pack<TV, VEC> o;
#pragma unroll
                for (int v = 0; v < VEC; ++v) o.v[v] = TR::from_acc(acc[v]);
                TV *dst = static_cast<TV *>(p.grad_value) + (((size_t)b * p.I + pix) * p.H + h) * p.D + c0;
                store_stream(dst, o);
            }
        }
    }
