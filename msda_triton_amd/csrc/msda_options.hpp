// msda_options.hpp — the process-wide options of msda_set_option / msda_get_option (include/msda_hip.h), each described
// ONCE: X(key, default, lowest, highest accepted value, dev).  dev: an experiment knob, reachable only in builds with
// -DMSDA_DEV.  The launchers read an option through option_<key>(), declared here; msda_api.hip makes the atomics, the
// getters and the set / get table from the same list.  Host only.
#pragma once

#define MSDA_OPTION_LIST(X)                                                                                          \
    X(xcd_map, 1, 0, 2, false)                                                                                       \
    /* 0: auto (single-launch LDS kernel when a plane-level fits, else sorted gather), 2: sorted, 3: single-launch */ \
    /* (1 is refused) */                                                                                             \
    X(value_path, 0, 0, 3, false)                                                                                    \
    /* caller's promise: no level has more than this many bilinear cells (0: unknown) */                             \
    X(level_cells, 0, 0, 0x7fffffff, false)                                                                          \
    /* queries per round of the sorted grad_value path (0: automatic) */                                             \
    X(q_round, 0, 0, 0x7fffffff, false)                                                                              \
    /* workgroups per (plane, level) of the single-launch grad_value kernel (0: automatic) */                        \
    X(small_ns, 0, 0, 16, false)                                                                                     \
    /* 1: grad_loc/grad_attn and grad_value run concurrently on a forked side stream; 0: never; -1: automatic */     \
    X(overlap, -1, -1, 1, false)                                                                                     \
    /* 0: level-major place pass with LDS-staged runs (msda_value_place.hpp); 1: the plane-major place pass */       \
    X(place_path, 0, 0, 3, false)                                                                                    \
    /* 1: refuse a backward whose grad_value would not be bitwise reproducible */                                    \
    X(strict, 0, 0, 1, false)                                                                                        \
    /* 1: the sorted records may live in the caller's grad_loc / grad_attn buffers */                                \
    X(records_in_grads, 1, 0, 1, false)                                                                              \
    /* measurement only: an event pair around every kernel launch (msda_profile_read) */                             \
    X(profile, 0, 0, 1, false)                                                                                       \
    /* LDS-served levels — 0: never, 1: where lds_levels_plan says so, 2: wherever the kernels exist */              \
    X(lds_levels, 1, 0, 2, false)                                                                                    \
    /* 1: small problems take the one-wave-per-unit forward; 2: every problem it can; 0: never */                    \
    X(unit_fwd, 1, 0, 2, false)                                                                                      \
    /* ablation mask */                                                                                              \
    X(debug, 0, (int)0x80000000, 0x7fffffff, true)                                                                   \
    /* (0, or at least 8: 1..7 are refused) */                                                                       \
    X(gather_win, 0, 0, 4096, true)                                                                                  \
    X(cell_slices, 0, 0, 64, true)                                                                                   \
    /* gather workgroups to aim for when choosing query chunks per workgroup */                                      \
    X(wg_target, 1 << 30, 1, 0x7fffffff, true)                                                                       \
    /* cap on the bytes of LDS-resident levels (-1: none) */                                                         \
    X(lds_budget, -1, -1, 0x7fffffff, true)                                                                          \
    /* start-up stagger of an LDSL workgroup's waves, in units of 64 cycles per wave (measured 0 / 4 / 12 / 24 at */ \
    /* c2 @ 10k: 0 is fastest — the work counter desynchronises the waves by itself) */                              \
    X(lds_stagger, 0, 0, 4096, true)                                                                                 \
    /* workgroups per CU the LDS-served-level launches are cut into (1: one round) */                                \
    X(lds_over, 1, 1, 8, true)                                                                                       \
    /* 0: two planes per LDS-level workgroup where the plan says so; 1: never; 2: whenever H is even */              \
    X(lds_planes, 0, 0, 2, false)                                                                                    \
    /* workgroups per plane from which a launch takes the linear block order (plane_grid) */                         \
    X(linear_slots, 320, 1, 1 << 30, false)                                                                          \
    /* Params::touch — 0: never, 2: always, 1: touch_plan's rule */                                                  \
    X(touch, 1, 0, 2, false)                                                                                         \
    /* 1: one unit per wave of the one-wave-per-unit forward; 2: two wherever the variant exists */                  \
    X(unit_waves, 1, 1, 2, false)                                                                                    \
    /* passes over the batch a workspace query sizes for when its flags name none (MSDA_WS_PASSES) */                \
    X(ws_passes, 1, 1, 128, false)

namespace msda {
#define MSDA_OPTION_GETTER(key, def, lo, hi, dev) int option_##key();
MSDA_OPTION_LIST(MSDA_OPTION_GETTER)
#undef MSDA_OPTION_GETTER
}  // namespace msda
