// msda_prologue.hpp — what the fused prologues of the two bilinear gather kernels (msda_kernels.hpp) differ in, each
// stated once: the sampling-point RULES, a sample's level, the projection's memory layout, the per-unit softmax statistics.
// Included by msda_kernels.hpp behind the kernarg types (not a header of its own: it reads Params and its relatives).
//
// A rule turns a sample's projected offsets (ox, oy) and its reference point `r` into the sampling point:
//
//   rule               kernarg type, ref_dim                forward's point                              the backward parks
//   MODULE2D           Params & masked relatives, 2         r + o / (h_l, w_l)   (stored (h, w) order)   o
//   MODULEBOX          Params, MaskedParams, 4              r + o * size / (2 P)                         o
//   MODULEBOXRAGGED    RaggedParams, RaggedMaskedParams, 4  r + o * size / (2 P_l)                       o * (1 / (2 P_l))
//   LEVELREF2D         LevelRef*Params, 2                   r_l + o / (w_l, h_l)                         o / (w_l, h_l)
//   LEVELREFBOX        LevelRef*Params, 4                   levelref_box_point(r_l, o / P, size)         o / P
//   HFBOX              HfBoxParams                          hfbox_point(r, o * s_l, size, offset_scale)  o * s_l
//
// and every rule states, next to each other, the five things the kernels need of it (see "the rules" below).  The
// contract the kernels' comments used to carry from place to place — "the same operations", "as the fused forward forms
// it" — is now visible in one screenful per rule: _REFORM on what _BACKWARD parked names the bilinear cell _BACKWARD's
// point sampled, and the operations and their order are PyTorch's / transformers' wherever a rule says so.
// A new prologue adds one rule — its macros, a line in MSDA_RULE_LADDER and, if it has a box, one in
// MSDA_RULE_STORE_SIZE_GRADS — and one kernarg type; the kernels do not change.
// The price of the macro form (names taken from the enclosing scope, no types at the seams) is accepted for one reason:
// it is the only form found that leaves every kernel's machine code as it was.
#pragma once

namespace msda {

// Elements of `ref` per query, and the reference point of (query fq, level l) behind the batch element's base.
__device__ __forceinline__ int ref_row_elems(const Params &p) { return p.ref_dim; }
__device__ __forceinline__ int ref_row_elems(const LevelRefParams &p) { return p.L * p.ref_dim; }
__device__ __forceinline__ int ref_row_elems(const LevelRefMaskedParams &p) { return p.L * p.ref_dim; }
template <typename T> __device__ __forceinline__ const T *ref_of(const Params &p, const T *refp, int fq, int)
{
    return refp + (size_t)fq * p.ref_dim;
}
template <typename T> __device__ __forceinline__ const T *ref_of(const LevelRefParams &p, const T *refp, int fq, int l)
{
    return refp + ((size_t)fq * p.L + l) * p.ref_dim;
}
template <typename T> __device__ __forceinline__ const T *ref_of(const LevelRefMaskedParams &p, const T *refp, int fq, int l)
{
    return refp + ((size_t)fq * p.L + l) * p.ref_dim;
}
// The 4-d point from the offset already divided by P: two rounded multiplies, then a rounded add — transformers'
// `ref + offsets / P * size * 0.5`, operation by operation.  The translation units are built with -ffp-contract=fast;
// the product passes through an empty asm statement (as discrete_pixel's) so that the add cannot take it as an FMA
// operand: the point is bit for bit the host's, and grad_value's parked copy of it (the backward's phase 3 calls this
// again on the same operands) names the cell the forward sampled.
template <typename A> __device__ __forceinline__ A levelref_box_point(A r, A q, A size)
{
    A t = q * size;
    t = t * (A)0.5;
    asm("" : "+v"(t));
    return r + t;
}

// s_l of the sample's level, converted to the arithmetic type: a select per level on scalars at constant kernarg offsets
// (as lvl_of's scan; the level itself comes from that scan, the host bounds L by kFusedRaggedMaxLevels).
template <typename A, typename PP> __device__ __forceinline__ A hfbox_scale(const PP &p, int l)
{
    if constexpr (kHfBox<PP>) {
        float s = p.lscale[0];
#pragma unroll
        for (int k = 1; k < kFusedRaggedMaxLevels; ++k) {
            if (k >= p.L) break;
            s = l >= k ? p.lscale[k] : s;
        }
        return (A)s;
    } else {
        return (A)0;
    }
}
// The point from q = o * s_l (the backward parks q: phase 3 calls this again on the same operands, so the copy written
// for grad_value names the cell the forward sampled).  The translation units are built with -ffp-contract=fast; the last
// product passes through an empty asm statement (as levelref_box_point's) so that the add cannot take it as an FMA operand.
template <typename A> __device__ __forceinline__ A hfbox_point(A r, A q, A size, A off_scale)
{
    A t = q * size;
    t = t * off_scale;
    asm("" : "+v"(t));
    return r + t;
}

// ---- the rules ----
// Shared as TEXT, not as functions: a force-inlined helper is simplified on its own before it is inlined, which moved
// the reference point's loads and the final add of the module rules across the ref_dim branch and changed the machine
// code of every fused kernel (build findings); the same tokens pasted into the kernel compile to the code
// the kernels had.  Every macro reads the enclosing kernel's `p`, `tab`, `A`, `TR` (and the backward's `half_inv_P`,
// declared by MSDA_RULE_BACKWARD_SETUP) and takes the sample's operands by name: `r` the reference point (ref_of), `l`
// the level, `npts` the level's point count, `ox` / `oy` the offsets, `x` / `y` (`kx` / `ky`) the results.
//   _FORWARD    msda_fwd_kernel, phase 0: the point
//   _BACKWARD   msda_bwd_sample_kernel, phase 0: the point, and (ox, oy) REPLACED by what the rule parks of them
//   _REFORM     ... phase 3: the point written out for the grad_value passes, from the parked (ox, oy) alone, each
//               coordinate through `cvt` (the parked type's from_acc; MSDA_ID where _BACKWARD reuses the text)
//   _SLOPE      ... phase 3: d point / d offset
//   _SIZE_GRAD  ... phase 2b: the box-size partial from g = sum(grad_point * parked offset) — box rules only; stored
//               by MSDA_RULE_STORE_SIZE_GRADS, the ladder over them
#define MSDA_ID(v) v
#define MSDA_RULE_BACKWARD_SETUP const A half_inv_P = (A)1 / (A)(2 * p.P) /* 1 / (2 P), rounded once */

// the reference module, 2-d reference points (frontend.py:275).  NB: the (x, y) offsets are divided by img_shapes in its
// STORED (h, w) order — x by the height, y by the width.  The raw offset is parked.
#define MSDA_MODULE2D_FORWARD(r, l, npts, ox, oy, x, y) \
    x = TR::to_acc(r[0]) + ox / (A)tab->h[l];            \
    y = TR::to_acc(r[1]) + oy / (A)tab->w[l];
#define MSDA_MODULE2D_BACKWARD(r, l, npts, ox, oy, x, y) MSDA_MODULE2D_FORWARD(r, l, npts, ox, oy, x, y)
#define MSDA_MODULE2D_REFORM(cvt, r, l, ox, oy, x, y) \
    x = cvt(TR::to_acc(r[0]) + ox / (A)tab->h[l]);       \
    y = cvt(TR::to_acc(r[1]) + oy / (A)tab->w[l]);
#define MSDA_MODULE2D_SLOPE(r, l, npts, kx, ky) \
    kx = (A)1 / (A)tab->h[l];                    \
    ky = (A)1 / (A)tab->w[l];

// the reference module, boxes, one point count P.  The forward DIVIDES by 2 P — multiply, divide, add, each rounded once:
// PyTorch's bits for the same expression — while the backward MULTIPLIES by half_inv_P = 1 / (2 P) in all of its places
// (phase 0's point, the parked point, the slope, the box-size partial).  For P a power of two the two agree bit for bit;
// for any other P the backward's point can differ from the forward's in the last place.  Kept as it is.
// The raw offset is parked.
#define MSDA_MODULEBOX_FORWARD(r, l, npts, ox, oy, x, y)            \
    x = TR::to_acc(r[0]) + ox * TR::to_acc(r[2]) / (A)(2 * p.P);    \
    y = TR::to_acc(r[1]) + oy * TR::to_acc(r[3]) / (A)(2 * p.P);
#define MSDA_MODULEBOX_BACKWARD(r, l, npts, ox, oy, x, y) MSDA_MODULEBOX_REFORM(MSDA_ID, r, l, ox, oy, x, y)
#define MSDA_MODULEBOX_REFORM(cvt, r, l, ox, oy, x, y)                   \
    x = cvt(TR::to_acc(r[0]) + ox * TR::to_acc(r[2]) * half_inv_P);      \
    y = cvt(TR::to_acc(r[1]) + oy * TR::to_acc(r[3]) * half_inv_P);
#define MSDA_MODULEBOX_SLOPE(r, l, npts, kx, ky) \
    kx = TR::to_acc(r[2]) * half_inv_P;           \
    ky = TR::to_acc(r[3]) * half_inv_P;
#define MSDA_MODULEBOX_SIZE_GRAD(g) ((g) * half_inv_P)

// the reference module, boxes, per-level point counts: npts = the count of the sample's OWN level.  The forward's point
// is multiply, divide, add — each rounded once, nothing for the compiler to fuse: bit for bit what the same expression
// gives in PyTorch, so a sample within an ulp of a pixel boundary lands on the same side of it as in the unfused
// composition.  The backward's phase 0 forms the point the same way (the location gradient sees the same bilinear cell)
// and parks the offset SCALED by 1 / (2 P_l): the box-size partial and the parked point need no level look-up of their
// own — at the price that _REFORM multiplies where _FORWARD divides (as the uniform rule's backward, with its caveat).
#define MSDA_MODULEBOXRAGGED_FORWARD(r, l, npts, ox, oy, x, y)      \
    x = TR::to_acc(r[0]) + ox * TR::to_acc(r[2]) / (A)(2 * npts);   \
    y = TR::to_acc(r[1]) + oy * TR::to_acc(r[3]) / (A)(2 * npts);
#define MSDA_MODULEBOXRAGGED_BACKWARD(r, l, npts, ox, oy, x, y) \
    MSDA_MODULEBOXRAGGED_FORWARD(r, l, npts, ox, oy, x, y)      \
    const A hinv = (A)1 / (A)(2 * npts);                        \
    ox *= hinv;                                                 \
    oy *= hinv;
#define MSDA_MODULEBOXRAGGED_REFORM(cvt, r, l, ox, oy, x, y) \
    x = cvt(TR::to_acc(r[0]) + ox * TR::to_acc(r[2]));        \
    y = cvt(TR::to_acc(r[1]) + oy * TR::to_acc(r[3]));
#define MSDA_MODULEBOXRAGGED_SLOPE(r, l, npts, kx, ky) \
    const A hinv = (A)1 / (A)(2 * npts);                \
    kx = TR::to_acc(r[2]) * hinv;                       \
    ky = TR::to_acc(r[3]) * hinv;
#define MSDA_MODULEBOXRAGGED_SIZE_GRAD(g) (g) /* (the parked offsets carry the 1 / (2 P_l)) */

// transformers' rule on the level's own 2-d reference point: x by the width, y by the height.  The QUOTIENT is parked,
// so the parked point is the forward's expression on the forward's operands.
#define MSDA_LEVELREF2D_FORWARD(r, l, npts, ox, oy, x, y) \
    x = TR::to_acc(r[0]) + ox / (A)tab->w[l];              \
    y = TR::to_acc(r[1]) + oy / (A)tab->h[l];
#define MSDA_LEVELREF2D_BACKWARD(r, l, npts, ox, oy, x, y) \
    ox = ox / (A)tab->w[l];                                 \
    oy = oy / (A)tab->h[l];                                 \
    MSDA_LEVELREF2D_REFORM(MSDA_ID, r, l, ox, oy, x, y)
#define MSDA_LEVELREF2D_REFORM(cvt, r, l, ox, oy, x, y) \
    x = cvt(TR::to_acc(r[0]) + ox);                      \
    y = cvt(TR::to_acc(r[1]) + oy);
#define MSDA_LEVELREF2D_SLOPE(r, l, npts, kx, ky) \
    kx = (A)1 / (A)tab->w[l];                      \
    ky = (A)1 / (A)tab->h[l];

// ... and on the level's own box: `ref + offsets / P * size * 0.5`, the division FIRST (levelref_box_point); o / P is
// parked.  The slope is size * half_inv_P (one rounding of 1 / (2 P), not the point's two multiplies: a gradient, not a
// cell choice); d point / d size = offset / P * 0.5, and the parked offsets carry the 1 / P.
#define MSDA_LEVELREFBOX_FORWARD(r, l, npts, ox, oy, x, y)                                  \
    x = levelref_box_point<A>(TR::to_acc(r[0]), ox / (A)p.P, TR::to_acc(r[2]));             \
    y = levelref_box_point<A>(TR::to_acc(r[1]), oy / (A)p.P, TR::to_acc(r[3]));
#define MSDA_LEVELREFBOX_BACKWARD(r, l, npts, ox, oy, x, y) \
    ox = ox / (A)p.P;                                       \
    oy = oy / (A)p.P;                                       \
    MSDA_LEVELREFBOX_REFORM(MSDA_ID, r, l, ox, oy, x, y)
#define MSDA_LEVELREFBOX_REFORM(cvt, r, l, ox, oy, x, y)                             \
    x = cvt(levelref_box_point<A>(TR::to_acc(r[0]), ox, TR::to_acc(r[2])));          \
    y = cvt(levelref_box_point<A>(TR::to_acc(r[1]), oy, TR::to_acc(r[3])));
#define MSDA_LEVELREFBOX_SLOPE(r, l, npts, kx, ky) \
    kx = TR::to_acc(r[2]) * half_inv_P;             \
    ky = TR::to_acc(r[3]) * half_inv_P;
#define MSDA_LEVELREFBOX_SIZE_GRAD(g) ((g) * (A)0.5)

// transformers' box rule with per-level point counts (D-FINE, DEIMv2, RT-DETRv2): s_l of the sample's level (the
// host's float32(1 / P_l), hfbox_scale) times the offset is parked; the point is hfbox_point of it, and the box-size
// partial the location gradient times it times offset_scale.
#define MSDA_HFBOX_FORWARD(r, l, npts, ox, oy, x, y)                                \
    const A s = hfbox_scale<A>(p, l), os = (A)p.off_scale;                          \
    x = hfbox_point<A>(TR::to_acc(r[0]), ox * s, TR::to_acc(r[2]), os);             \
    y = hfbox_point<A>(TR::to_acc(r[1]), oy * s, TR::to_acc(r[3]), os);
#define MSDA_HFBOX_BACKWARD(r, l, npts, ox, oy, x, y)                               \
    const A s = hfbox_scale<A>(p, l), os = (A)p.off_scale;                          \
    ox = ox * s;                                                                    \
    oy = oy * s;                                                                    \
    x = hfbox_point<A>(TR::to_acc(r[0]), ox, TR::to_acc(r[2]), os);                 \
    y = hfbox_point<A>(TR::to_acc(r[1]), oy, TR::to_acc(r[3]), os);
#define MSDA_HFBOX_REFORM(cvt, r, l, ox, oy, x, y)                                       \
    x = cvt(hfbox_point<A>(TR::to_acc(r[0]), ox, TR::to_acc(r[2]), (A)p.off_scale));     \
    y = cvt(hfbox_point<A>(TR::to_acc(r[1]), oy, TR::to_acc(r[3]), (A)p.off_scale));
#define MSDA_HFBOX_SLOPE(r, l, npts, kx, ky)                    \
    const A s = hfbox_scale<A>(p, l), os = (A)p.off_scale;      \
    kx = s * TR::to_acc(r[2]) * os;                             \
    ky = s * TR::to_acc(r[3]) * os;
#define MSDA_HFBOX_SIZE_GRAD(g) ((g) * (A)p.off_scale)

// The ONE ladder over the kernarg types and Params::ref_dim: which rule a kernel applies.  A new prologue adds its five
// macros above and its line here.
#define MSDA_RULE_LADDER(FACET, ...)                         \
    if constexpr (kHfBox<PP>) {                              \
        MSDA_HFBOX_##FACET(__VA_ARGS__)                      \
    } else if constexpr (kLevelRef<PP>) {                    \
        if (p.ref_dim == 2) {                                \
            MSDA_LEVELREF2D_##FACET(__VA_ARGS__)             \
        } else {                                             \
            MSDA_LEVELREFBOX_##FACET(__VA_ARGS__)            \
        }                                                    \
    } else if (p.ref_dim == 2) {                             \
        MSDA_MODULE2D_##FACET(__VA_ARGS__)                   \
    } else if constexpr (kRagged<PP>) {                      \
        MSDA_MODULEBOXRAGGED_##FACET(__VA_ARGS__)            \
    } else {                                                 \
        MSDA_MODULEBOX_##FACET(__VA_ARGS__)                  \
    }
#define MSDA_RULE_FORWARD(r, l, npts, ox, oy, x, y) MSDA_RULE_LADDER(FORWARD, r, l, npts, ox, oy, x, y)
#define MSDA_RULE_BACKWARD(r, l, npts, ox, oy, x, y) MSDA_RULE_LADDER(BACKWARD, r, l, npts, ox, oy, x, y)
#define MSDA_RULE_REFORM(cvt, r, l, ox, oy, x, y) MSDA_RULE_LADDER(REFORM, cvt, r, l, ox, oy, x, y)
#define MSDA_RULE_SLOPE(r, l, npts, kx, ky) MSDA_RULE_LADDER(SLOPE, r, l, npts, kx, ky)
// phase 2b: the pair of box-size partials stored behind the point's.  Only the box rules have one, so this facet has
// a ladder of its own over them (a new box rule adds its line here too)
#define MSDA_STORE_SIZE(RULE, dst, gw, gh)                   \
    dst[2] = TR::from_acc(MSDA_##RULE##_SIZE_GRAD(gw));      \
    dst[3] = TR::from_acc(MSDA_##RULE##_SIZE_GRAD(gh));
#define MSDA_RULE_STORE_SIZE_GRADS(dst, gw, gh)              \
    if constexpr (kHfBox<PP>) {                              \
        MSDA_STORE_SIZE(HFBOX, dst, gw, gh)                  \
    } else if (p.ref_dim == 4) {                             \
        if constexpr (kLevelRef<PP>) {                       \
            MSDA_STORE_SIZE(LEVELREFBOX, dst, gw, gh)        \
        } else if constexpr (kRagged<PP>) {                  \
            MSDA_STORE_SIZE(MODULEBOXRAGGED, dst, gw, gh)    \
        } else {                                             \
            MSDA_STORE_SIZE(MODULEBOX, dst, gw, gh)          \
        }                                                    \
    }

// ---- the level `l` of sample `sl` and its level's point count `npts` (declares both; reads the kernel's `inv_P`) ----
#define MSDA_SAMPLE_LEVEL(sl, l, npts)                       \
    [[maybe_unused]] int npts = p.P;                         \
    int l;                                                   \
    if constexpr (kRagged<PP>) l = lvl_of(p, sl, npts);      \
    else l = div_small(sl, p.P, inv_P);

// ---- the projection's layout: (x offset, y offset, logit) of a sample, and their three gradients.  Text, as the rules
// (as a struct it renumbered the backward's accumulators: DESIGN.md 3).  Read the kernel's `p`, `TS`, `SR` ----
// Interleaved: `loc` holds the raw projection [B, Q, H, S, 3] and `grad_loc` its gradient.  Split (what two Linear
// layers produce, kSplitProj): `loc` holds the offsets [B, Q, H, S, 2] and `grad_loc` their gradient; the logits
// [B, Q, H, S] and their gradient ride behind Params.  `s0` = the plane's first sample, `sidx` = the sample behind it.
#define MSDA_PROJ_DECLARE(s0)                                                              \
    [[maybe_unused]] const TS *proj3 = static_cast<const TS *>(p.loc) + 3 * s0;            \
    [[maybe_unused]] const TS *off2 = nullptr, *lgt1 = nullptr;                            \
    if constexpr (kSplitProj<PP>) {                                                        \
        off2 = static_cast<const TS *>(p.loc) + 2 * s0;                                    \
        lgt1 = static_cast<const TS *>(p.logits) + s0;                                     \
    }
#define MSDA_PROJ_REBASE(s0)                                 \
    proj3 = static_cast<const TS *>(p.loc) + 3 * s0;         \
    if constexpr (kSplitProj<PP>) {                          \
        off2 = static_cast<const TS *>(p.loc) + 2 * s0;      \
        lgt1 = static_cast<const TS *>(p.logits) + s0;       \
    }
#define MSDA_PROJ_LOAD(sidx, ox, oy, lg)                                                   \
    if constexpr (kSplitProj<PP>) {                                                        \
        ox = SR::to_acc(off2[2 * sidx]), oy = SR::to_acc(off2[2 * sidx + 1]);              \
        lg = SR::to_acc(lgt1[sidx]);                                                       \
    } else {                                                                               \
        ox = SR::to_acc(proj3[3 * sidx]), oy = SR::to_acc(proj3[3 * sidx + 1]);            \
        lg = SR::to_acc(proj3[3 * sidx + 2]);                                              \
    }
#define MSDA_PROJ_STORE(s, on, gx, gy, gl)                                 \
    if constexpr (kSplitProj<PP>) {                                        \
        TS *go_ = static_cast<TS *>(p.grad_loc) + 2 * (s);                 \
        TS *gg_ = static_cast<TS *>(p.grad_logits) + (s);                  \
        if (on) {                                                          \
            store_stream(go_, gx);                                         \
            store_stream(go_ + 1, gy);                                     \
            store_stream(gg_, gl);                                         \
        }                                                                  \
    } else {                                                               \
        TS *gp_ = static_cast<TS *>(p.grad_loc) + 3 * (s);                 \
        if (on) {                                                          \
            store_stream(gp_, gx);                                         \
            store_stream(gp_ + 1, gy);                                     \
            store_stream(gp_ + 2, gl);                                     \
        }                                                                  \
    }

// ---- per-unit softmax statistics over the logits phase 0 parked (field 0 of the records w_rec[u .. u + sc)): the unit's
// G lanes (this one is lane j of it) leave max and 1 / sum(exp) in the unit's padding slot w_rec[u + sc].  Text, as the
// rules: as a function its two loops were rotated on their own and every fused kernel changed ----
#define MSDA_UNIT_SOFTMAX_STATS(w_rec, u, sc, j)                                          \
    {                                                                                     \
        A mx = -__builtin_huge_val();                                                     \
        for (int sl = j; sl < sc; sl += G) mx = fmax_t(mx, w_rec[u + sl].v[0]);           \
        mx = group_max<G>(mx);                                                            \
        A sum = (A)0;                                                                     \
        for (int sl = j; sl < sc; sl += G) sum += exp_t(w_rec[u + sl].v[0] - mx);         \
        sum = group_sum<G>(sum);                                                          \
        if (j == 0) {                                                                     \
            w_rec[u + sc].v[0] = mx;                                                      \
            w_rec[u + sc].v[1] = (A)1 / sum;                                              \
        }                                                                                 \
    }

}  // namespace msda
