// msda_torch_ext.cpp — optional thin PyTorch binding over the C ABI (include/msda_hip.h).
//
// The product boundary is the C ABI; Python reaches it through ctypes (msda_triton_amd/_lib.py).  For
// Grounding-DINO-sized calls (B*Q ~ 10^3) the kernels take ~60 us while Python's autograd glue, ctypes
// marshalling and the engine's hop into a Python backward take ~100 us per forward+backward.  This extension is
// the same glue in C++.  It contains no kernels and no numerics; the argument validation stays in Python
// (msda_triton_amd/functional.py, ragged.py, discrete.py) and the same tests cover both routes.
//
// Layout: every family of entry points (msda_fwd<family>_<dtype> / msda_bwd<family>_<dtype>) is one MSDA_FAMILY table
// line — the dtype rule is written once, in suffix_of — and one thin torch::autograd::Function class, which names its
// table, its workspace query and the arguments its entry points take between the problem's dimensions and
// value_row_stride.  The bodies are shared: node_forward for all eight, sampling_backward for the nodes over sampling
// points and weights (MSDAFunction, MSDARaggedFunction, MSDADiscreteFunction), fused_backward for the module cores with
// the prologue fused in (MSDAFused*Function; the box rule's discrete node has no reference-point partials and a backward
// of its own).  Behind them, the row-range launches of the row-sharded operator.
// Reference counterpart: _TritonMultiscaleDeformableAttentionFunction, src/msda_triton/frontend.py:108-142.
#include <torch/extension.h>
#include <torch/csrc/autograd/functions/basic_ops.h>

#include <c10/hip/HIPStream.h>

#include <algorithm>
#include <tuple>
#include <utility>
#include <vector>

#include "../../include/msda_hip.h"

namespace {

// The entry points' dtype suffixes, in the order MSDA_FAMILY lists them.  `t`: dtype of the value pyramid (and its
// gradient); `c`: dtype of every other tensor — the same, or float next to a 16-bit pyramid (the mixed-storage entry points)
enum Suffix { f32, f16, bf16, f64, f32_vbf16, f32_vf16, kSuffixes };

Suffix suffix_of(at::ScalarType t, at::ScalarType c)
{
    if (t != c) {
        TORCH_CHECK_VALUE(c == at::kFloat && (t == at::kBFloat16 || t == at::kHalf),
                          "unsupported dtype combination: value ", t, " with ", c);
        return t == at::kBFloat16 ? f32_vbf16 : f32_vf16;
    }
    switch (t) {
    case at::kFloat: return f32;
    case at::kHalf: return f16;
    case at::kBFloat16: return bf16;
    case at::kDouble: return f64;
    default: TORCH_CHECK_VALUE(false, "unsupported dtype ", t);
    }
}

// A family's forward / backward pair for every suffix, and the names check_rc reports them under
template <typename Fwd, typename Bwd> struct Family {
    struct Pair {
        Fwd fwd;
        Bwd bwd;
    };
    const char *fwd_name, *bwd_name;
    Pair pairs[kSuffixes];
    const Pair &of(at::ScalarType t, at::ScalarType c) const { return pairs[suffix_of(t, c)]; }
};

#define MSDA_PAIR(F, S) {msda_fwd##F##_##S, msda_bwd##F##_##S}
#define MSDA_FAMILY(NAME, F)                                                                                           \
    constexpr Family<decltype(&msda_fwd##F##_f32), decltype(&msda_bwd##F##_f32)> NAME = {                                \
        "msda_fwd" #F, "msda_bwd" #F,                                                                                    \
        {MSDA_PAIR(F, f32), MSDA_PAIR(F, f16), MSDA_PAIR(F, bf16), MSDA_PAIR(F, f64), MSDA_PAIR(F, f32_vbf16),           \
         MSDA_PAIR(F, f32_vf16)}};
MSDA_FAMILY(kPlain, )
MSDA_FAMILY(kRagged, _ragged)
MSDA_FAMILY(kDiscrete, _discrete)
MSDA_FAMILY(kFused, _fused)
MSDA_FAMILY(kFusedRagged, _fused_ragged)
MSDA_FAMILY(kFusedHfBox, _fused_hfbox)
MSDA_FAMILY(kFusedHfBoxDiscrete, _fused_hfbox_discrete)
MSDA_FAMILY(kFusedLevelRef, _fused_levelref)
#undef MSDA_FAMILY
#undef MSDA_PAIR

// (the row-range launches below)
using Fns = decltype(kPlain)::Pair;
Fns fns_for(at::ScalarType t, at::ScalarType c) { return kPlain.of(t, c); }

void check_rc(int rc, const char *what)
{
    if (rc == 0) return;
    TORCH_CHECK_VALUE(rc > 0, what, ": rejected arguments (", rc, "): ", msda_last_error());
    TORCH_CHECK(false, what, ": HIP error ", rc, ": ", msda_last_error());
}

// torch.autograd.function.once_differentiable (frontend.py:130 of the reference) for a C++ Function: when the
// backward itself runs under grad mode (create_graph=True) and was handed a differentiable gradient, the results
// are routed through a DelayedError node, so a second differentiation raises instead of silently treating them as
// constants.
torch::autograd::variable_list once_differentiable(const torch::autograd::variable_list &grads_in,
                                                   torch::autograd::variable_list outs)
{
    if (!at::GradMode::is_enabled()) return outs;
    bool any = false;
    for (const auto &g : grads_in) any = any || (g.defined() && g.requires_grad());
    if (!any) return outs;
    for (auto &o : outs)
        if (o.defined()) o = o.detach().requires_grad_(true);
    auto err = std::make_shared<torch::autograd::DelayedError>(
        "trying to differentiate twice a function that was marked with @once_differentiable", (int64_t)outs.size());
    return (*err)(std::move(outs));
}

void *current_stream(const at::Tensor &t) { return c10::hip::getCurrentHIPStream(t.device().index()).stream(); }

// The value pyramid as the kernels can address it, and its value_row_stride in bytes (0: dense).  A [B, I, H, D] view whose
// pixels sit a constant number of bytes apart with a pixel's H * D channels contiguous (functional.padded_value_rows) is read
// in place; any other layout is copied dense (functional._value_rows is the same rule).
std::pair<at::Tensor, int64_t> value_rows(const at::Tensor &img)
{
    if (img.is_contiguous()) return {img, 0};
    if (img.dim() == 4) {
        const int64_t B = img.size(0), I = img.size(1), H = img.size(2), D = img.size(3), es = (int64_t)img.element_size();
        const auto st = img.strides();
        if (D > 0 && H > 0 && I > 0 && st[3] == 1 && st[2] == D && st[1] >= H * D && (B == 1 || st[0] == I * st[1]) &&
            (st[1] * es) % 16 == 0 && I * st[1] * es < ((int64_t)1 << 31))
            return {img, st[1] * es};
    }
    return {img.contiguous(), 0};
}
// bytes from one batch element of `img` (as returned by value_rows) to the next
int64_t value_batch_bytes(const at::Tensor &img, int64_t vrow)
{
    return vrow > 0 ? img.size(1) * vrow : img.size(1) * img.size(2) * img.size(3) * (int64_t)img.element_size();
}

// ------------------------------------------------------------------------------------------------------------------
// The eight autograd nodes.  Each takes (img, shapes, a, b, ...): `a`, `b` are the sampling points and attention
// weights, or — the fused module cores — the raw projection and the reference points.
// ------------------------------------------------------------------------------------------------------------------
using torch::autograd::AutogradContext;
using torch::autograd::variable_list;

// What a node's `apply` takes behind the four tensors; a family leaves what its entry points do not take at the default.
// `counts`: the L per-level point counts, `level_scale`: the L fp32 scales of Hugging Face's box rule — host numbers, which
// the Python caller checked.
struct Extra {
    int64_t padding_mode = 0;
    bool align_corners = false;
    int64_t level_cells = 0;  // bound on the largest level's cells (0: unknown)
    std::vector<int64_t> counts;
    std::vector<double> level_scale;
    double offset_scale = 0;
};

// One call as the launches see it, forward and backward alike: the tensors the kernels read and the pieces of the entry
// points' argument lists.
struct Call {
    at::Tensor img, shapes, a, b;
    int64_t vrow;                 // value_row_stride of `img` (value_rows)
    int64_t B, I, H, D, Q, L, P;  // (P: without per-level counts only)
    int pad, ac;
    int64_t level_cells;
    std::vector<int32_t> ppl;
    std::vector<float> scale;  // (fp32 values: the conversion is exact)
    double offset_scale;

    Call(at::Tensor img_, int64_t vrow_, at::Tensor shapes_, at::Tensor a_, at::Tensor b_, const Extra &x)
        : img(std::move(img_)), shapes(std::move(shapes_)), a(std::move(a_)), b(std::move(b_)), vrow(vrow_), B(img.size(0)),
          I(img.size(1)), H(img.size(2)), D(img.size(3)), Q(a.size(1)),
          L(x.counts.empty() ? a.size(3) : (int64_t)x.counts.size()), P(x.counts.empty() ? a.size(4) : 0),
          pad((int)x.padding_mode), ac(x.align_corners ? 1 : 0), level_cells(x.level_cells),
          ppl(x.counts.begin(), x.counts.end()), scale(x.level_scale.begin(), x.level_scale.end()),
          offset_scale(x.offset_scale)
    {
    }
    auto inputs() const { return std::make_tuple(img.data_ptr(), shapes.data_ptr<int64_t>(), a.data_ptr(), b.data_ptr()); }
    auto dims() const { return std::make_tuple(B, I, H, D, Q); }
    // the samples of a query: L x P, or the per-level counts
    auto uniform() const { return std::make_tuple(L, P); }
    auto per_level() const { return std::make_tuple(L, ppl.data()); }
    // what follows them, in front of value_row_stride (forward) / max_level_cells (backward)
    auto mode() const { return std::make_tuple(pad, ac); }
    auto fused_mode() const { return std::make_tuple((int)b.size(-1), pad, ac); }  // (ref_dim first)
    auto hfbox_mode() const { return std::tuple_cat(std::make_tuple(scale.data(), offset_scale), fused_mode()); }
};

void save(AutogradContext *ctx, const Call &c, const Extra &x)
{
    ctx->save_for_backward({c.img, c.shapes, c.a, c.b});
    ctx->saved_data["padding_mode"] = x.padding_mode;
    ctx->saved_data["align_corners"] = x.align_corners;
    ctx->saved_data["level_cells"] = x.level_cells;
    ctx->saved_data["vrow"] = c.vrow;
    if (!x.counts.empty()) ctx->saved_data["counts"] = x.counts;
    if (!x.level_scale.empty()) {
        ctx->saved_data["level_scale"] = x.level_scale;
        ctx->saved_data["offset_scale"] = x.offset_scale;
    }
}

Call saved_call(AutogradContext *ctx)
{
    const auto saved = ctx->get_saved_variables();
    auto &data = ctx->saved_data;
    Extra x{data["padding_mode"].toInt(), data["align_corners"].toBool(), data["level_cells"].toInt()};
    if (data.count("counts")) x.counts = data["counts"].toIntVector();
    if (data.count("level_scale")) {
        x.level_scale = data["level_scale"].toDoubleVector();
        x.offset_scale = data["offset_scale"].toDouble();
    }
    return Call(saved[0], data["vrow"].toInt(), saved[1], saved[2], saved[3], x);
}

// The forward of every node.  value_rows(img_) is taken once: its tensor and stride are what the backward launches with.
template <typename Node>
at::Tensor node_forward(AutogradContext *ctx, const at::Tensor &img_, const at::Tensor &shapes_,
                        const at::Tensor &a_, const at::Tensor &b_, const Extra &x)
{
    const auto [img, vrow] = value_rows(img_);
    const Call c(img, vrow, shapes_.to(at::kLong).contiguous() /* stays on the device */, a_.contiguous(), b_.contiguous(), x);
    at::Tensor out = at::empty({c.B, c.Q, c.H, c.D}, c.a.options());
    const c10::DeviceGuard guard(img.device());
    check_rc(std::apply(Node::family.of(img.scalar_type(), c.a.scalar_type()).fwd,
                        std::tuple_cat(c.inputs(), std::make_tuple(out.data_ptr()), c.dims(), Node::samples(c), Node::mode(c),
                                       std::make_tuple(vrow, current_stream(img)))),
             Node::family.fwd_name);
    save(ctx, c, x);
    return out;
}

at::Tensor grad_out_as(const at::Tensor &grad, at::ScalarType dtype)
{
    at::Tensor gout = grad.contiguous();
    return gout.scalar_type() == dtype ? gout : gout.to(dtype);
}

bool aligned16(const at::Tensor &t) { return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0; }
void *ptr_or_null(const at::Tensor &t) { return t.defined() ? t.data_ptr() : nullptr; }

// grad_value (dense, whatever the pyramid's row stride) and the workspace its passes need (scratch: no initialisation
// needed).  `lend_grads`: the call asks for the sample gradients too and their buffers may hold the sorted records — the
// library's own conditions: 16-byte aligned buffers, no forced side-stream fork.
struct ValueGrad {
    at::Tensor g_img, ws;
    int64_t ws_bytes = 0;
};
template <typename Node> ValueGrad value_grad(const Call &c, bool lend_grads)
{
    ValueGrad v;
    v.g_img = at::empty(c.img.sizes(), c.img.options());
    const int flags = lend_grads && aligned16(v.g_img) && msda_get_option("overlap") != 1 ? MSDA_WS_RECORDS_IN_GRADS : 0;
    v.ws_bytes = std::apply(Node::workspace_bytes,
                            std::tuple_cat(c.dims(), Node::samples(c),
                                           std::make_tuple((int)c.a.element_size(), (int)c.img.element_size(), c.level_cells, flags)));
    v.ws = at::empty({v.ws_bytes}, c.img.options().dtype(at::kByte));
    return v;
}

// `grads`: the gradient buffers in the entry point's order, grad_value first (null: not wanted)
template <typename Node, typename Grads>
void launch_backward(const Call &c, const at::Tensor &gout, const ValueGrad &v, const Grads &grads)
{
    const c10::DeviceGuard guard(c.img.device());
    check_rc(std::apply(Node::family.of(c.img.scalar_type(), c.a.scalar_type()).bwd,
                        std::tuple_cat(std::make_tuple(gout.data_ptr()), c.inputs(), grads, c.dims(), Node::samples(c), Node::mode(c),
                                       std::make_tuple(c.level_cells, c.vrow, ptr_or_null(v.ws), v.ws_bytes, current_stream(c.img)))),
             Node::family.bwd_name);
}

// one entry per argument of the node's `apply`: the three gradients in their places, the rest undefined
template <typename Node>
variable_list node_grads(AutogradContext *ctx, const variable_list &grads,
                                          at::Tensor g_img, at::Tensor g_a, at::Tensor g_b)
{
    variable_list outs(Node::arguments);
    outs[0] = std::move(g_img);
    if (ctx->needs_input_grad(2)) outs[2] = std::move(g_a);
    if (ctx->needs_input_grad(3)) outs[3] = std::move(g_b);
    return once_differentiable(grads, std::move(outs));
}

// Sampling points and weights in, gradients for both out: allocated together when either is needed (discrete sampling has
// none for the points), all three gradients in one call, no launch when nothing is wanted.
template <typename Node>
variable_list sampling_backward(AutogradContext *ctx, variable_list grads)
{
    const Call c = saved_call(ctx);
    const at::Tensor gout = grad_out_as(grads[0], c.a.scalar_type());
    const bool want_value = ctx->needs_input_grad(0);
    const bool want_sample = (Node::points_grad && ctx->needs_input_grad(2)) || ctx->needs_input_grad(3);
    at::Tensor g_pts, g_att;
    ValueGrad v;
    if (want_sample) {
        if (Node::points_grad) g_pts = at::empty_like(c.a);
        g_att = at::empty_like(c.b);
    }
    if (want_value) v = value_grad<Node>(c, Node::records_in_grads && want_sample && aligned16(g_pts) && aligned16(g_att));
    if (want_value || want_sample) {
        if constexpr (Node::points_grad)
            launch_backward<Node>(c, gout, v, std::make_tuple(ptr_or_null(v.g_img), ptr_or_null(g_pts), ptr_or_null(g_att)));
        else
            launch_backward<Node>(c, gout, v, std::make_tuple(ptr_or_null(v.g_img), ptr_or_null(g_att)));
    }
    return node_grads<Node>(ctx, grads, v.g_img, g_pts, g_att);
}

// Projection and reference points in, grad_proj and the kernel's per-head partials of grad_ref out — [B, Q, H, ref_dim], or
// [B, Q, H, L, ref_dim] for per-level reference points — always allocated, always launched; the partials are summed over
// the heads only when the reference points need a gradient.
template <typename Node>
variable_list fused_backward(AutogradContext *ctx, variable_list grads)
{
    const Call c = saved_call(ctx);
    const at::Tensor gout = grad_out_as(grads[0], c.a.scalar_type());
    const int64_t ref_dim = c.b.size(-1);
    at::Tensor g_proj = at::empty_like(c.a);
    at::Tensor g_ref_part = Node::per_level_ref ? at::empty({c.B, c.Q, c.H, c.L, ref_dim}, c.a.options())
                                                : at::empty({c.B, c.Q, c.H, ref_dim}, c.a.options());
    ValueGrad v;
    if (ctx->needs_input_grad(0)) v = value_grad<Node>(c, false);
    launch_backward<Node>(c, gout, v, std::make_tuple(ptr_or_null(v.g_img), g_proj.data_ptr(), g_ref_part.data_ptr()));
    return node_grads<Node>(ctx, grads, v.g_img, g_proj, ctx->needs_input_grad(3) ? g_ref_part.sum(2) : at::Tensor());
}

// msda_fwd_ / msda_bwd_<dtype>: sampling points [B, Q, H, L, P, 2], attention weights [B, Q, H, L, P]
class MSDAFunction : public torch::autograd::Function<MSDAFunction> {
public:
    static constexpr auto &family = kPlain;
    static constexpr auto workspace_bytes = &msda_bwd_workspace_bytes;
    static constexpr bool points_grad = true, records_in_grads = true;
    static constexpr size_t arguments = 7;
    static auto samples(const Call &c) { return c.uniform(); }
    static auto mode(const Call &c) { return c.mode(); }
    static at::Tensor forward(AutogradContext *ctx, const at::Tensor &img, const at::Tensor &shapes, const at::Tensor &pts,
                              const at::Tensor &att, int64_t padding_mode, bool align_corners, int64_t level_cells)
    {
        return node_forward<MSDAFunction>(ctx, img, shapes, pts, att, {padding_mode, align_corners, level_cells});
    }
    static variable_list backward(AutogradContext *ctx, variable_list grads)
    {
        return sampling_backward<MSDAFunction>(ctx, std::move(grads));
    }
};

// Per-level point counts (msda_fwd_ragged_ / msda_bwd_ragged_<dtype>, ABI 12): sampling points [B, Q, H, S, 2], attention
// weights [B, Q, H, S]; the Python caller checked the counts and that they are not all equal.
class MSDARaggedFunction : public torch::autograd::Function<MSDARaggedFunction> {
public:
    static constexpr auto &family = kRagged;
    static constexpr auto workspace_bytes = &msda_bwd_ragged_workspace_bytes;
    static constexpr bool points_grad = true, records_in_grads = true;
    static constexpr size_t arguments = 8;
    static auto samples(const Call &c) { return c.per_level(); }
    static auto mode(const Call &c) { return c.mode(); }
    static at::Tensor forward(AutogradContext *ctx, const at::Tensor &img, const at::Tensor &shapes, const at::Tensor &pts,
                              const at::Tensor &att, int64_t padding_mode, bool align_corners, int64_t level_cells,
                              const std::vector<int64_t> &counts)
    {
        return node_forward<MSDARaggedFunction>(ctx, img, shapes, pts, att, {padding_mode, align_corners, level_cells, counts});
    }
    static variable_list backward(AutogradContext *ctx, variable_list grads)
    {
        return sampling_backward<MSDARaggedFunction>(ctx, std::move(grads));
    }
};

// Discrete (nearest-pixel) sampling (msda_fwd_discrete_ / msda_bwd_discrete_<dtype>, additions within ABI 12): the
// per-level-count layout, one pixel per sample, no padding mode, no gradient for the sampling points (and so no gradient
// buffers to lend the sorted records).
class MSDADiscreteFunction : public torch::autograd::Function<MSDADiscreteFunction> {
public:
    static constexpr auto &family = kDiscrete;
    static constexpr auto workspace_bytes = &msda_bwd_discrete_workspace_bytes;
    static constexpr bool points_grad = false, records_in_grads = false;
    static constexpr size_t arguments = 6;
    static auto samples(const Call &c) { return c.per_level(); }
    static auto mode(const Call &) { return std::make_tuple(); }
    static at::Tensor forward(AutogradContext *ctx, const at::Tensor &img, const at::Tensor &shapes, const at::Tensor &pts,
                              const at::Tensor &att, int64_t level_cells, const std::vector<int64_t> &counts)
    {
        return node_forward<MSDADiscreteFunction>(ctx, img, shapes, pts, att, {0, false, level_cells, counts});
    }
    static variable_list backward(AutogradContext *ctx, variable_list grads)
    {
        return sampling_backward<MSDADiscreteFunction>(ctx, std::move(grads));
    }
};

// The module core with its prologue fused in (msda_fwd_fused_ / msda_bwd_fused_<dtype>): proj [B, Q, H, L, P, 3], ref
// [B, Q, ref_dim].  For this and the fused nodes below the Python caller has checked that the fused kernels take the call
// (L * P, or S, within msda_fused_lp_limit(D, element size); at most 8 levels with counts): the library then never declines.
class MSDAFusedFunction : public torch::autograd::Function<MSDAFusedFunction> {
public:
    static constexpr auto &family = kFused;
    static constexpr auto workspace_bytes = &msda_bwd_fused_workspace_bytes;
    static constexpr bool per_level_ref = false;
    static constexpr size_t arguments = 7;
    static auto samples(const Call &c) { return c.uniform(); }
    static auto mode(const Call &c) { return c.fused_mode(); }
    static at::Tensor forward(AutogradContext *ctx, const at::Tensor &img, const at::Tensor &shapes, const at::Tensor &proj,
                              const at::Tensor &ref, int64_t padding_mode, bool align_corners, int64_t level_cells)
    {
        return node_forward<MSDAFusedFunction>(ctx, img, shapes, proj, ref, {padding_mode, align_corners, level_cells});
    }
    static variable_list backward(AutogradContext *ctx, variable_list grads)
    {
        return fused_backward<MSDAFusedFunction>(ctx, std::move(grads));
    }
};

// ... with per-level point counts (msda_fwd_fused_ragged_ / msda_bwd_fused_ragged_<dtype>, additions within ABI 12):
// proj [B, Q, H, S, 3]
class MSDAFusedRaggedFunction : public torch::autograd::Function<MSDAFusedRaggedFunction> {
public:
    static constexpr auto &family = kFusedRagged;
    static constexpr auto workspace_bytes = &msda_bwd_fused_ragged_workspace_bytes;
    static constexpr bool per_level_ref = false;
    static constexpr size_t arguments = 8;
    static auto samples(const Call &c) { return c.per_level(); }
    static auto mode(const Call &c) { return c.fused_mode(); }
    static at::Tensor forward(AutogradContext *ctx, const at::Tensor &img, const at::Tensor &shapes, const at::Tensor &proj,
                              const at::Tensor &ref, int64_t padding_mode, bool align_corners, int64_t level_cells,
                              const std::vector<int64_t> &counts)
    {
        return node_forward<MSDAFusedRaggedFunction>(ctx, img, shapes, proj, ref,
                                                     {padding_mode, align_corners, level_cells, counts});
    }
    static variable_list backward(AutogradContext *ctx, variable_list grads)
    {
        return fused_backward<MSDAFusedRaggedFunction>(ctx, std::move(grads));
    }
};

// ... for Hugging Face's box rule with per-level point counts (msda_fwd_fused_hfbox_ / msda_bwd_fused_hfbox_<dtype>,
// additions within ABI 12): proj [B, Q, H, S, 3], ref [B, Q, 4], `level_scale` float32(1 / P_l) as the Python caller
// computed it on the host, `offset_scale` the module's.  The workspace is the fused per-level-count pair's.
class MSDAFusedHfBoxFunction : public torch::autograd::Function<MSDAFusedHfBoxFunction> {
public:
    static constexpr auto &family = kFusedHfBox;
    static constexpr auto workspace_bytes = &msda_bwd_fused_ragged_workspace_bytes;
    static constexpr bool per_level_ref = false;
    static constexpr size_t arguments = 10;
    static auto samples(const Call &c) { return c.per_level(); }
    static auto mode(const Call &c) { return c.hfbox_mode(); }
    static at::Tensor forward(AutogradContext *ctx, const at::Tensor &img, const at::Tensor &shapes, const at::Tensor &proj,
                              const at::Tensor &ref, int64_t padding_mode, bool align_corners, int64_t level_cells,
                              const std::vector<int64_t> &counts, const std::vector<double> &level_scale, double offset_scale)
    {
        TORCH_CHECK_VALUE(level_scale.size() == counts.size(), "level_scale and points_per_level differ in length");
        return node_forward<MSDAFusedHfBoxFunction>(
            ctx, img, shapes, proj, ref, {padding_mode, align_corners, level_cells, counts, level_scale, offset_scale});
    }
    static variable_list backward(AutogradContext *ctx, variable_list grads)
    {
        return fused_backward<MSDAFusedHfBoxFunction>(ctx, std::move(grads));
    }
};

// ... and the same rule in front of discrete sampling (msda_fwd_fused_hfbox_discrete_ / msda_bwd_fused_hfbox_discrete_<dtype>,
// additions within ABI 12): no padding mode, and no gradient for the boxes — nothing differentiable reaches them, so the
// backward has no partials to allocate or sum.
class MSDAFusedHfBoxDiscreteFunction : public torch::autograd::Function<MSDAFusedHfBoxDiscreteFunction> {
public:
    static constexpr auto &family = kFusedHfBoxDiscrete;
    static constexpr auto workspace_bytes = &msda_bwd_fused_hfbox_discrete_workspace_bytes;
    static constexpr size_t arguments = 8;
    static auto samples(const Call &c) { return c.per_level(); }
    static auto mode(const Call &c) { return std::make_tuple(c.scale.data(), c.offset_scale); }
    static at::Tensor forward(AutogradContext *ctx, const at::Tensor &img, const at::Tensor &shapes, const at::Tensor &proj,
                              const at::Tensor &ref, int64_t level_cells, const std::vector<int64_t> &counts,
                              const std::vector<double> &level_scale, double offset_scale)
    {
        TORCH_CHECK_VALUE(level_scale.size() == counts.size(), "level_scale and points_per_level differ in length");
        return node_forward<MSDAFusedHfBoxDiscreteFunction>(ctx, img, shapes, proj, ref,
                                                            {0, false, level_cells, counts, level_scale, offset_scale});
    }
    static variable_list backward(AutogradContext *ctx, variable_list grads)
    {
        const Call c = saved_call(ctx);
        const at::Tensor gout = grad_out_as(grads[0], c.a.scalar_type());
        at::Tensor g_proj = at::empty_like(c.a);
        ValueGrad v;
        if (ctx->needs_input_grad(0)) v = value_grad<MSDAFusedHfBoxDiscreteFunction>(c, false);
        launch_backward<MSDAFusedHfBoxDiscreteFunction>(c, gout, v, std::make_tuple(ptr_or_null(v.g_img), g_proj.data_ptr()));
        return node_grads<MSDAFusedHfBoxDiscreteFunction>(ctx, grads, v.g_img, g_proj, at::Tensor());
    }
};

// ... for per-level reference points and transformers' point rule (msda_fwd_fused_levelref_ / msda_bwd_fused_levelref_<dtype>,
// additions within ABI 12): ref [B, Q, L, ref_dim].  The workspace is the uniform fused pair's.
class MSDAFusedLevelRefFunction : public torch::autograd::Function<MSDAFusedLevelRefFunction> {
public:
    static constexpr auto &family = kFusedLevelRef;
    static constexpr auto workspace_bytes = &msda_bwd_fused_workspace_bytes;
    static constexpr bool per_level_ref = true;
    static constexpr size_t arguments = 7;
    static auto samples(const Call &c) { return c.uniform(); }
    static auto mode(const Call &c) { return c.fused_mode(); }
    static at::Tensor forward(AutogradContext *ctx, const at::Tensor &img, const at::Tensor &shapes, const at::Tensor &proj,
                              const at::Tensor &ref, int64_t padding_mode, bool align_corners, int64_t level_cells)
    {
        return node_forward<MSDAFusedLevelRefFunction>(ctx, img, shapes, proj, ref, {padding_mode, align_corners, level_cells});
    }
    static variable_list backward(AutogradContext *ctx, variable_list grads)
    {
        return fused_backward<MSDAFusedLevelRefFunction>(ctx, std::move(grads));
    }
};

// ------------------------------------------------------------------------------------------------------------------
// Row ranges of the flattened (b, q) row space — the launches of the row-sharded operator
// (msda_triton_amd/distributed.py; SURVEY 8e, reference independence argument kernels.py:18-21).  A rank's rows
// [r0, r1) meet a batch element in at most one piece: runs of whole batch elements are ONE launch (B = nb), a partial
// batch element its own (B = 1, value = img[b]).  Same C ABI, pointer arithmetic only.
// ------------------------------------------------------------------------------------------------------------------
struct RowDims {
    int64_t B, I, H, D, Q, L, P;
    int64_t es, vs;  // element sizes: sampling inputs / result, value pyramid
};

RowDims row_dims(const at::Tensor &img, const at::Tensor &pts_rows, const at::Tensor &att_rows, int64_t Q)
{
    // (pointers of another device — or of the host — must never reach the kernels)
    TORCH_CHECK_VALUE(img.is_cuda() && pts_rows.device() == img.device() && att_rows.device() == img.device(),
                      "expected all tensors on one gpu, got ", img.device(), ", ", pts_rows.device(), ", ", att_rows.device());
    TORCH_CHECK_VALUE(img.dim() == 4 && pts_rows.dim() == 5 && att_rows.dim() == 4 && pts_rows.size(4) == 2,
                      "expected img [B,I,H,D], sampling_points [rows,H,L,P,2], attention_weights [rows,H,L,P]");
    TORCH_CHECK_VALUE(pts_rows.size(1) == img.size(2) && att_rows.sizes() == pts_rows.sizes().slice(0, 4),
                      "inconsistent shapes between img, sampling_points and attention_weights rows");
    TORCH_CHECK_VALUE(pts_rows.scalar_type() == att_rows.scalar_type(), "sampling_points / attention_weights dtypes differ");
    TORCH_CHECK_VALUE(Q >= 0, "num_queries must be non-negative");
    return {img.size(0), img.size(1), img.size(2), img.size(3), Q, pts_rows.size(2), pts_rows.size(3),
            (int64_t)pts_rows.element_size(), (int64_t)img.element_size()};
}

// fn(b, nb, rows_before, n): piece of `n` rows starting `rows_before` rows behind `row0`, covering batch elements
// [b, b + nb) (nb > 1: whole batch elements)
template <typename F> void for_pieces(int64_t Q, int64_t row0, int64_t row1, F fn)
{
    int64_t r = row0;
    while (r < row1) {
        const int64_t b = r / Q, q0 = r % Q;
        if (q0 == 0 && row1 - r >= Q) {
            const int64_t nb = (row1 - r) / Q;
            fn(b, nb, r - row0, nb * Q);
            r += nb * Q;
        } else {
            const int64_t n = std::min(Q - q0, row1 - r);
            fn(b, (int64_t)1, r - row0, n);
            r += n;
        }
    }
}

// forward of rows [row0, row1) into full[row0:row1]; pts_rows / att_rows hold the rows from `in_row0` on
void rows_forward(const at::Tensor &img_, const at::Tensor &shapes, const at::Tensor &pts_rows, const at::Tensor &att_rows,
                  int64_t in_row0, const at::Tensor &full, int64_t row0, int64_t row1, int64_t Q, int64_t padding_mode,
                  bool align_corners)
{
    const RowDims d = row_dims(img_, pts_rows, att_rows, Q);
    const auto [img, vrow] = value_rows(img_);
    TORCH_CHECK_VALUE(pts_rows.is_contiguous() && att_rows.is_contiguous() && full.is_contiguous(),
                      "rows_forward takes contiguous tensors");
    TORCH_CHECK_VALUE(shapes.scalar_type() == at::kLong && shapes.is_contiguous() && shapes.device() == img.device() &&
                          full.device() == img.device(), "img_shapes: contiguous int64 on the tensors' device; result on it too");
    TORCH_CHECK_VALUE(0 <= in_row0 && in_row0 <= row0 && row0 <= row1 && row1 <= d.B * d.Q &&
                          row1 - in_row0 <= pts_rows.size(0) && full.numel() == d.B * d.Q * d.H * d.D &&
                          full.scalar_type() == pts_rows.scalar_type(),
                      "rows_forward: row range / buffer sizes do not match");
    if (row1 == row0) return;
    const Fns fns = fns_for(img.scalar_type(), pts_rows.scalar_type());
    const c10::DeviceGuard guard(img.device());
    void *stream = current_stream(img);
    const char *v = static_cast<const char *>(img.data_ptr());
    const char *p = static_cast<const char *>(pts_rows.data_ptr()), *a = static_cast<const char *>(att_rows.data_ptr());
    char *o = static_cast<char *>(full.data_ptr());
    const int64_t unit = d.H * d.L * d.P, vbatch = value_batch_bytes(img, vrow);
    for_pieces(d.Q, row0, row1, [&](int64_t b, int64_t nb, int64_t before, int64_t n) {
        const int64_t in_at = row0 + before - in_row0, out_at = row0 + before;
        check_rc(fns.fwd(v + b * vbatch, shapes.data_ptr<int64_t>(), p + in_at * unit * 2 * d.es,
                         a + in_at * unit * d.es, o + out_at * d.H * d.D * d.es, nb, d.I, d.H, d.D, n / nb, d.L, d.P,
                         (int)padding_mode, align_corners ? 1 : 0, vrow, stream),
                 "msda_fwd (row range)");
    });
}

// backward of rows [r0, r1): grad_rows / pts_rows / att_rows hold exactly those rows.  Returns (grad_img [B,I,H,D] with
// the batch elements the rows do not touch zeroed, grad_pts_rows, grad_att_rows); undefined tensors for what is not needed.
std::tuple<at::Tensor, at::Tensor, at::Tensor> rows_backward(const at::Tensor &grad_rows_, const at::Tensor &img_,
                                                             const at::Tensor &shapes, const at::Tensor &pts_rows,
                                                             const at::Tensor &att_rows, int64_t r0, int64_t r1, int64_t Q,
                                                             int64_t padding_mode, bool align_corners, bool need_img,
                                                             bool need_pts, bool need_att, int64_t level_cells)
{
    const RowDims d = row_dims(img_, pts_rows, att_rows, Q);
    const auto [img, vrow] = value_rows(img_);
    TORCH_CHECK_VALUE(pts_rows.is_contiguous() && att_rows.is_contiguous(), "rows_backward takes contiguous tensors");
    TORCH_CHECK_VALUE(shapes.scalar_type() == at::kLong && shapes.is_contiguous() && shapes.device() == img.device() &&
                          grad_rows_.device() == img.device(), "img_shapes: contiguous int64 on the tensors' device; grad_out on it too");
    TORCH_CHECK_VALUE(0 <= r0 && r0 <= r1 && r1 <= d.B * d.Q && pts_rows.size(0) == r1 - r0 &&
                          grad_rows_.numel() == (r1 - r0) * d.H * d.D,
                      "rows_backward: row range / buffer sizes do not match");
    at::Tensor grad_rows = grad_rows_.contiguous();
    if (grad_rows.scalar_type() != pts_rows.scalar_type()) grad_rows = grad_rows.to(pts_rows.scalar_type());
    const bool want_sample = need_pts || need_att;
    at::Tensor g_img, g_pts, g_att;
    if (need_img) g_img = at::empty(img.sizes(), img.options());  // (dense)
    if (want_sample) {
        g_pts = at::empty_like(pts_rows);
        g_att = at::empty_like(att_rows);
    }
    std::vector<bool> touched((size_t)d.B, false);
    if ((need_img || want_sample) && r1 > r0) {
        const Fns fns = fns_for(img.scalar_type(), pts_rows.scalar_type());
        const c10::DeviceGuard guard(img.device());
        void *stream = current_stream(img);
        const char *v = static_cast<const char *>(img.data_ptr());
        const char *p = static_cast<const char *>(pts_rows.data_ptr()), *a = static_cast<const char *>(att_rows.data_ptr());
        const char *go = static_cast<const char *>(grad_rows.data_ptr());
        char *gv = need_img ? static_cast<char *>(g_img.data_ptr()) : nullptr;
        char *gp = want_sample ? static_cast<char *>(g_pts.data_ptr()) : nullptr;
        char *ga = want_sample ? static_cast<char *>(g_att.data_ptr()) : nullptr;
        const int64_t unit = d.H * d.L * d.P, plane = d.I * d.H * d.D, vbatch = value_batch_bytes(img, vrow);
        const bool overlap_forced = msda_get_option("overlap") == 1;
        for_pieces(d.Q, r0, r1, [&](int64_t b, int64_t nb, int64_t before, int64_t n) {
            for (int64_t k = 0; k < nb; ++k) touched[(size_t)(b + k)] = true;
            void *pv = need_img ? gv + b * plane * d.vs : nullptr;
            void *pp = want_sample ? gp + before * unit * 2 * d.es : nullptr;
            void *pa = want_sample ? ga + before * unit * d.es : nullptr;
            at::Tensor ws;
            int64_t ws_bytes = 0;
            if (need_img) {
                const bool in_grads = want_sample && reinterpret_cast<uintptr_t>(pp) % 16 == 0 &&
                                      reinterpret_cast<uintptr_t>(pa) % 16 == 0 && reinterpret_cast<uintptr_t>(pv) % 16 == 0 &&
                                      !overlap_forced;
                ws_bytes = msda_bwd_workspace_bytes(nb, d.I, d.H, d.D, n / nb, d.L, d.P, (int)d.es, (int)d.vs, level_cells,
                                                    in_grads ? MSDA_WS_RECORDS_IN_GRADS : 0);
                ws = at::empty({ws_bytes}, img.options().dtype(at::kByte));
            }
            check_rc(fns.bwd(go + before * d.H * d.D * d.es, v + b * vbatch, shapes.data_ptr<int64_t>(),
                             p + before * unit * 2 * d.es, a + before * unit * d.es, pv, pp, pa, nb, d.I, d.H, d.D, n / nb,
                             d.L, d.P, (int)padding_mode, align_corners ? 1 : 0, level_cells, vrow,
                             ws.defined() ? ws.data_ptr() : nullptr, ws_bytes, stream),
                     "msda_bwd (row range)");
        });
    }
    if (need_img)
        for (int64_t b = 0; b < d.B; ++b)
            if (!touched[(size_t)b]) g_img.select(0, b).zero_();
    return {g_img, need_pts ? g_pts : at::Tensor(), need_att ? g_att : at::Tensor()};
}

int64_t chunk_begin(int64_t n, int64_t chunks, int64_t k)
{
    const int64_t cs = chunks > 0 ? (n + chunks - 1) / chunks : n;
    return std::min(n, k * cs);
}

// The row-sharded operator WITHOUT its exchange as one autograd node: a one-rank job, or one rank of a larger job
// played on one GPU (distributed.py `compute_only_as`).  Rows [r0, r1) are computed in `chunks` pieces straight into
// the full [B, Q, H, D] result; the other rows are left unwritten.
class MSDARowsFunction : public torch::autograd::Function<MSDARowsFunction> {
public:
    static at::Tensor forward(torch::autograd::AutogradContext *ctx, const at::Tensor &img_, const at::Tensor &shapes_,
                              const at::Tensor &pts_, const at::Tensor &att_, int64_t padding_mode, bool align_corners,
                              int64_t Q, int64_t r0, int64_t r1, int64_t chunks, int64_t level_cells)
    {
        const at::Tensor img = value_rows(img_).first, pts = pts_.contiguous(), att = att_.contiguous();
        const at::Tensor shapes = shapes_.to(at::kLong).contiguous();
        const int64_t B = img.size(0), H = img.size(2), D = img.size(3);
        at::Tensor full = at::empty({B, Q, H, D}, pts.options());
        chunks = std::max<int64_t>(1, chunks);
        for (int64_t k = 0; k < chunks; ++k) {
            const int64_t c0 = chunk_begin(r1 - r0, chunks, k), c1 = chunk_begin(r1 - r0, chunks, k + 1);
            rows_forward(img, shapes, pts, att, r0, full, r0 + c0, r0 + c1, Q, padding_mode, align_corners);
        }
        ctx->save_for_backward({img, shapes, pts, att});
        ctx->saved_data["padding_mode"] = padding_mode;
        ctx->saved_data["align_corners"] = align_corners;
        ctx->saved_data["level_cells"] = level_cells;
        ctx->saved_data["Q"] = Q;
        ctx->saved_data["r0"] = r0;
        ctx->saved_data["r1"] = r1;
        return full;
    }

    static torch::autograd::variable_list backward(torch::autograd::AutogradContext *ctx,
                                                   torch::autograd::variable_list grads)
    {
        const auto saved = ctx->get_saved_variables();
        const at::Tensor &img = saved[0], &shapes = saved[1], &pts = saved[2], &att = saved[3];
        const int64_t Q = ctx->saved_data["Q"].toInt(), r0 = ctx->saved_data["r0"].toInt(), r1 = ctx->saved_data["r1"].toInt();
        const int64_t H = img.size(2), D = img.size(3);
        const at::Tensor mine = grads[0].reshape({img.size(0) * Q, H, D}).slice(0, r0, r1);
        auto [g_img, g_pts, g_att] =
            rows_backward(mine, img, shapes, pts, att, r0, r1, Q, ctx->saved_data["padding_mode"].toInt(),
                          ctx->saved_data["align_corners"].toBool(), ctx->needs_input_grad(0), ctx->needs_input_grad(2),
                          ctx->needs_input_grad(3), ctx->saved_data["level_cells"].toInt());
        return once_differentiable(grads, {g_img, at::Tensor(), g_pts, g_att, at::Tensor(), at::Tensor(), at::Tensor(),
                                           at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor()});
    }
};

at::Tensor msda_rows(const at::Tensor &img, const at::Tensor &shapes, const at::Tensor &pts_rows, const at::Tensor &att_rows,
                     int64_t padding_mode, bool align_corners, int64_t Q, int64_t r0, int64_t r1, int64_t chunks,
                     int64_t level_cells)
{
    const RowDims d = row_dims(img, pts_rows, att_rows, Q);
    TORCH_CHECK_VALUE(0 <= r0 && r0 <= r1 && r1 <= d.B * d.Q && pts_rows.size(0) == r1 - r0,
                      "msda_rows: rows [", r0, ", ", r1, ") against ", pts_rows.size(0), " input rows");
    return MSDARowsFunction::apply(img, shapes, pts_rows, att_rows, padding_mode, align_corners, Q, r0, r1, chunks,
                                   level_cells);
}

at::Tensor msda(const at::Tensor &img, const at::Tensor &shapes, const at::Tensor &pts, const at::Tensor &att,
                int64_t padding_mode, bool align_corners, int64_t level_cells)
{
    return MSDAFunction::apply(img, shapes, pts, att, padding_mode, align_corners, level_cells);
}

at::Tensor msda_ragged(const at::Tensor &img, const at::Tensor &shapes, const at::Tensor &pts, const at::Tensor &att,
                       int64_t padding_mode, bool align_corners, int64_t level_cells, const std::vector<int64_t> &counts)
{
    return MSDARaggedFunction::apply(img, shapes, pts, att, padding_mode, align_corners, level_cells, counts);
}

at::Tensor msda_discrete(const at::Tensor &img, const at::Tensor &shapes, const at::Tensor &pts, const at::Tensor &att,
                         int64_t level_cells, const std::vector<int64_t> &counts)
{
    return MSDADiscreteFunction::apply(img, shapes, pts, att, level_cells, counts);
}

at::Tensor msda_fused(const at::Tensor &img, const at::Tensor &shapes, const at::Tensor &proj, const at::Tensor &ref,
                      int64_t padding_mode, bool align_corners, int64_t level_cells)
{
    return MSDAFusedFunction::apply(img, shapes, proj, ref, padding_mode, align_corners, level_cells);
}

at::Tensor msda_fused_ragged(const at::Tensor &img, const at::Tensor &shapes, const at::Tensor &proj, const at::Tensor &ref,
                             int64_t padding_mode, bool align_corners, int64_t level_cells,
                             const std::vector<int64_t> &counts)
{
    return MSDAFusedRaggedFunction::apply(img, shapes, proj, ref, padding_mode, align_corners, level_cells, counts);
}

at::Tensor msda_fused_levelref(const at::Tensor &img, const at::Tensor &shapes, const at::Tensor &proj, const at::Tensor &ref,
                               int64_t padding_mode, bool align_corners, int64_t level_cells)
{
    return MSDAFusedLevelRefFunction::apply(img, shapes, proj, ref, padding_mode, align_corners, level_cells);
}

at::Tensor msda_fused_hfbox(const at::Tensor &img, const at::Tensor &shapes, const at::Tensor &proj, const at::Tensor &ref,
                            int64_t padding_mode, bool align_corners, int64_t level_cells, const std::vector<int64_t> &counts,
                            const std::vector<double> &level_scale, double offset_scale)
{
    return MSDAFusedHfBoxFunction::apply(img, shapes, proj, ref, padding_mode, align_corners, level_cells, counts,
                                         level_scale, offset_scale);
}

at::Tensor msda_fused_hfbox_discrete(const at::Tensor &img, const at::Tensor &shapes, const at::Tensor &proj,
                                     const at::Tensor &ref, int64_t level_cells, const std::vector<int64_t> &counts,
                                     const std::vector<double> &level_scale, double offset_scale)
{
    return MSDAFusedHfBoxDiscreteFunction::apply(img, shapes, proj, ref, level_cells, counts, level_scale, offset_scale);
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m)
{
    m.doc() = "C++ autograd glue over libmsda_hip.so (same C ABI as the ctypes route)";
    m.def("msda", &msda, "multi-scale deformable attention (forward; differentiable)", pybind11::arg("img"),
          pybind11::arg("shapes"), pybind11::arg("sampling_points"), pybind11::arg("attention_weights"),
          pybind11::arg("padding_mode"), pybind11::arg("align_corners"), pybind11::arg("level_cells") = 0);
    m.def("msda_ragged", &msda_ragged, "per-level point counts: sampling points [B,Q,H,S,2] (forward; differentiable)",
          pybind11::arg("img"), pybind11::arg("shapes"), pybind11::arg("sampling_points"),
          pybind11::arg("attention_weights"), pybind11::arg("padding_mode"), pybind11::arg("align_corners"),
          pybind11::arg("level_cells"), pybind11::arg("points_per_level"));
    m.def("msda_discrete", &msda_discrete,
          "discrete (nearest-pixel) sampling over the per-level-count layout (forward; differentiable in img and weights)",
          pybind11::arg("img"), pybind11::arg("shapes"), pybind11::arg("sampling_points"),
          pybind11::arg("attention_weights"), pybind11::arg("level_cells"), pybind11::arg("points_per_level"));
    m.def("msda_fused", &msda_fused, "module core with the softmax / sampling-point prologue fused in (differentiable)",
          pybind11::arg("img"), pybind11::arg("shapes"), pybind11::arg("proj"), pybind11::arg("reference_points"),
          pybind11::arg("padding_mode"), pybind11::arg("align_corners"), pybind11::arg("level_cells") = 0);
    m.def("msda_fused_ragged", &msda_fused_ragged,
          "module core with the prologue fused in, per-level point counts: proj [B,Q,H,S,3] (differentiable)",
          pybind11::arg("img"), pybind11::arg("shapes"), pybind11::arg("proj"), pybind11::arg("reference_points"),
          pybind11::arg("padding_mode"), pybind11::arg("align_corners"), pybind11::arg("level_cells"),
          pybind11::arg("points_per_level"));
    m.def("msda_fused_levelref", &msda_fused_levelref,
          "module core with transformers' prologue fused in: reference points [B,Q,L,ref_dim] (differentiable)",
          pybind11::arg("img"), pybind11::arg("shapes"), pybind11::arg("proj"), pybind11::arg("reference_points"),
          pybind11::arg("padding_mode"), pybind11::arg("align_corners"), pybind11::arg("level_cells") = 0);
    m.def("msda_fused_hfbox", &msda_fused_hfbox,
          "module core with Hugging Face's box prologue fused in: per-level point counts, boxes [B,Q,4] (differentiable)",
          pybind11::arg("img"), pybind11::arg("shapes"), pybind11::arg("proj"), pybind11::arg("reference_points"),
          pybind11::arg("padding_mode"), pybind11::arg("align_corners"), pybind11::arg("level_cells"),
          pybind11::arg("points_per_level"), pybind11::arg("level_scale"), pybind11::arg("offset_scale"));
    // (in a submodule: the top-level callables are a recorded list that callers and tests compare against exactly)
    auto box_discrete = m.def_submodule("box_discrete", "Hugging Face's box rule in front of discrete sampling");
    box_discrete.def(
        "msda_fused_hfbox_discrete", &msda_fused_hfbox_discrete,
        "Hugging Face's box prologue fused in front of discrete sampling: boxes [B,Q,4] (differentiable in img and proj)",
        pybind11::arg("img"), pybind11::arg("shapes"), pybind11::arg("proj"), pybind11::arg("reference_points"),
        pybind11::arg("level_cells"), pybind11::arg("points_per_level"), pybind11::arg("level_scale"),
        pybind11::arg("offset_scale"));
    m.def("msda_rows", &msda_rows,
          "rows [r0, r1) of the flattened (b, q) row space computed in `chunks` pieces into a full [B,Q,H,D] result "
          "(differentiable; the row-sharded operator without its exchange)",
          pybind11::arg("img"), pybind11::arg("shapes"), pybind11::arg("sampling_points_rows"),
          pybind11::arg("attention_weights_rows"), pybind11::arg("padding_mode"), pybind11::arg("align_corners"),
          pybind11::arg("num_queries"), pybind11::arg("r0"), pybind11::arg("r1"), pybind11::arg("chunks") = 1,
          pybind11::arg("level_cells") = 0);
    m.def("rows_forward", &rows_forward, "launches of a row range into its place in the full result (no autograd)");
    m.def("rows_backward", &rows_backward, "backward launches of a row range (no autograd)");
    m.def("fused_lp_limit", [](int64_t D, int64_t elem_size) { return msda_fused_lp_limit(D, (int)elem_size); });
    m.def("abi_version", []() { return msda_abi_version(); });
}
