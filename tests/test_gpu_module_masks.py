"""GPU: both padding masks inside the nn.Module's own fused kernels (msda_{fwd,bwd}_fused_masked_<suffix>,
msda_{fwd,bwd}_fused_ragged_masked_<suffix>), through `fused_module_core(value_mask=, query_mask=)`, the launchers and
`MultiscaleDeformableAttention.forward`.

The bar is EQUALITY, as for the value-mask and query-mask kernels before (tests/test_gpu_value_mask.py,
tests/test_gpu_query_mask.py): the masked kernels on a pyramid whose padding pixels hold NaN (+Inf for the "rect" mask) give,
bit for bit, what the unmasked fused twin gives on where(mask, value, 0) at the same options; a query mask leaves the real
queries' rows as they were and stores zeros for the others.  Both legs run the Python `Function` (under a KernelTimer): the
C++ node of the unmasked pair sums the grad_reference_points partials in another order.  The CPU oracle on the pre-masked
pyramid is held next to it at tests/test_gpu_parity.py's bounds, so that a fault shared by both GPU routes cannot hide."""
import contextlib
import zlib

import numpy as np
import pytest
import torch

import query_mask_cases as qmc
from conftest import kink_mask
from guarded_alloc import contract_violations
from msda_triton_amd import MultiscaleDeformableAttention, _lib, functional, module as msda_module, ragged
from msda_triton_amd.functional import KernelTimer, fused_module_core, module_sampling_inputs
from msda_triton_amd.ragged import ragged_module_sampling_inputs
from test_gpu_fused_ragged import COUNTS, SHAPES, make
from test_gpu_lds_levels import CASES as LDS_CASES
from test_gpu_parity import BWD_TOL, DEV, FWD_TOL, SHAPE_MATRIX
from test_gpu_value_mask import MASKS, assert_contract, make_mask, no_composition, options, poisoned, premasked

pytestmark = pytest.mark.gpu

UNIFORM = {k: LDS_CASES[k] for k in ("c2_like_f32", "many_samples_two_trips", "bf16_g4", "f64", "d64_f32_g16")}
UNIFORM["d5_scalar"] = SHAPE_MATRIX["d5_scalar"] + (torch.float32,)
PAIRS = [("zeros", False), ("border", True)]
HOSTILE = (float("nan"), float("inf"), 1e30)


def uniform_inputs(B, Q, H, D, levels, P, ref_dim, seed, dtype=torch.float32):
    g = torch.Generator(device="cpu").manual_seed(seed)
    value = torch.randn(B, sum(h * w for h, w in levels), H, D, generator=g, dtype=torch.float64).to(dtype)
    proj = (torch.randn(B, Q, H, len(levels), P, 3, generator=g, dtype=torch.float64) * 1.5).to(dtype)
    ref = torch.rand(B, Q, ref_dim, generator=g, dtype=torch.float64).to(dtype)
    gout = torch.rand(B, Q, H, D, generator=g, dtype=torch.float64).to(dtype)
    return [t.to(DEV) for t in (value, torch.tensor(levels), proj, ref, gout)]


def core_run(v, s, pr, rf, go, pm, ac, counts=None, vm=None, qm=None, timed=True, **kw):
    """forward + backward of the core -> (out, grad_value, grad_proj, grad_ref); `timed`: inside a KernelTimer, which keeps
    the unmasked leg on the Python Function too"""
    v, pr, rf = (t.detach().clone().requires_grad_(True) for t in (v, pr, rf))
    with (KernelTimer() if timed else contextlib.nullcontext()):
        out = fused_module_core(v, s, pr, rf, pm, ac, None, counts, vm, qm, **kw)
        out.backward(go.to(out.dtype))
    torch.cuda.synchronize()
    return out.detach(), v.grad, pr.grad, rf.grad


@contextlib.contextmanager
def nothing_composed(calls=None):
    """no_composition() for the value mask plus the same spy on functional.apply_query_mask"""
    real = functional.apply_query_mask

    def spy(per_query, query_mask, fill=0.0):
        if query_mask is not None:
            if calls is None:
                raise AssertionError("the query mask was composed instead of going into the kernels")
            calls.append(1)
        return real(per_query, query_mask, fill)

    functional.apply_query_mask = spy
    try:
        with no_composition(calls):
            yield
    finally:
        functional.apply_query_mask = real


def taken_by_the_kernels(v, pr, rf, counts=None):
    S = pr.shape[3] * pr.shape[4] if counts is None else pr.shape[3]
    return functional.module_masks_in_kernels(v, pr, rf, S, None if counts is None else len(counts))


def rows(t, m):
    return m.reshape(m.shape + (1,) * (t.dim() - 2)).expand_as(t)


def assert_per_unit(got, plain, qm, what):
    """everything but grad_value (index 1): real queries' rows equal plain's, masked queries' rows are zeros"""
    for i, (g, w) in enumerate(zip(got, plain)):
        if i == 1:
            continue
        sel = rows(g, qm)
        assert torch.equal(g[sel], w[sel]), f"{what}: result {i}, real rows differ from the call without the query mask"
        assert torch.equal(g[~sel], torch.zeros_like(g[~sel])), f"{what}: result {i}, a masked row is not zeros"


def value_mask_contract(c, levels, counts, seed, what):
    v, s, pr, rf, go = c
    B = v.shape[0]
    in_kernels = taken_by_the_kernels(v, pr, rf, counts)
    for kind in MASKS:
        m = make_mask(kind, B, levels, seed).to(DEV)
        vp = poisoned(v, m, float("inf") if kind == "rect" else float("nan"))
        pre = premasked(v, m)
        for pm, ac in PAIRS:
            ref = {}
            for lds in (0, 2):
                with options(lds_levels=lds):
                    want = core_run(pre, s, pr, rf, go, pm, ac, counts)
                    composed = []
                    with nothing_composed(None if in_kernels else composed):
                        got = core_run(vp, s, pr, rf, go, pm, ac, counts, m)
                        info = _lib.last_launch_info()
                    assert in_kernels or composed, what  # (a shape the fused kernels decline composes, as before)
                tag = f"{what} {kind} {pm}/{ac} lds_levels={lds}"
                assert_contract(got, want, m, tag)
                assert not torch.signbit(got[1][~m]).any(), tag  # +0
                assert info["fwd_variant"] in (0, 1), (tag, info)  # never the one-wave-per-unit forward
                ref[lds] = got
            for x, y in zip(ref[0], ref[2]):  # (the variants are bit-identical among themselves, as their twins are)
                assert torch.equal(x, y)
            if kind == "all_ones":  # equals the unmasked call on the raw pyramid
                with options(lds_levels=0):
                    raw = core_run(v, s, pr, rf, go, pm, ac, counts)
                for x, y in zip(ref[0], raw):
                    assert torch.equal(x, y)
    return in_kernels


# ------------------------------------------------------------------------------------------ 1 the value mask
@pytest.mark.parametrize("ref_dim", [2, 4])
@pytest.mark.parametrize("name", list(UNIFORM))
def test_uniform_pair_equals_the_unmasked_twin_on_the_premasked_pyramid(name, ref_dim):
    B, Q, H, D, levels, P, td = UNIFORM[name]
    seed = zlib.crc32(f"mm{name}{ref_dim}".encode())
    c = uniform_inputs(B, Q, H, D, levels, P, ref_dim, seed, td)
    in_kernels = value_mask_contract(c, levels, None, seed, f"{name} ref_dim {ref_dim}")
    # L * P = 40 samples per unit are beyond one LDS pass of the fused backward: that call composes; every other shape is the kernels'
    assert in_kernels == (name != "many_samples_two_trips")


@pytest.mark.parametrize("ref_dim", [2, 4])
@pytest.mark.parametrize("cname", list(COUNTS))
@pytest.mark.parametrize("name", list(SHAPES))
def test_ragged_pair_equals_the_unmasked_twin_on_the_premasked_pyramid(name, cname, ref_dim):
    counts = COUNTS[cname]
    B, Q, H, D, levels = SHAPES[name]
    seed = zlib.crc32(f"mr{name}{cname}{ref_dim}".encode())
    c = make(B, Q, H, D, levels, counts, ref_dim, seed)
    assert value_mask_contract(c, levels[:len(counts)], counts, seed, f"{name} {cname} ref_dim {ref_dim}")


# ------------------------------------------------------------------------------------------ 2 both grad_value routes
def _route_case(layout):
    if layout == "uniform":
        B, Q, H, D, levels, P, td = UNIFORM["c2_like_f32"]
        return uniform_inputs(B, Q, H, D, levels, P, 4, 41, td), levels, None
    B, Q, H, D, levels = SHAPES["d32"]
    counts = COUNTS["3_6_3"]
    return make(B, Q, H, D, levels, counts, 4, 43), levels[:len(counts)], counts


@pytest.mark.parametrize("rig", [0, 1], ids=["records_in_workspace", "records_in_grads"])
@pytest.mark.parametrize("path,passes", [(2, 1), (2, 2), (3, 1)], ids=["sorted", "sorted_two_passes", "single_launch"])
@pytest.mark.parametrize("layout", ["uniform", "ragged"])
def test_both_grad_value_routes(layout, path, passes, rig):
    (v, s, pr, rf, go), levels, counts = _route_case(layout)
    B, Q = v.shape[0], pr.shape[1]
    for kind in ("bernoulli", "level_edges", "element0_masked"):
        m = make_mask(kind, B, levels, 7).to(DEV)
        with options(value_path=path, ws_passes=passes, records_in_grads=rig):
            want = core_run(premasked(v, m), s, pr, rf, go, "zeros", False, counts)
            info_want = _lib.last_launch_info()
            with nothing_composed():
                got = core_run(poisoned(v, m, float("nan")), s, pr, rf, go, "zeros", False, counts, m)
                info = _lib.last_launch_info()
                # ... and with a query mask on top: the count / place passes (the single-launch kernel's walks) on the masked kernarg
                qm = qmc.make_query_mask("tail", B, Q, 7).to(DEV)
                both = core_run(poisoned(v, m, float("nan")), s, pr, rf, go, "zeros", False, counts, m, qm)
                info_q = _lib.last_launch_info()
                again = core_run(poisoned(v, m, float("nan")), s, pr, rf, go, "zeros", False, counts, m, qm)
        for i in (info, info_want, info_q):
            assert i["value_path"] == (1 if path == 3 else 2) and i["value_passes"] == passes, (kind, i)
        assert_contract(got, want, m, kind)
        assert not torch.signbit(got[1][~m]).any()
        assert_per_unit(both, got, qm, kind)
        assert torch.equal(both[1][~m], torch.zeros_like(both[1][~m])) and not torch.signbit(both[1][~m]).any()
        for x, y in zip(both, again):
            assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------ 3 the query mask
def query_mask_contract(c, levels, counts, P, seed, what):
    v, s, pr, rf, go = c
    B, Q, H, D = v.shape[0], pr.shape[1], v.shape[2], v.shape[3]
    for kind in qmc.KINDS:
        qm = qmc.make_query_mask(kind, B, Q, seed, (B, Q, H, D, levels, P, v.element_size())).to(DEV)
        for vm in (None, make_mask("rect", B, levels, seed).to(DEV)):
            for pm, ac in PAIRS:
                for lds in (0, 2):
                    with options(lds_levels=lds):
                        plain = core_run(v, s, pr, rf, go, pm, ac, counts, vm)
                        with nothing_composed():
                            got = core_run(v, s, pr, rf, go, pm, ac, counts, vm, qm)
                            info = _lib.last_launch_info()
                            again = core_run(v, s, pr, rf, go, pm, ac, counts, vm, qm)
                    tag = f"{what} {kind} {pm}/{ac} lds_levels={lds} value_mask={'rect' if vm is not None else None}"
                    assert_per_unit(got, plain, qm, tag)
                    # a fused backward with a query mask: the 256-thread sample-gradient kernel; never the unit forward
                    assert info["sample_variant"] == 0 and info["fwd_variant"] in (0, 1), (tag, info)
                    for x, y in zip(got, again):
                        assert torch.equal(x, y), tag
                    if kind == "all_ones":
                        assert torch.equal(got[1], plain[1]), tag
                    if kind == "all_zeros":
                        assert torch.equal(got[1], torch.zeros_like(got[1])), tag


@pytest.mark.parametrize("ref_dim", [2, 4])
@pytest.mark.parametrize("name", ["c2_like_f32", "bf16_g4", "d5_scalar"])
def test_uniform_pair_real_rows_equal_the_plain_call_and_masked_rows_are_zeros(name, ref_dim):
    B, Q, H, D, levels, P, td = UNIFORM[name]
    seed = zlib.crc32(f"mq{name}{ref_dim}".encode())
    query_mask_contract(uniform_inputs(B, Q, H, D, levels, P, ref_dim, seed, td), levels, None, P, seed, name)


@pytest.mark.parametrize("ref_dim", [2, 4])
@pytest.mark.parametrize("name", ["d32", "d5", "d64"])
def test_ragged_pair_real_rows_equal_the_plain_call_and_masked_rows_are_zeros(name, ref_dim):
    counts = COUNTS["3_6_3"]
    B, Q, H, D, levels = SHAPES[name]
    seed = zlib.crc32(f"mqr{name}{ref_dim}".encode())
    query_mask_contract(make(B, Q, H, D, levels, counts, ref_dim, seed), levels[:3], counts, max(counts), seed, name)


@pytest.mark.parametrize("layout", ["uniform", "ragged"])
def test_nothing_a_masked_query_holds_reaches_a_result(layout):
    (v, s, pr, rf, go), levels, counts = _route_case(layout)
    B, Q = v.shape[0], pr.shape[1]
    for kind in ("bernoulli", "tail"):
        qm = qmc.make_query_mask(kind, B, Q, 5).to(DEV)
        for vm in (None, make_mask("rect", B, levels, 5).to(DEV)):
            for path in (2, 3):
                with options(value_path=path):
                    benign = core_run(v, s, pr, rf, go, "zeros", False, counts, vm, qm)
                    for which in ((0,), (1,), (2,), (0, 1, 2)):
                        p2, r2, g2 = (qmc.hostile_fill(t, qm, HOSTILE) if i in which else t for i, t in enumerate((pr, rf, go)))
                        got = core_run(v, s, p2, r2, g2, "zeros", False, counts, vm, qm)
                        for x, y in zip(got, benign):
                            assert torch.isfinite(x).all() and torch.equal(x, y), (layout, kind, path, which)


def _exact_inputs(counts, ref_dim, seed):
    """Fused inputs on which every sum of the backward is exactly representable in float32, so that grad_value does not
    depend on where the gather cuts its windows (tests/query_mask_cases.py states why only such inputs can be compared
    bit for bit): power-of-two levels, equal logits over a power-of-two sample count (the softmax is 1 / S <= 1 / 16
    exactly), reference points on multiples of 1 / 4 and integer offsets (a box of size 1: offset / (2 P) is a multiple of
    1 / 8), so that every pixel coordinate is a multiple of 1 / 4 on every level and a sample's four weights are multiples of
    2^-8; rows of small integers.  A pixel of the coarsest level collects at most Q * P = 1200 samples of weight * row <= 7:
    8 fraction bits under 14 integer bits, inside float32's 24."""
    levels = [(16, 16), (8, 8), (4, 4), (2, 2)][:len(counts)]
    B, Q, H, D = 2, 300, 4, 32
    g = torch.Generator(device="cpu").manual_seed(seed)
    S = sum(counts)
    assert S & (S - 1) == 0
    value = torch.randint(-4, 5, (B, sum(h * w for h, w in levels), H, D), generator=g).float()
    proj = torch.zeros(B, Q, H, S, 3)
    proj[..., :2] = torch.randint(-2, 3, (B, Q, H, S, 2), generator=g).float()
    ref = torch.randint(0, 5, (B, Q, ref_dim), generator=g).float() / 4
    if ref_dim == 4:
        ref[..., 2:] = 1.0
    gout = torch.randint(0, 8, (B, Q, H, D), generator=g).float()
    return [t.to(DEV) for t in (value, torch.tensor(levels), proj, ref, gout)], levels


@pytest.mark.parametrize("path,passes", [(2, 1), (2, 2), (3, 1)], ids=["sorted", "sorted_two_passes", "single_launch"])
@pytest.mark.parametrize("layout,counts", [("uniform", [4, 4, 4, 4]), ("ragged", [2, 4, 2])])
def test_grad_value_equals_the_unmasked_kernels_on_sanitised_exact_inputs(layout, counts, path, passes):
    for ref_dim in (2, 4):
        (v, s, pr, rf, go), levels = _exact_inputs(counts, ref_dim, 3 + ref_dim)
        B, Q, H, D = v.shape[0], pr.shape[1], v.shape[2], v.shape[3]
        cts = None if layout == "uniform" else counts
        if cts is None:
            pr = pr.reshape(B, Q, H, len(counts), counts[0], 3)
        for kind in ("bernoulli", "tail", "slice_edges", "one_real_query", "all_zeros"):
            qm = qmc.make_query_mask(kind, B, Q, 11, (B, Q, H, D, levels, max(counts))).to(DEV)
            sp, sr, sg = qmc.sanitised_fused(pr, rf, go, qm)
            for vm in (None, make_mask("bernoulli", B, levels, 11).to(DEV)):
                with options(value_path=path, ws_passes=passes):
                    want = core_run(v if vm is None else premasked(v, vm), s, sp, sr, sg, "zeros", False, cts)
                    with nothing_composed():
                        got = core_run(v, s, pr, rf, go, "zeros", False, cts, vm, qm)
                        info = _lib.last_launch_info()
                assert info["value_path"] == (1 if path == 3 else 2) and info["value_passes"] == passes, info
                gv = want[1] if vm is None else torch.where(vm[:, :, None, None], want[1], torch.zeros_like(want[1]))
                assert torch.equal(got[1], gv), (layout, ref_dim, kind, vm is not None)
                # (the real queries' rows; a sanitised query still attends — equal logits are a uniform softmax — a masked one is zeros)
                assert torch.equal(got[0][rows(got[0], qm)], want[0][rows(want[0], qm)])


# ------------------------------------------------------------------------------------------ 4 the kernels took it
@contextlib.contextmanager
def spied_symbols(log):
    """records every call of an entry point in `_lib.MODULE_MASK_SYMBOLS` (as tests/test_gpu_query_mask.py's spy)"""
    lib = _lib.load()
    real = {n: getattr(lib, n) for n in _lib.MODULE_MASK_SYMBOLS}

    def spy(n):
        def call(*a):
            log.append(n)
            return real[n](*a)
        return call

    for n in real:
        setattr(lib, n, spy(n))
    try:
        yield
    finally:
        for n in real:
            setattr(lib, n, real[n])


@pytest.mark.parametrize("layout", ["uniform", "ragged"])
def test_one_forward_and_one_backward_symbol_per_call_and_nothing_composed(layout):
    (v, s, pr, rf, go), levels, counts = _route_case(layout)
    B, Q = v.shape[0], pr.shape[1]
    fam = "fused_masked" if counts is None else "fused_ragged_masked"
    vm, qm = make_mask("rect", B, levels, 9).to(DEV), qmc.make_query_mask("tail", B, Q, 9).to(DEV)
    for masks in ((vm, None), (None, qm), (vm, qm)):
        for timed in (True, False):  # (outside a timer too: a masked call never takes the C++ node)
            log = []
            with nothing_composed(), spied_symbols(log):
                core_run(v, s, pr, rf, go, "zeros", False, counts, *masks, timed=timed)
                info = _lib.last_launch_info()
            assert log == [f"msda_fwd_{fam}_f32", f"msda_bwd_{fam}_f32"], (masks[0] is not None, masks[1] is not None, log)
            assert info["fwd_variant"] in (0, 1)
            if masks[1] is not None:
                assert info["sample_variant"] == 0, info
    # the switch: mask_in_kernels=False composes and calls none of the symbols
    log, composed = [], []
    with nothing_composed(composed), spied_symbols(log):
        off = core_run(v, s, pr, rf, go, "zeros", False, counts, vm, qm, mask_in_kernels=False)
    assert not log and composed
    on = core_run(v, s, pr, rf, go, "zeros", False, counts, vm, qm)
    assert torch.equal(on[0], off[0]) and torch.equal(on[2], off[2]) and torch.equal(on[3], off[3])
    # the launchers through ctypes agree with the Function
    if counts is None:
        out = functional.msda_hip_fwd_fused(v, s, pr, rf, "zeros", False, value_mask=vm, query_mask=qm)
        grads = functional.msda_hip_bwd_fused(go, v, s, pr, rf, "zeros", False, value_mask=vm, query_mask=qm)
    else:
        out = ragged.ragged_hip_fwd_fused(v, s, pr, rf, "zeros", False, tuple(counts), vm, qm)
        grads = ragged.ragged_hip_bwd_fused(go, v, s, pr, rf, "zeros", False, tuple(counts), value_mask=vm, query_mask=qm)
    for x, y in zip(on, (out,) + tuple(grads)):
        assert torch.equal(x, y)


@pytest.mark.parametrize("layout", ["uniform", "ragged"])
def test_a_frozen_projection_still_gets_the_masked_grad_value(layout):
    """only the pyramid requires a gradient: the backward has no grad_proj to produce and still must not compose"""
    (v, s, pr, rf, go), levels, counts = _route_case(layout)
    B, Q = v.shape[0], pr.shape[1]
    vm, qm = make_mask("rect", B, levels, 17).to(DEV), qmc.make_query_mask("tail", B, Q, 17).to(DEV)
    vp = poisoned(v, vm, float("nan"))
    full = core_run(vp, s, pr, rf, go, "zeros", False, counts, vm, qm)
    leaf = vp.detach().clone().requires_grad_(True)
    with nothing_composed():
        out = fused_module_core(leaf, s, pr, rf, "zeros", False, None, counts, vm, qm)
        out.backward(go)
    torch.cuda.synchronize()
    assert torch.equal(out.detach(), full[0])
    assert torch.isfinite(leaf.grad).all() and not leaf.grad[~vm].any()
    assert torch.equal(leaf.grad, full[1])  # (the same fused backward, its grad_proj discarded)


# ------------------------------------------------------------------------------------------ 5 storage
@pytest.mark.parametrize("layout", ["uniform", "ragged"])
@pytest.mark.parametrize("storage", ["f32_vbf16", "f32_sbf16"])
def test_storage_suffixes(layout, storage):
    (v, s, pr, rf, go), levels, counts = _route_case(layout)
    B, Q = v.shape[0], pr.shape[1]
    fam = "fused_masked" if counts is None else "fused_ragged_masked"
    v = v.to(torch.bfloat16)
    if storage == "f32_sbf16":
        pr, go = pr.to(torch.bfloat16), go.to(torch.bfloat16)
    m, qm = make_mask("rect", B, levels, 3).to(DEV), qmc.make_query_mask("tail", B, Q, 3).to(DEV)
    for lds in (0, 2):
        with options(lds_levels=lds):
            want = core_run(premasked(v, m), s, pr, rf, go, "zeros", False, counts)
            log = []
            with nothing_composed(), spied_symbols(log):
                got = core_run(poisoned(v, m, float("inf")), s, pr, rf, go, "zeros", False, counts, m)
                both = core_run(poisoned(v, m, float("inf")), s, pr, rf, go, "zeros", False, counts, m, qm)
        assert log == [f"msda_fwd_{fam}_{storage}", f"msda_bwd_{fam}_{storage}"] * 2, log
        assert got[1].dtype == torch.bfloat16
        assert_contract(got, want, m, f"{storage} lds_levels={lds}")
        assert_per_unit(both, got, qm, storage)


@pytest.mark.parametrize("layout", ["uniform", "ragged"])
def test_core_under_autocast(layout):
    """fp32 tensors under torch.autocast(bfloat16): the Functions cast to fp32 and the masked f32 pair runs — equality
    against the unmasked twin under the same autocast on the pre-masked pyramid, as for the storage suffixes"""
    (v, s, pr, rf, go), levels, counts = _route_case(layout)
    B, Q = v.shape[0], pr.shape[1]
    fam = "fused_masked" if counts is None else "fused_ragged_masked"
    m, qm = make_mask("rect", B, levels, 19).to(DEV), qmc.make_query_mask("tail", B, Q, 19).to(DEV)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        want = core_run(premasked(v, m), s, pr, rf, go, "zeros", False, counts)
        log = []
        with nothing_composed(), spied_symbols(log):
            got = core_run(poisoned(v, m, float("nan")), s, pr, rf, go, "zeros", False, counts, m)
            both = core_run(poisoned(v, m, float("nan")), s, pr, rf, go, "zeros", False, counts, m, qm)
    assert log == [f"msda_fwd_{fam}_f32", f"msda_bwd_{fam}_f32"] * 2, log
    assert_contract(got, want, m, "autocast")
    assert_per_unit(both, got, qm, "autocast")


@pytest.mark.parametrize("layout", ["uniform", "ragged"])
def test_a_forward_the_library_declines_composes(layout, monkeypatch):
    """MSDA_ERR_UNSUPPORTED from the masked forward (the launcher returns None, nothing was launched): the core composes"""
    (v, s, pr, rf, go), levels, counts = _route_case(layout)
    B, Q = v.shape[0], pr.shape[1]
    m, qm = make_mask("rect", B, levels, 23).to(DEV), qmc.make_query_mask("tail", B, Q, 23).to(DEV)
    want = core_run(v, s, pr, rf, go, "zeros", False, counts, m, qm, mask_in_kernels=False)
    mod, name = (functional, "msda_hip_fwd_fused") if counts is None else (ragged, "ragged_hip_fwd_fused")
    real = getattr(mod, name)

    def declining(*a, **kw):
        masked = kw.get("value_mask") is not None or (counts is not None and len(a) > 7 and a[7] is not None)
        return None if masked else real(*a, **kw)

    monkeypatch.setattr(mod, name, declining)
    composed, log = [], []
    with nothing_composed(composed), spied_symbols(log):
        got = core_run(v, s, pr, rf, go, "zeros", False, counts, m, qm)
    assert composed and not log
    for x, y in zip(got, want):
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------ 6 the CPU oracle
def _oracle_reference(oracle, v, s, pr, rf, go, pm, ac, counts, m):
    """the pre-masked CPU oracle behind the prologue in PyTorch -> (out, grad_value, grad_proj, grad_ref, kinks [B, Q])"""
    dt = np.float64 if v.dtype == torch.float64 else np.float32
    prc, rfc = pr.cpu().requires_grad_(True), rf.cpu().requires_grad_(True)
    sc = s.cpu()
    if counts is None:
        pts, att = module_sampling_inputs(prc, sc, rfc)
        loc_u, att_u = pts, att
    else:
        pts, att = ragged_module_sampling_inputs(prc, sc, rfc, counts)
        # per-level counts as a uniform call: every level padded to max(counts) points of weight 0 at the pyramid's centre
        B, Q, H = pts.shape[:3]
        P = max(counts)
        loc_u = torch.full((B, Q, H, len(counts), P, 2), 0.5, dtype=pts.dtype)
        att_u = torch.zeros((B, Q, H, len(counts), P), dtype=pts.dtype)
        idx, st = [], 0
        for l, p in enumerate(counts):
            idx += [(l, k, st + k) for k in range(p)]
            st += p
        lv, kk, ss = (torch.tensor(x) for x in zip(*idx))
        loc_u[:, :, :, lv, kk] = pts.detach()[:, :, :, ss]
        att_u[:, :, :, lv, kk] = att.detach()[:, :, :, ss]
    host = premasked(v.cpu(), m.cpu()).numpy().astype(dt)
    args = (host, sc.numpy().astype(np.int64), loc_u.detach().numpy().astype(dt), att_u.detach().numpy().astype(dt), pm, ac)
    out = oracle.forward(*args)
    gv, gl, ga = oracle.backward(go.cpu().numpy().astype(dt), *args)
    kink = kink_mask(args[2], args[1], ac)
    gl = np.where(kink, 0, gl)
    gl, ga = torch.from_numpy(gl).to(pts.dtype), torch.from_numpy(ga).to(pts.dtype)
    if counts is not None:
        gl, ga = gl[:, :, :, lv, kk], ga[:, :, :, lv, kk]
    g_proj, g_ref = torch.autograd.grad([pts, att], [prc, rfc], [gl, ga])
    return out, np.where(m.cpu().numpy()[:, :, None, None], gv, 0), g_proj.numpy(), g_ref.numpy(), kink.any(axis=(2, 3, 4, 5))


@pytest.mark.parametrize("ref_dim", [2, 4])
@pytest.mark.parametrize("layout,td", [("uniform", torch.float32), ("uniform", torch.float64), ("ragged", torch.float32),
                                       ("ragged", torch.float64)])
def test_against_the_premasked_cpu_oracle(oracle, layout, td, ref_dim):
    if layout == "uniform":
        B, Q, H, D, levels, P, _ = UNIFORM["c2_like_f32" if td == torch.float32 else "f64"]
        (v, s, pr, rf, go), counts = uniform_inputs(B, Q, H, D, levels, P, ref_dim, 51, td), None
    else:
        B, Q, H, D, levels = SHAPES["d32"]
        counts = COUNTS["3_6_3"]
        v, s, pr, rf, go = make(B, Q, H, D, levels, counts, ref_dim, 53, td)
        levels = levels[:3]
    m = make_mask("bernoulli", B, levels, 51).to(DEV)
    for pm, ac in PAIRS:
        with nothing_composed():
            got = [t.cpu().numpy() for t in core_run(poisoned(v, m, float("nan")), s, pr, rf, go, pm, ac, counts, m)]
        r_out, r_gv, r_gp, r_gr, kinks = _oracle_reference(oracle, v, s, pr, rf, go, pm, ac, counts, m)
        np.testing.assert_allclose(got[0], r_out, err_msg="out", **FWD_TOL[td])
        np.testing.assert_allclose(got[1], r_gv, err_msg="grad_value", **BWD_TOL[td])
        keep = ~kinks  # (a query with a sample on a lattice line: its location gradient legitimately picks either side)
        assert keep.mean() > 0.5
        np.testing.assert_allclose(got[2][keep], r_gp[keep], err_msg="grad_proj", **BWD_TOL[td])
        np.testing.assert_allclose(got[3][keep], r_gr[keep], err_msg="grad_ref", **BWD_TOL[td])


# ------------------------------------------------------------------------------------------ 7 buffers
@pytest.mark.parametrize("layout", ["uniform", "ragged"])
def test_guard_banded_launches(layout):
    (v, s, pr, rf, go), levels, counts = _route_case(layout)
    B, Q = v.shape[0], pr.shape[1]
    vm, qm = make_mask("rect", B, levels, 13).to(DEV), qmc.make_query_mask("bernoulli", B, Q, 13).to(DEV)
    vp = poisoned(v, vm, float("nan"))
    if counts is None:
        fwd = lambda: functional.msda_hip_fwd_fused(vp, s, pr, rf, "zeros", False, value_mask=vm, query_mask=qm)  # noqa: E731
        bwd = lambda: functional.msda_hip_bwd_fused(go, vp, s, pr, rf, "zeros", False, value_mask=vm, query_mask=qm)  # noqa: E731
    else:
        fwd = lambda: ragged.ragged_hip_fwd_fused(vp, s, pr, rf, "zeros", False, tuple(counts), vm, qm)  # noqa: E731
        bwd = lambda: ragged.ragged_hip_bwd_fused(go, vp, s, pr, rf, "zeros", False, tuple(counts), value_mask=vm, query_mask=qm)  # noqa: E731
    for path in (2, 3):
        with options(value_path=path):
            bad, _, _ = contract_violations(fwd, 1, DEV, names=["out"])
            assert not bad, bad
            # grad_value, grad_proj, the per-head partials, the workspace (the partials' sum is a reduction, not torch.empty)
            bad, _, _ = contract_violations(bwd, 4, DEV, names=["grad_value", "grad_proj", "grad_ref"])
            assert not bad, bad


# ------------------------------------------------------------------------------------------ 8 the nn.Module
def _module_run(mod, img, s, q, ref, vm, qm, autocast=False):
    mod.zero_grad()
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        out = mod(img, s, q, ref, value_mask=vm, query_mask=qm)
        out.float().square().sum().backward()
    torch.cuda.synchronize()
    return out.detach(), {k: p.grad.clone() for k, p in mod.named_parameters()}


@pytest.mark.parametrize("num_points", [4, [3, 6, 3]], ids=["int", "per_level"])
def test_module_hands_both_masks_to_the_kernels(num_points):
    torch.manual_seed(6)
    levels = [(12, 10), (6, 5), (3, 3)]
    mod = MultiscaleDeformableAttention(32, 32, 3, 4, num_points, "zeros", False).to(DEV)
    B, Q, I = 2, 40, sum(h * w for h, w in levels)  # noqa: E741
    s = torch.tensor(levels, device=DEV)
    img, q, ref = torch.randn(B, I, 32, device=DEV), torch.randn(B, Q, 32, device=DEV), torch.rand(B, Q, 4, device=DEV)
    vm, qm = make_mask("rect", B, levels, 6).to(DEV), qmc.make_query_mask("tail", B, Q, 6).to(DEV)
    img_p, q_p = img.clone(), q.clone()
    img_p[~vm], q_p[~qm] = float("nan"), float("nan")
    fam = "fused_masked" if isinstance(num_points, int) else "fused_ragged_masked"
    keep = msda_module.MASK_IN_KERNELS
    try:
        msda_module.MASK_IN_KERNELS = True
        log = []
        with spied_symbols(log):
            on = _module_run(mod, img, s, q, ref, vm, qm)
        assert log == [f"msda_fwd_{fam}_f32", f"msda_bwd_{fam}_f32"], log
        hostile = _module_run(mod, img_p, s, q_p, ref, vm, qm)
        log = []
        with spied_symbols(log):
            cast = _module_run(mod, img, s, q, ref, vm, qm, autocast=True)
        assert log == [f"msda_fwd_{fam}_f32_sbf16", f"msda_bwd_{fam}_f32_sbf16"], log
        hostile_cast = _module_run(mod, img_p, s, q_p, ref, vm, qm, autocast=True)
        msda_module.MASK_IN_KERNELS = False
        log, composed = [], []
        with spied_symbols(log), nothing_composed(composed):
            off = _module_run(mod, img, s, q, ref, vm, qm)
        assert not log and composed
        log, composed = [], []
        with spied_symbols(log), nothing_composed(composed):
            off_cast = _module_run(mod, img, s, q, ref, vm, qm, autocast=True)
        assert not log and composed
    finally:
        msda_module.MASK_IN_KERNELS = keep
    assert torch.equal(on[0], off[0])
    bias = mod.query_output_proj.bias.detach()
    assert torch.equal(on[0][~qm], bias.expand_as(on[0][~qm]))
    for k in on[1]:  # parameter gradients: the bounds of tests/test_gpu_fused_ragged.py's fp32 comparisons
        torch.testing.assert_close(on[1][k], off[1][k], atol=1e-3, rtol=1e-3)
    # NaN in padded pixels of `img` and in padded `queries` changes nothing.  (Except the two input projections' WEIGHT
    # gradients, which are GEMMs of the core's gradient rows with `img` / `queries` themselves: a zero row times a NaN row
    # is NaN in any implementation, the composition's included.  Their bias gradients are sums of the gradient rows.)
    assert torch.equal(hostile[0], on[0])
    for k in on[1]:
        if k not in ("img_input_proj.weight", "query_input_proj.weight"):
            assert torch.isfinite(hostile[1][k]).all() and torch.equal(hostile[1][k], on[1][k]), k
    # under autocast: the same bf16 GEMMs and the f32_sbf16 kernels on both routes — the composition's bits
    assert torch.equal(cast[0], off_cast[0]) and torch.equal(hostile_cast[0], cast[0])
    for k in cast[1]:
        torch.testing.assert_close(cast[1][k], off_cast[1][k], atol=1e-3, rtol=1e-3)
    scale = on[0].abs().max()
    torch.testing.assert_close(cast[0].float() / scale, on[0] / scale, rtol=3e-2, atol=2e-2)  # (test_module_under_autocast's)
    assert torch.equal(cast[0][~qm].float(), _module_bias_row(mod, cast[0][~qm]))


def _module_bias_row(mod, like):
    with torch.autocast("cuda", dtype=torch.bfloat16):  # the output projection of a zero row under autocast: the bias, rounded
        return mod.query_output_proj(torch.zeros(like.shape[0], mod.hidden_dim, device=like.device)).float()


@pytest.mark.parametrize("value_dtype,suffix", [(torch.bfloat16, "f32_vbf16"), (torch.float16, None)], ids=["bf16", "fp16"])
def test_module_value_dtype_routes_on_the_dtype_the_kernels_read(value_dtype, suffix):
    """`value_dtype`: the pyramid is cast after the projection, and the routing decision is taken on the cast tensor — a bf16
    pyramid goes to the mixed-storage masked pair, an fp16 one (not measured: DESIGN.md 20) composes"""
    torch.manual_seed(8)
    levels = [(12, 10), (6, 5), (3, 3)]
    mod = MultiscaleDeformableAttention(32, 32, 3, 4, 4, "zeros", False, value_dtype=value_dtype).to(DEV)
    B, Q, I = 2, 40, sum(h * w for h, w in levels)  # noqa: E741
    s = torch.tensor(levels, device=DEV)
    img, q, ref = torch.randn(B, I, 32, device=DEV), torch.randn(B, Q, 32, device=DEV), torch.rand(B, Q, 4, device=DEV)
    vm, qm = make_mask("rect", B, levels, 8).to(DEV), qmc.make_query_mask("tail", B, Q, 8).to(DEV)
    log, composed = [], []
    with spied_symbols(log), nothing_composed(composed):
        on = _module_run(mod, img, s, q, ref, vm, qm)
    if suffix is None:
        assert not log and composed
    else:
        assert log == [f"msda_fwd_fused_masked_{suffix}", f"msda_bwd_fused_masked_{suffix}"] and not composed, (log, composed)
    keep = msda_module.MASK_IN_KERNELS
    try:
        msda_module.MASK_IN_KERNELS = False
        off = _module_run(mod, img, s, q, ref, vm, qm)
    finally:
        msda_module.MASK_IN_KERNELS = keep
    assert torch.equal(on[0], off[0])
