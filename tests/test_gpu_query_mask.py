"""GPU: the query padding mask in the value-mask twins (msda_{fwd,bwd}_qmasked_<dtype>,
msda_{fwd,bwd}_fused_levelref_qmasked_<suffix>).  ``plain`` is the same call without ``query_mask`` (the _masked_ twin, or
the unmasked operator); ``sanitised`` inputs hold points 0.5, weights / logits 0 and a zero grad_out row in masked queries.

    real queries     rows of out, grad_loc, grad_attn (grad_proj, the reference-point partials) torch.equal plain's
    masked queries   rows of zeros, every one written
    grad_value       equal to plain on sanitised inputs on exactly representable inputs (tests/exact_cases.py); within
                     BWD_TOL (atol * 4, as tests/test_gpu_parity.py) of the fp64 oracle on random ones; reproducible
    containment      no bit of a masked query's inputs reaches any result"""
import contextlib
import zlib

import numpy as np
import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

import exact_cases as ec
import hostile_cases as hc
import query_mask_cases as qmc
from msda_triton_amd import _lib, functional
from msda_triton_amd.functional import KernelTimer, fused_hf_module_core, multiscale_deformable_attention
from test_gpu_fused_ragged import SHAPES as FUSED_SHAPES
from test_gpu_parity import BWD_TOL, DEV, FWD_TOL, rand_case
from test_gpu_value_mask import CASES, fused_inputs, make_mask, no_composition, options, tensors

pytestmark = pytest.mark.gpu

PAIRS = [("zeros", False), ("border", True)]  # both padding / align pairs
NAMES = ("out", "grad_value", "grad_loc", "grad_attn")


def run(v, s, l, a, go, pm, ac, vm=None, qm=None):
    v, l, a = (t.detach().clone().requires_grad_(True) for t in (v, l, a))
    out = multiscale_deformable_attention(v, s, l, a, pm, ac, value_mask=vm, query_mask=qm)
    out.backward(go)
    torch.cuda.synchronize()
    return out.detach(), v.grad, l.grad, a.grad


def fused_run(v, s, pr, rf, go, pm, ac, vm=None, qm=None, **kw):
    v, pr, rf = (t.detach().clone().requires_grad_(True) for t in (v, pr, rf))
    out = fused_hf_module_core(v, s, pr, rf, pm, ac, value_mask=vm, query_mask=qm, **kw)
    out.backward(go.to(out.dtype))
    torch.cuda.synchronize()
    return out.detach(), v.grad, pr.grad, rf.grad


def rows(t, m):
    return m.reshape(m.shape + (1,) * (t.dim() - 2)).expand_as(t)


def assert_per_unit(got, plain, qm, what):
    """everything but grad_value (index 1): real queries' rows equal plain's, masked queries' rows equal zeros"""
    for i, (g, w) in enumerate(zip(got, plain)):
        if i == 1:
            continue
        sel = rows(g, qm)
        assert torch.equal(g[sel], w[sel]), f"{what}: result {i}, real rows differ from the call without the query mask"
        assert torch.equal(g[~sel], torch.zeros_like(g[~sel])), f"{what}: result {i}, a masked row is not zeros"


def sanitise(l, a, go, qm, fill=0.5):
    return (torch.where(rows(l, qm), l, torch.full_like(l, fill)), torch.where(rows(a, qm), a, torch.zeros_like(a)),
            torch.where(rows(go, qm), go, torch.zeros_like(go)))


def shape_of(name):
    B, Q, H, D, levels, P, td = CASES[name]
    return (B, Q, H, D, levels, P, torch.empty((), dtype=td).element_size())


# ------------------------------------------------------------------------------------------ 1 per-unit results
@pytest.mark.parametrize("kind", qmc.KINDS)
@pytest.mark.parametrize("name", list(CASES))
def test_real_rows_equal_the_plain_call_and_masked_rows_are_zeros(name, kind):
    B, Q, H, D, levels, P, td = CASES[name]
    seed = zlib.crc32(f"q{name}{kind}".encode())
    c = rand_case(np.random.default_rng(seed), B, Q, H, D, levels, P, dtype=np.float64 if td == torch.float64 else np.float32)
    v, l, a, go, s = tensors(c, td)
    qm = qmc.make_query_mask(kind, B, Q, seed, shape_of(name)).to(DEV)
    for vm in (None, make_mask("rect", B, levels, seed).to(DEV)):
        for pm, ac in PAIRS:
            for lds in (0, 2):  # memory-served and LDS-served levels
                with options(unit_fwd=0, lds_levels=lds):
                    plain = run(v, s, l, a, go, pm, ac, vm)
                    with no_composition():
                        got = run(v, s, l, a, go, pm, ac, vm, qm)
                what = f"{name} {kind} {pm}/{ac} lds_levels={lds} value_mask={'rect' if vm is not None else None}"
                assert_per_unit(got, plain, qm, what)
                if kind == "all_ones":  # ... and grad_value too: nothing was dropped
                    assert torch.equal(got[1], plain[1]), what
                if kind == "all_zeros":  # an all-masked plane: empty lists, a zero grad_value
                    assert torch.equal(got[1], torch.zeros_like(got[1])), what


@pytest.mark.parametrize("kind", qmc.KINDS)
@pytest.mark.parametrize("ref_dim", [2, 4])
@pytest.mark.parametrize("name", ["d32", "d5", "d64"])
def test_fused_pair_real_rows_equal_the_plain_call_and_masked_rows_are_zeros(name, ref_dim, kind):
    B, Q, H, D, levels = FUSED_SHAPES[name]
    P = 4
    seed = zlib.crc32(f"qf{name}{ref_dim}{kind}".encode())
    v, s, pr, rf, go = fused_inputs(B, Q, H, D, levels, P, ref_dim, seed)
    qm = qmc.make_query_mask(kind, B, Q, seed, (B, Q, H, D, levels, P)).to(DEV)
    for vm in (None, make_mask("rect", B, levels, seed).to(DEV)):
        for pm, ac in PAIRS:
            for lds in (0, 2):
                with options(lds_levels=lds):
                    plain = fused_run(v, s, pr, rf, go, pm, ac, vm, mask_in_kernels=True)
                    with no_composition():
                        got = fused_run(v, s, pr, rf, go, pm, ac, vm, qm)
                what = f"fused {name} ref_dim {ref_dim} {kind} {pm}/{ac} lds_levels={lds}"
                # (grad_ref is the partials summed over the heads by one torch call in both runs: rows of zeros stay zeros)
                assert_per_unit(got, plain, qm, what)
                if kind == "all_ones":
                    assert torch.equal(got[1], plain[1]), what
                if kind == "all_zeros":
                    assert torch.equal(got[1], torch.zeros_like(got[1])), what


# ------------------------------------------------------------------------------------------ 2 grad_value, exact
ROUTES = [(n, 2, 1) for n in qmc.EXACT] + [(n, 2, 2) for n in ("d32_vec_g8", "b4_passes", "flood")] + \
         [(n, 3, 1) for n in ("d32_vec_g8", "d5_scalar", "d8_vec_g4", "lds_q200", "b4_passes")]


@pytest.mark.parametrize("rig", [0, 1], ids=["records_in_workspace", "records_in_grads"])
@pytest.mark.parametrize("name,path,passes", ROUTES,
                         ids=[f"{n}-{'single_launch' if p == 3 else 'sorted'}{'_two_passes' if k == 2 else ''}" for n, p, k in ROUTES])
def test_grad_value_is_exact_on_exactly_representable_inputs(name, path, passes, rig):
    """tests/exact_cases.py's generators with the mask laid over them: equal to plain on the sanitised inputs AND to the fp64
    oracle (tests/test_query_mask.py shows that the sums stay exactly representable under the mask)"""
    c = ec.get_case(name)
    B, Q, H, D, levels, P = ec.CASES[name][1]
    v, l, a, go, s = tensors(c, torch.float32)
    for kind in ("bernoulli", "tail", "slice_edges", "one_real_query", "all_zeros"):
        qm_h = qmc.exact_query_mask(name, kind)
        qm = qm_h.to(DEV)
        sl, sa, sgo = sanitise(l, a, go, qm)
        for pm, ac in PAIRS:
            _, ref = qmc.exact_reference(name, pm, ac, qm_h.numpy())
            with options(unit_fwd=0, value_path=path, ws_passes=passes, records_in_grads=rig):
                want = run(v, s, sl, sa, sgo, pm, ac)
                got = run(v, s, l, a, go, pm, ac, None, qm)
                info = _lib.last_launch_info()
            what = f"{name} {kind} {pm}/{ac}"
            assert info["value_path"] == (1 if path == 3 else 2) and info["value_passes"] == passes, (what, info)
            assert torch.equal(got[1], want[1]), f"{what}: grad_value differs from the plain call on the sanitised inputs"
            for i, k in enumerate(NAMES):
                assert torch.equal(got[i].double().cpu(), torch.from_numpy(ref[k])), f"{what}: {k} differs from the fp64 oracle"


# ------------------------------------------------------------------------------------------ 3 grad_value, random
# (16-bit storage has no oracle tolerance in tests/test_gpu_parity.py's tables: those shapes are held by the equality tests)
@pytest.mark.parametrize("name", [n for n in CASES if CASES[n][6] in BWD_TOL])
def test_grad_value_on_random_inputs_against_the_oracle_and_reproducible(oracle, name):
    B, Q, H, D, levels, P, td = CASES[name]
    seed = zlib.crc32(f"qr{name}".encode())
    c = rand_case(np.random.default_rng(seed), B, Q, H, D, levels, P, dtype=np.float64 if td == torch.float64 else np.float32)
    v, l, a, go, s = tensors(c, td)
    tol = dict(BWD_TOL[td], atol=BWD_TOL[td]["atol"] * 4)
    for kind in ("bernoulli", "tail", "slice_edges"):
        qm_h = qmc.make_query_mask(kind, B, Q, seed, shape_of(name))
        qm = qm_h.to(DEV)
        sc = qmc.sanitised(c, qm_h.numpy())
        for path in (2, 3):
            with options(unit_fwd=0, value_path=path):
                got = run(v, s, l, a, go, "zeros", False, None, qm)
                again = run(v, s, l, a, go, "zeros", False, None, qm)
            for x, y in zip(got, again):
                assert torch.equal(x, y), (name, kind, path)
            r_gv, _, r_ga = oracle.backward(sc["grad_out"], sc["value"], sc["shapes"], sc["loc"], sc["attn"], "zeros", False)
            print(f"{name} {kind} path {path}: grad_value max abs err {np.abs(got[1].cpu().numpy() - r_gv).max():.3e}")
            np.testing.assert_allclose(got[1].cpu().numpy(), r_gv, err_msg="grad_value", **tol)
            np.testing.assert_allclose(got[3].cpu().numpy(), r_ga, err_msg="grad_attn", **tol)
            r_out = oracle.forward(sc["value"], sc["shapes"], sc["loc"], sc["attn"], "zeros", False)
            np.testing.assert_allclose(got[0].cpu().numpy(), r_out, err_msg="out", **FWD_TOL[td])


# ------------------------------------------------------------------------------------------ 4 containment
HOSTILE = (float("nan"), float("inf"), 1e30)


@pytest.mark.parametrize("name", list(hc.plain_shapes()))
def test_nothing_a_masked_query_holds_reaches_a_result(name):
    """tests/hostile_cases.py's inputs; NaN, +Inf and 1e30 in the masked queries' points, weights and grad_out rows"""
    c, _, td = hc.plain_case(name)
    B, Q, H, D, levels, P, _ = hc.plain_shapes()[name]
    v, l, a, go, s = tensors(c, td)
    seed = hc.seed_of("qmask", name)
    for kind in ("bernoulli", "tail", "slice_edges"):
        qm = qmc.make_query_mask(kind, B, Q, seed, (B, Q, H, D, levels, P, v.element_size())).to(DEV)
        bad = [qmc.hostile_fill(t, qm, HOSTILE) for t in (l, a, go)]
        for vm in (None, make_mask("rect", B, levels, seed).to(DEV)):
            for path, rig in ((2, 0), (2, 1), (3, 0)):
                with options(unit_fwd=0, value_path=path, records_in_grads=rig):
                    benign = run(v, s, l, a, go, "zeros", False, vm, qm)
                    for which in ((0,), (1,), (2,), (0, 1, 2)):
                        l2, a2, g2 = (bad[i] if i in which else t for i, t in enumerate((l, a, go)))
                        got = run(v, s, l2, a2, g2, "zeros", False, vm, qm)
                        for k, x, y in zip(NAMES, got, benign):
                            assert torch.isfinite(x.float()).all() and torch.equal(x, y), (name, kind, path, rig, which, k)


@pytest.mark.parametrize("ref_dim", [2, 4])
def test_fused_pair_contains_the_masked_queries_inputs(ref_dim):
    B, Q, H, D, levels = FUSED_SHAPES["d32"]
    v, s, pr, rf, go = fused_inputs(B, Q, H, D, levels, 4, ref_dim, 77 + ref_dim)
    for kind in ("bernoulli", "tail"):
        qm = qmc.make_query_mask(kind, B, Q, 5, (B, Q, H, D, levels, 4)).to(DEV)
        vm = make_mask("rect", B, levels, 5).to(DEV)
        for lds in (0, 2):
            with options(lds_levels=lds):
                benign = fused_run(v, s, pr, rf, go, "zeros", False, vm, qm)
                for which in ((0,), (1,), (2,), (0, 1, 2)):
                    p2, r2, g2 = (qmc.hostile_fill(t, qm, HOSTILE) if i in which else t for i, t in enumerate((pr, rf, go)))
                    got = fused_run(v, s, p2, r2, g2, "zeros", False, vm, qm)
                    for x, y in zip(got, benign):
                        assert torch.isfinite(x).all() and torch.equal(x, y), (kind, lds, which)


# ------------------------------------------------------------------------------------------ 5 the kernels took it
class _NoSelectionOps(TorchDispatchMode):
    """fails on the ops a composition of the mask would run: where / masked_fill / index*"""
    BANNED = ("where", "masked_fill", "index", "index_put", "index_select", "masked_scatter", "masked_select")

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        name = func.overloadpacket.__name__
        if name in self.BANNED:
            raise AssertionError(f"{name} ran: the query mask was composed instead of going into the kernels")
        return func(*args, **(kwargs or {}))


@contextlib.contextmanager
def spied_symbols(log):
    """records every call of a `_qmasked_` / `_masked_` entry point of the loaded library"""
    lib = _lib.load()
    names = [n for n in _lib.EXPORTED_SYMBOLS + _lib.QUERY_MASK_SYMBOLS if "masked_" in n]
    real = {n: getattr(lib, n) for n in names}

    def spy(n):
        def call(*a):
            log.append(n)
            return real[n](*a)
        return call

    for n in names:
        setattr(lib, n, spy(n))
    try:
        yield
    finally:
        for n in names:
            setattr(lib, n, real[n])


def test_the_qmasked_symbols_run_and_nothing_is_composed():
    B, Q, H, D, levels, P, td = CASES["c2_like_f32"]
    c = rand_case(np.random.default_rng(9), B, Q, H, D, levels, P)
    v, l, a, go, s = tensors(c, td)
    qm = qmc.make_query_mask("tail", B, Q, 9).to(DEV)
    vm = make_mask("rect", B, levels, 9).to(DEV)
    for mask in (None, vm):
        log = []
        with options(unit_fwd=0), no_composition(), spied_symbols(log), _NoSelectionOps(), KernelTimer() as kt:
            run(v, s, l, a, go, "zeros", False, mask, qm)
        assert log == ["msda_fwd_qmasked_f32", "msda_bwd_qmasked_f32", "msda_bwd_qmasked_f32"], log  # (timed: two backward calls)
        assert [r[0] for r in kt.records] == ["msda_fwd_qmasked", "msda_bwd_qmasked_sample", "msda_bwd_qmasked_value"]
    Bf, Qf, Hf, Df, lv = FUSED_SHAPES["d32"]
    fv, fs, pr, rf, fgo = fused_inputs(Bf, Qf, Hf, Df, lv, 4, 2, 9)
    fq = qmc.make_query_mask("bernoulli", Bf, Qf, 9).to(DEV)
    for dt in (torch.float32, torch.bfloat16):  # the plain fused pair and the module-storage one (16-bit value and projection)
        log = []
        with no_composition(), spied_symbols(log), _NoSelectionOps():
            fused_run(fv.to(dt), fs, pr.to(dt), rf, fgo.to(dt), "zeros", False, None, fq)
        suf = "f32" if dt == torch.float32 else "f32_sbf16"
        assert log == [f"msda_fwd_fused_levelref_qmasked_{suf}", f"msda_bwd_fused_levelref_qmasked_{suf}"], log
    # mixed storage and autocast take the entry points as well
    log = []
    with options(unit_fwd=0), spied_symbols(log), _NoSelectionOps():
        run(v.to(torch.bfloat16), s, l, a, go, "zeros", False, None, qm)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            run(v, s, l, a, go, "zeros", False, None, qm)
    assert log == ["msda_fwd_qmasked_f32_vbf16", "msda_bwd_qmasked_f32_vbf16", "msda_fwd_qmasked_f32", "msda_bwd_qmasked_f32"], log


# ------------------------------------------------------------------------------------------ 6 ctypes
def test_ctypes_calls_agree_with_the_function_and_null_masks_are_bad_arguments():
    B, Q, H, D, levels, P, td = CASES["c2_like_f32"]
    c = rand_case(np.random.default_rng(21), B, Q, H, D, levels, P)
    v, l, a, go, s = tensors(c, td)
    qm = qmc.make_query_mask("bernoulli", B, Q, 21).to(DEV)
    vm = make_mask("rect", B, levels, 21).to(DEV)
    ones_q = torch.ones_like(qm)
    with options(unit_fwd=0):
        got = run(v, s, l, a, go, "zeros", False, vm, qm)
        out = functional.msda_hip_fwd(v, s, l, a, "zeros", False, value_mask=vm, query_mask=qm)
        grads = functional.msda_hip_bwd(go, v, s, l, a, "zeros", False, value_mask=vm, query_mask=qm)
        for x, y in zip(got, (out,) + tuple(grads)):
            assert torch.equal(x, y)
        # the _masked_ entry points still give their bits: the _qmasked_ call with an all-ones query mask is the same
        masked = run(v, s, l, a, go, "zeros", False, vm)
        allones = run(v, s, l, a, go, "zeros", False, vm, ones_q)
    for k, x, y in zip(NAMES, masked, allones):
        assert torch.equal(x, y), k
    Bf, Qf, Hf, Df, lv = FUSED_SHAPES["d32"]
    fv, fs, pr, rf, fgo = fused_inputs(Bf, Qf, Hf, Df, lv, 4, 4, 22)
    fq = qmc.make_query_mask("bernoulli", Bf, Qf, 22).to(DEV)
    fm = make_mask("rect", Bf, lv, 22).to(DEV)
    got = fused_run(fv, fs, pr, rf, fgo, "zeros", False, fm, fq)
    out = functional.msda_hip_fwd_fused(fv, fs, pr, rf, "zeros", False, levelref=True, value_mask=fm, query_mask=fq)
    g_img, g_proj, g_ref = functional.msda_hip_bwd_fused(fgo, fv, fs, pr, rf, "zeros", False, levelref=True, value_mask=fm, query_mask=fq)
    for x, y in zip(got, (out, g_img, g_proj, g_ref)):
        assert torch.equal(x, y)
    # a NULL in either mask: MSDA_ERR_BAD_ARG, nothing launched (real device buffers behind every other argument)
    lib = _lib.load()
    u8v, u8q = functional.check_value_mask(vm, v), functional.check_query_mask(qm, l)
    sh = functional._shapes_i64(s)
    o = torch.empty(B, Q, H, D, device=DEV)
    for vp_, qp_ in ((None, u8q.data_ptr()), (u8v.data_ptr(), None)):
        rc = lib.msda_fwd_qmasked_f32(v.data_ptr(), vp_, qp_, sh.data_ptr(), l.data_ptr(), a.data_ptr(), o.data_ptr(), B, v.shape[1], H, D,
                                      Q, len(levels), P, 0, 0, 0, None)
        assert rc == -1, rc
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ 7 guard-banded buffers
def test_guard_banded_buffers_every_row_is_written():
    from guarded_alloc import contract_violations
    B, Q, H, D, levels, P, td = CASES["c2_like_f32"]
    c = rand_case(np.random.default_rng(31), B, Q, H, D, levels, P)
    v, l, a, go, s = tensors(c, td)
    qm = qmc.make_query_mask("slice_edges", B, Q, 31, shape_of("c2_like_f32")).to(DEV)
    vm = make_mask("rect", B, levels, 31).to(DEV)
    bad_l, bad_a, bad_go = (qmc.hostile_fill(t, qm, HOSTILE) for t in (l, a, go))  # (a masked row that is skipped keeps the pre-fill)
    for lds in (0, 2):
        for path in (2, 3):
            with options(unit_fwd=0, lds_levels=lds, value_path=path):
                bad, _, res = contract_violations(lambda: functional.msda_hip_fwd(v, s, bad_l, bad_a, "zeros", False, value_mask=vm, query_mask=qm),
                                                  1, DEV, names=["out"])
                assert not bad, bad
                assert torch.equal(res[1][0][~qm], torch.zeros_like(res[1][0][~qm]))
                bad, _, res = contract_violations(
                    lambda: functional.msda_hip_bwd(bad_go, v, s, bad_l, bad_a, "zeros", False, value_mask=vm, query_mask=qm), 4, DEV,
                    names=["grad_value", "grad_loc", "grad_attn"])
                assert not bad, bad
                for t in res[1][1:]:
                    assert torch.equal(t[~qm], torch.zeros_like(t[~qm]))
    Bf, Qf, Hf, Df, lv = FUSED_SHAPES["d32"]
    fv, fs, pr, rf, fgo = fused_inputs(Bf, Qf, Hf, Df, lv, 4, 4, 32)
    fq = qmc.make_query_mask("bernoulli", Bf, Qf, 32).to(DEV)
    fm = make_mask("rect", Bf, lv, 32).to(DEV)
    bp, br, bg = (qmc.hostile_fill(t, fq, HOSTILE) for t in (pr, rf, fgo))
    for lds in (0, 2):
        with options(lds_levels=lds):
            bad, _, _ = contract_violations(lambda: functional.msda_hip_fwd_fused(fv, fs, bp, br, "zeros", False, levelref=True, value_mask=fm,
                                                                                  query_mask=fq), 1, DEV, names=["out"])
            assert not bad, bad
            bad, _, res = contract_violations(lambda: functional.msda_hip_bwd_fused(bg, fv, fs, bp, br, "zeros", False, levelref=True,
                                                                                    value_mask=fm, query_mask=fq), 4, DEV,
                                              names=["grad_value", "grad_proj", "grad_ref"])
            assert not bad, bad
            assert torch.equal(res[1][1][~fq], torch.zeros_like(res[1][1][~fq]))


# ------------------------------------------------------------------------------------------ 8 the adapter
def test_deformable_detr_with_skip_padded_queries():
    """The tiny Deformable-DETR of tests/test_hf_model.py, B 2 with the second image padded: skip_padded_queries=True against
    False at that file's GPU bounds for the same model (outputs atol 1e-4 / rtol 1e-3, gradients 2e-3 relative L2)."""
    pytest.importorskip("transformers")
    from msda_triton_amd import hf_adapter
    from test_hf_model import WATCHED, _inputs, run_model, tiny_deformable_detr
    x, mask = _inputs(DEV)
    assert not mask[1].all()
    model = tiny_deformable_detr().to(DEV)
    assert hf_adapter.replace_hf_msda(model, skip_padded_queries=True) == 4  # the flag without fused=True: no effect, same count
    assert not any(getattr(m, "skip_padded_queries", False) for m in model.modules())
    assert hf_adapter.replace_hf_msda(model, fused=True) == 4                # the default: off
    fused = [m for m in model.modules() if isinstance(m, hf_adapter.FusedHFDeformableAttention)]
    assert len(fused) == 4 and not any(m.skip_padded_queries for m in fused)
    hs0, enc0, g0 = run_model(model, x, mask)
    assert hf_adapter.replace_hf_msda(model, fused=True, skip_padded_queries=True) == 0  # nothing left to wrap; the flag is set
    assert all(m.skip_padded_queries for m in fused)
    log, seen = [], []
    hook = fused[0].register_forward_pre_hook(lambda mod, args, kwargs: seen.append(kwargs.get("attention_mask")), with_kwargs=True)
    with spied_symbols(log):
        hs1, enc1, g1 = run_model(model, x, mask)
        torch.cuda.synchronize()
    hook.remove()
    # the two encoder layers took the query-mask entry points, the two decoder cross-attentions (Q = 30 object queries) did not
    assert sum("fused_levelref_qmasked" in n for n in log) == 4 and sum("fused_levelref_masked" in n for n in log) == 4, log
    valid = seen[0].bool()
    torch.testing.assert_close(hs1, hs0, atol=1e-4, rtol=1e-3)
    torch.testing.assert_close(enc1[valid], enc0[valid], atol=1e-4, rtol=1e-3)
    for k in WATCHED:
        err = float((g1[k] - g0[k]).norm() / g0[k].norm().clamp_min(1e-30))
        assert err < 2e-3, (k, err)
    print("skip_padded_queries: decoder states bit-equal:", torch.equal(hs1, hs0), "valid encoder rows bit-equal:",
          torch.equal(enc1[valid], enc0[valid]))
