"""CPU: the derived error bound of tests/error_bound_cases.py is RIGHT — independent float32 evaluations (the C oracle, torch
compositions of the prologues) stay inside it on every fixture, mode, tensor and element, and its fp64 values agree with
the existing fp64 references — and it has TEETH: each emulated wrong kernel below leaves it in at least one element.

The largest error / bound of every float32 evaluation is printed per tensor.  Where it exceeds 0.5 the bound is nearly
sharp, and legitimately so:
  * grad_value and `out` under align_corners (up to ~0.8): the coordinate is ONE rounded multiply, x * (W - 1), whose bound
    U |x| (W - 1) is attained up to a factor below 2, and an element fed by a single sample with a steep bilinear slope is
    dominated by that one term — the oracle and the kernels form the same product, so they share it;
  * discrete grad_value (up to 0.995): an element with one sample is the single product a * g, bound U |a g|, attained when
    the product falls next to a rounding boundary;
  * 16-bit storage (up to 1.0): the bound is then dominated by r, half a unit of the storage type, which round-to-nearest
    attains.
The kernels use other summation orders than these references; the sum rule covers every order, so none of that is fitted.

Mutants the worst-case bound cannot see are listed in NOT_DETECTABLE with their measured ratios."""
import numpy as np
import pytest
import torch

import error_bound_cases as eb
import exact_cases as ec
from error_bound_cases import BF16, F16, F32, MODES

MODE_IDS = [f"{pm}_{int(ac)}" for pm, ac in MODES]
PLAIN_STORAGE = {"d32": list(eb.STORAGE), "d5": list(eb.STORAGE), "d64": list(eb.STORAGE), "counts": ["f32", "bf16"],
                 "long_sum": ["f32", "bf16", "f32_vbf16"], "range": ["f32", "bf16", "f32_vbf16"], "range_h": ["fp16", "f32_vf16"]}
RUNS = [(n, s) for n, ss in PLAIN_STORAGE.items() for s in ss]


def _stored(res, storage):
    vdt, cdt = eb.STORAGE[storage]
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(vdt if k == "grad_value" else cdt) for k, v in res.items()}


def _report(what, res):
    print(f"{what}: " + ", ".join(f"{k} {r:.3f}" for k, (_, r) in res.items()))
    assert all(n == 0 and r <= 1.0 for n, r in res.values()), (what, res)


# ----------------------------------------------------------------------------------------- the evaluator itself
def test_evaluator_rules():
    a, b = eb.Ev(3.0, 0.5), eb.Ev(-2.0, 0.25)
    u = eb.U
    assert (a + b).err == 0.75 + u * 1.0 and (a - b).err == 0.75 + u * 5.0
    assert (a * b).err == 3.0 * 0.25 + 2.0 * 0.5 + u * 6.0
    assert np.isclose((a / b).err, 0.5 / 2.0 + 1.5 * 0.25 / 2.0 + u * 1.5)
    s = eb.Ev(np.array([1.0, -2.0, 4.0]), np.array([0.1, 0.2, 0.3])).sum(0)
    assert s.val == 3.0 and np.isclose(s.err, 0.6 + 2 * u * 7.0)
    e = eb.ev_exp(eb.Ev(1.0, 0.01))
    assert np.isclose(e.err, np.e * (0.01 + eb.EXP_C * u))
    with pytest.raises(AssertionError):
        eb.Ev(np.ones(2 ** 15)).sum(0)  # n * U > 2^-10: the second-order factor would not cover it


def test_half_spacing_in_the_normal_and_subnormal_range():
    m = np.array([0.0, 2.0 ** -20, 2.0 ** -14, 1.0, 1.999, 2.0, 1000.0])
    assert np.array_equal(eb.half_spacing(m, F16), [2.0 ** -25, 2.0 ** -25, 2.0 ** -25, 2.0 ** -11, 2.0 ** -11, 2.0 ** -10, 0.25])
    assert np.array_equal(eb.half_spacing(m[3:], BF16), [2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0])
    assert not eb.half_spacing(m, F32).any()


# ----------------------------------------------------------------------------------------- plain operator
@pytest.mark.parametrize("pm,ac", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name,storage", RUNS)
def test_plain_formulas_agree_with_the_oracle_and_bound_its_float32_run(name, storage, pm, ac):
    c = eb.get_case(name, storage)
    o = ec._oracle()
    ref = ec._oracle_all(o, c, pm, ac, np.float64)
    cond = ec.condition_sums(c, pm, ac)
    f32 = _stored(ec._oracle_all(o, c, pm, ac, np.float32), storage)
    for records in ("float", "q20"):
        form, keep = eb.plain_reference(name, storage, pm, ac, records)
        for k, r in ref.items():
            assert np.abs(form[k].val - r).max() <= 1e-12 * cond[k], (k, records)
            top = np.abs(form[k].val) + form[k].err
            vdt, cdt = eb.STORAGE[storage]
            dt = vdt if k == "grad_value" else cdt
            assert dt == F32 or top.max() < 0.5 * torch.finfo(dt).max, (k, float(top.max()))
        _report(f"{name} {storage} {pm} {int(ac)} {records}", eb.ratios(f32, form, keep))
    assert eb.excluded_share(c, ac) <= eb.MAX_EXCLUDED


def test_range_fixture_reaches_fp16_subnormals():
    form, _ = eb.plain_reference("range_h", "fp16", "zeros", False)
    v = np.abs(form["grad_value"].val)
    assert ((v > 0) & (v < 2.0 ** -14)).sum() >= 10


@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_discrete_formulas(storage):
    c = eb.get_case("discrete", storage)
    form, keep, near = eb.discrete_reference("discrete", storage)
    ref = ec._discrete_all(c, ec._ref_discrete, ec.F64)
    for k, r in ref.items():
        assert np.abs(form[k].val - r).max() <= 1e-12 * max(np.abs(r).max(), 1.0), k
    f32 = ec._discrete_all(c, ec._index_discrete, F32)
    vdt, cdt = eb.STORAGE[storage]
    got = {k: torch.from_numpy(v).to(vdt if k == "grad_value" else cdt) for k, v in f32.items()}
    _report(f"discrete {storage}", eb.ratios(got, form, keep))
    assert near.mean() <= eb.MAX_EXCLUDED, near.mean()


# ----------------------------------------------------------------------------------------- fused families
@pytest.mark.parametrize("storage", list(eb.FUSED_STORAGE))
@pytest.mark.parametrize("name", list(eb.FUSED))
def test_fused_formulas_agree_with_autograd_and_bound_a_float32_composition(name, storage):
    fc = eb.fused_case(name, storage)
    sdt, rdt = eb.FUSED_STORAGE[storage]
    for pm, ac in (MODES if name != "hfbox_discrete" else [("border", False)]):
        form, keep, kink = eb.fused_reference(name, storage, pm, ac)
        r64 = eb.fused_torch(fc, name, pm, ac, torch.float64)
        assert set(r64) == set(form)
        for k, r in r64.items():
            assert np.abs(form[k].val - r.numpy()).max() <= 1e-12 * max(float(r.abs().max()), 1.0), (name, pm, ac, k)
        r32 = eb.fused_torch(fc, name, pm, ac, torch.float32)
        got = {k: v.to(rdt if k == "grad_ref" else sdt) for k, v in r32.items()}
        _report(f"{name} {storage} {pm} {int(ac)}", eb.ratios(got, form, keep))
        assert kink.mean() <= eb.MAX_EXCLUDED, (name, pm, ac, kink.mean())


# ----------------------------------------------------------------------------------------- emulated wrong kernels
def _hits(got, form, keep):
    res = eb.ratios(got, form, keep)
    return sum(n for n, _ in res.values()), max(r for _, r in res.values())


def _plain_out_mutant(fn, storage="f32", names=("d32", "d5")):
    """A mutant of `out`: fn(case, pm, ac) -> fp64 out; stored in the case's type."""
    worst = (0, 0.0)
    for name in names:
        c = eb.get_case(name, storage)
        for pm, ac in MODES:
            form, keep = eb.plain_reference(name, storage, pm, ac)
            got = _stored(dict(out=fn(c, pm, ac)), storage)
            n, r = _hits(got, dict(out=form["out"]), keep)
            worst = (worst[0] + n, max(worst[1], r))
    return worst


def _record_bits(bits):
    def run():
        worst = (0, 0.0)
        for name in ("d32", "long_sum"):
            c = eb.get_case(name)
            for pm, ac in MODES:
                form, keep = eb.plain_reference(name, "f32", pm, ac, "q20")
                got = dict(grad_value=eb.emulated_grad_value(c, pm, ac, eb.quantised(bits)))
                n, r = _hits(got, dict(grad_value=form["grad_value"]), keep)
                worst = (worst[0] + n, max(worst[1], r))
        return worst
    return run


def _weights_in(dtype):
    return lambda: _plain_out_mutant(lambda c, pm, ac: ec.contributions(c, pm, ac, weight_fn=eb.rounded_to(dtype)).sum((3, 4)))


def _coordinate_in_fp16():
    return _plain_out_mutant(lambda c, pm, ac: eb.out_from_taps(c, pm, ac, eb.rounded_to(F16)(ec.pixel_coordinates(c, ac))))


def _accumulate_in(dtype, storage):
    rnd = eb.rounded_to(dtype)

    def fn(c, pm, ac):
        t = ec.contributions(c, pm, ac)
        t = t.reshape(t.shape[:3] + (-1, t.shape[-1]))
        acc = np.zeros(t.shape[:3] + t.shape[-1:])
        for s in range(t.shape[3]):
            acc = rnd(acc + t[:, :, :, s])
        return acc
    return lambda: _plain_out_mutant(fn, storage)


def _second_rounding(dtype, storage):
    rnd = eb.rounded_to(dtype)
    return lambda: _plain_out_mutant(lambda c, pm, ac: rnd(ec.contributions(c, pm, ac).sum(4)).sum(3), storage)


def _truncation(dtype, storage):
    def run():
        worst = (0, 0.0)
        for pm, ac in MODES:
            form, keep = eb.plain_reference("d32", storage, pm, ac)
            vdt, cdt = eb.STORAGE[storage]
            got = {k: ec.truncate(torch.from_numpy(e.val).float(), dtype) if (vdt if k == "grad_value" else cdt) == dtype
                   else torch.from_numpy(e.val).float() for k, e in form.items()}
            n, r = _hits(got, form, keep)
            worst = (worst[0] + n, max(worst[1], r))
        return worst
    return run


def _fused_out_with(name, pm, ac, attn=None, pro=None, fc=None):
    """`out` of a fused family in fp64 with a mutant's attention weights or points behind the right prologue's rest."""
    fc = eb.fused_case(name) if fc is None else fc
    good = eb.prologue(fc, name)
    c = eb.fused_operator_case(fc, good if pro is None else pro)
    if attn is not None:
        c = dict(c, attn=attn)
    form, keep, _ = eb.fused_formulas(fc, name, pm, ac, pro=good)
    t = ec.contributions(c, pm, ac)
    out = t.sum((3, 4)) if t.ndim == 6 else t.sum(3)
    return _hits(dict(out=out), dict(out=form["out"]), keep)


def _exp_with_relative_error():
    """every exp off by a factor 1 +- 2^-16 (a table-driven or half-precision exp)"""
    worst = (0, 0.0)
    for name in ("module2", "hfbox"):
        fc = eb.fused_case(name)
        z = fc["proj"][..., 2]
        zf = z.reshape(z.shape[:3] + (-1,))
        sign = np.where(np.random.default_rng(5).random(zf.shape) < 0.5, -1.0, 1.0)
        e = np.exp(zf - zf.max(-1, keepdims=True)) * (1 + sign * 2.0 ** -16)
        a = (e / e.sum(-1, keepdims=True)).reshape(z.shape)
        for pm, ac in MODES:
            n, r = _fused_out_with(name, pm, ac, attn=a)
            worst = (worst[0] + n, max(worst[1], r))
    return worst


def _softmax_without_max():
    """exp(z) / sum exp(z) in float32 on logits around 60 (no overflow yet: exp(64) < 3.4e38)"""
    worst = (0, 0.0)
    for name in ("module2", "hfbox"):
        fc = dict(eb.fused_case(name))
        proj = np.array(fc["proj"])
        proj[..., 2] = eb.rounded_to(F32)(proj[..., 2] + 60.0)
        fc["proj"] = proj
        z = proj[..., 2]
        zf = z.reshape(z.shape[:3] + (-1,)).astype(np.float32)
        e = np.exp(zf)
        a = (e * (np.float32(1) / e.sum(-1, keepdims=True, dtype=np.float32))).astype(np.float64).reshape(z.shape)
        for pm, ac in MODES:
            n, r = _fused_out_with(name, pm, ac, attn=a, fc=fc)
            worst = (worst[0] + n, max(worst[1], r))
    return worst


def _level_scale_in_bf16():
    """the box rule's float32(1 / P_l) rounded to bf16: 1 / 3 moves by 2^-10 relative"""
    worst = (0, 0.0)
    fc = eb.fused_case("hfbox")
    bad = eb.prologue(fc, "hfbox", scale_fn=lambda s: torch.from_numpy(s).to(BF16).float().numpy())
    for pm, ac in MODES:
        n, r = _fused_out_with("hfbox", pm, ac, pro=bad)
        worst = (worst[0] + n, max(worst[1], r))
    return worst


MUTANTS = {
    "record fractions of 16 bits": _record_bits(16),
    "record fractions of 12 bits": _record_bits(12),
    "corner weights rounded to fp16": _weights_in(F16),
    "corner weights rounded to bf16": _weights_in(BF16),
    "pixel coordinate formed in fp16": _coordinate_in_fp16,
    "fp16 accumulation, fp16 storage": _accumulate_in(F16, "fp16"),
    "bf16 accumulation, bf16 storage": _accumulate_in(BF16, "bf16"),
    "per-level partial sums rounded to bf16 before the final sum": _second_rounding(BF16, "bf16"),
    "per-level partial sums rounded to fp16 before the final sum": _second_rounding(F16, "fp16"),
    "truncation on store, bf16": _truncation(BF16, "bf16"),
    "truncation on store, fp16": _truncation(F16, "fp16"),
    "truncation on store of grad_value, f32_vbf16": _truncation(BF16, "f32_vbf16"),
    "exp with relative error 2^-16": _exp_with_relative_error,
    "softmax without the subtracted max, logits around 60": _softmax_without_max,
    "1 / P_l rounded to bf16": _level_scale_in_bf16,
}
# name: the largest error / bound measured on this machine — not detectable by this bound, and the bound is NOT tuned to
# catch them.
#   softmax without the max: while nothing overflows, exp(z) / sum exp(z) in float32 is as accurate as the shifted form (the
#     logits are exact inputs and expf is accurate to an ulp at 60 as at 0); what the shift buys is range, which
#     tests/test_gpu_hostile_inputs.py holds, not precision.
# Dropped from the issue's list: the box rule's `* 0.5` applied before instead of after the product — a multiplication by a
# power of two is exact (nothing here is near the underflow threshold), so both orders give the same bits: no mutant exists.
NOT_DETECTABLE = {
    "softmax without the subtracted max, logits around 60": 0.058,
}


@pytest.mark.parametrize("name", list(MUTANTS))
def test_emulated_wrong_kernel_leaves_the_bound(name):
    n, r = MUTANTS[name]()
    print(f"{name}: {n} elements beyond the bound, largest error / bound {r:.3g}")
    if name in NOT_DETECTABLE:
        assert n == 0 and r <= 1.0, "the bound now sees this mutant: move it out of NOT_DETECTABLE"
    else:
        assert n > 0 and r > 1.0, (name, n, r)


def test_record_fractions_of_20_bits_are_inside_the_sorted_bound_and_not_the_float_one():
    """The sorted route's documented 20 bits pass the "q20" formulas; against the single-launch route's float formulas they
    do not — which is why the GPU tests read the route back before they pick the formula."""
    inside = outside = 0
    for pm, ac in MODES:
        c = eb.get_case("d32")
        got = dict(grad_value=eb.emulated_grad_value(c, pm, ac, eb.quantised(20)))
        for records in ("q20", "float"):
            form, keep = eb.plain_reference("d32", "f32", pm, ac, records)
            n, r = _hits(got, dict(grad_value=form["grad_value"]), keep)
            print(f"20-bit fractions {pm} {int(ac)} against {records}: {n} beyond, largest {r:.3f}")
            inside += n if records == "q20" else 0
            outside += n if records == "float" else 0
    assert inside == 0 and outside > 0
