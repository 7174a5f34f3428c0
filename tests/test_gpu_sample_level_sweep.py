"""The samples of a unit and the level count swept through every kernel family (tests/sample_level_cases.py): S decides
how many trips a kernel makes over a unit's samples and which kernel runs at all, L which scan fills the level table, how
far the scans over the per-level-count starts run and what grad_value's cell words carry.  The rest of the suite runs one
trip of samples almost everywhere, multi-trip units at G = 4 only, and 1, 2, 3, 4, 8 or 17 levels.

Every comparison of the plain, masked, query-masked, per-level-count and discrete families is an EQUALITY with the fp64
oracle on the exact inputs of tests/exact_cases.py (rounded once for 16-bit results; the precondition is asserted before the
GPU is touched), and every test holds `msda_last_launch_info` — variant, group, trips, grad_value path, place-pass
variant — to the rules restated in sample_level_cases: a moved cap fails the test instead of turning it into a duplicate.
The fused families, whose softmax rules equality out, are held to the derived bound of tests/error_bound_cases.py.  Run
with ``-m gpu``."""
import contextlib

import numpy as np
import pytest
import torch

import exact_cases as ec
import head_dim_cases as hd
import sample_level_cases as sl
from test_gpu_exact_numerics import DEV, STORAGE, _dev, assert_exact, launch_info, options, run
from test_gpu_value_mask import make_mask

pytestmark = pytest.mark.gpu

BLOCK256 = dict(unit_fwd=0, lds_levels=0)       # the 256-thread forward and sample gradients
OPTION_SETS = {"default": {}, "block256": BLOCK256}
ROUTES = {"sorted_gather": (2, 2), "single_launch": (3, 1)}  # name: (option value_path, launch info value_path)
BILINEAR_LEVEL_CASES = [n for n in sl.LEVEL_CASES if ec.CASES[n][0] != "discrete"]
DISCRETE_LEVEL_CASES = [n for n in sl.LEVEL_CASES if ec.CASES[n][0] == "discrete"]
UNIFORM = [n for n in sl.ALL_CASES if sl.case_dims(n)[7] is None]


def expect(name, storage, opts, **kw):
    B, Q, H, D, _, S, _, _ = sl.case_dims(name)
    keys = {k: opts[k] for k in ("unit_fwd", "unit_waves", "lds_levels") if k in opts}
    return sl.expect(storage, D, S, units=B * Q * H, discrete=ec.CASES[name][0] == "discrete", **keys, **kw)


def run_query_masked(c, pm, ac, vdt, cdt, qm):
    """`run` with a query padding mask ([B, Q] bool on the host, True = real): the padded queries' points and weights hold NaN"""
    from msda_triton_amd import multiscale_deformable_attention
    m = qm.to(DEV)
    v = _dev(c["value"], vdt).requires_grad_(True)
    loc, attn = _dev(c["loc"], cdt), _dev(c["attn"], cdt)
    loc = torch.where(m.reshape(m.shape + (1,) * (loc.dim() - 2)), loc, torch.full_like(loc, float("nan"))).requires_grad_(True)
    attn = torch.where(m.reshape(m.shape + (1,) * (attn.dim() - 2)), attn, torch.full_like(attn, float("nan"))).requires_grad_(True)
    out = multiscale_deformable_attention(v, torch.from_numpy(np.array(c["shapes"])).to(DEV), loc, attn, pm, ac, query_mask=m)
    out.backward(_dev(c["grad_out"], cdt))
    torch.cuda.synchronize()
    return dict(out=out.detach().cpu(), grad_value=v.grad.cpu(), grad_loc=loc.grad.cpu(), grad_attn=attn.grad.cpu())


def sweep(name, storage, opts, what, mask=None, qmask=None, extra=None):
    """The case in its modes under the options: exact, and launched as the restated rules say.  -> the last launch info"""
    vdt, cdt = STORAGE[storage]
    discrete = ec.CASES[name][0] == "discrete"
    # (the mask kernels serve the uniform call; with per-level counts the package composes where(mask, value, 0) with the
    #  per-level-count kernels, which may be the one-wave-per-unit forward)
    want = expect(name, storage, opts, masked=(mask is not None or qmask is not None) and name in UNIFORM)
    want.update(extra or {})
    info = None
    with options(**opts):
        for pm, ac in sl.case_modes(name):
            tag = f"{what} {name} {storage} {pm} {int(ac)}"
            if qmask is not None:
                import query_mask_cases as qmc
                _, ref = qmc.exact_reference(name, pm, ac, qmask.numpy())
                got = run_query_masked(ec.get_case(name), pm, ac, vdt, cdt, qmask)
            elif mask is not None:
                ref = ec.masked_reference(name, pm, ac, mask.numpy())
                got = run(ec.get_case(name), pm, ac, vdt, cdt, mask=mask)
            else:
                ref = ec.checked_reference(name) if discrete else ec.checked_reference(name, pm, ac)
                got = run(ec.get_case(name), pm, ac, vdt, cdt, discrete=discrete)
            info = launch_info()
            assert_exact(got, ref, tag)
            sl.assert_info(info, want, tag)
    return info


def value_mask(name):
    B, _, _, _, levels, _ = ec.CASES[name][1]
    mask = make_mask("bernoulli", B, levels, seed=len(levels))
    assert 0 < int(mask.sum()) < mask.numel()
    return mask


# ----------------------------------------------------------------------------------------- the level counts
# (one test item per case, or per case and storage: the option sets, grad_value routes and, for the sample counts, the
#  storages are loops inside the item — every combination runs and names itself in the assertion's message)
@pytest.mark.parametrize("storage", hd.STORAGES)
@pytest.mark.parametrize("name", BILINEAR_LEVEL_CASES)
def test_level_counts_are_exact(name, storage):
    """1 ... 32 tiny unequal levels, uniform and per-level point counts, 16-byte and scalar path, all four modes: with
    default options (the one-wave-per-unit forward where it exists) and through the 256-thread kernels; grad_value by
    whichever route the size picks, read from the launch info."""
    for optset, opts in OPTION_SETS.items():
        info = sweep(name, storage, opts, optset)
        assert info["value_path"] in (1, 2), (optset, info)


@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("name", BILINEAR_LEVEL_CASES)
def test_level_counts_on_both_grad_value_routes(name, storage):
    """the sorted pipeline (5-bit level field of the cell words, place workgroups per (level, slice)) and the single-launch
    kernel (workgroups per (plane, level))"""
    for route, (opt, path) in ROUTES.items():
        sweep(name, storage, dict(BLOCK256, value_path=opt), route, extra=dict(value_path=path))


@pytest.mark.parametrize("storage", ["f32", "f64", "bf16"])
@pytest.mark.parametrize("name", DISCRETE_LEVEL_CASES)
def test_level_counts_discrete(name, storage):
    for route, (opt, path) in ROUTES.items():
        sweep(name, storage, dict(value_path=opt), route, extra=dict(value_path=path))


@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_thirty_two_levels_in_rounds_of_queries_and_two_passes(storage):
    info = sweep(sl.LEVEL_ROUNDS_CASE, storage, dict(BLOCK256, **sl.LEVEL_ROUNDS_OPTIONS), "rounds and passes",
                 extra=dict(value_path=2, value_passes=2))
    assert info["value_rounds"] > 1, info


@pytest.mark.parametrize("storage", ["f32", "bf16", "f32_vbf16"])
@pytest.mark.parametrize("name", BILINEAR_LEVEL_CASES)
def test_level_counts_under_a_value_mask(name, storage):
    """the value-mask twins on a pyramid with NaN in every padding pixel, against the oracle on where(mask, value, 0)"""
    for optset, opts in OPTION_SETS.items():  # (a masked kernel is never the one-wave-per-unit forward: variant 0 in both)
        sweep(name, storage, opts, f"value mask {optset}", mask=value_mask(name))


@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("name", [n for n in BILINEAR_LEVEL_CASES if n in UNIFORM])
def test_level_counts_under_a_query_mask(name, storage):
    sweep(name, storage, BLOCK256, "query mask", qmask=sl.query_mask(name))


@pytest.mark.parametrize("name", BILINEAR_LEVEL_CASES)
def test_level_counts_with_lds_served_levels(name):
    """lds_levels = 2 on 1 ... 32 levels: the kernel keeps the longest suffix of the level list that fits in LDS — here the
    whole list of tiny levels, up to 32 level bases and sizes — and walks 64 samples (L = 32) in four trips of 16; the
    scalar-path cases have no such variant, which the restated rule says and the launch info must confirm"""
    for storage in ("f32", "f32_vbf16"):
        info = sweep(name, storage, dict(unit_fwd=0, lds_levels=2), "lds levels")
        vec, g, _ = hd.instantiation(storage, sl.case_dims(name)[3])
        assert info["fwd_variant"] == int(vec == 4 and g <= 16), (storage, info)
        if info["fwd_variant"] == 1:
            assert info["fwd_lds_level_bytes"] > 0, (storage, info)


# ----------------------------------------------------------------------------------------- the samples of a unit
@pytest.mark.parametrize("name", sl.SAMPLE_CASES)
def test_trips_of_the_256_thread_kernels(name):
    """one full trip, a second trip of one sample, two full trips, three and more with a partial last one — per lane group
    of float32's 16-byte path and on the scalar path; the other storages run the same S in whatever trips their own caps give"""
    for storage in hd.STORAGES:
        sweep(name, storage, BLOCK256, "block256")


@pytest.mark.parametrize("name", sl.SAMPLE_CASES)
def test_trips_with_default_options(name):
    """what a small float32 call takes by default: the one-wave-per-unit forward in ceil(S / 64) trips where it exists"""
    for storage in ("f32", "bf16"):
        sweep(name, storage, {}, "default")


@pytest.mark.parametrize("name", sl.SAMPLE_CASES)
def test_trips_under_the_masks(name):
    for storage in ("f32", "bf16"):
        sweep(name, storage, BLOCK256, "value mask", mask=value_mask(name))
        if name in UNIFORM:
            sweep(name, storage, BLOCK256, "query mask", qmask=sl.query_mask(name))


@pytest.mark.parametrize("name", sl.LDS_CASES)
def test_trips_of_the_lds_served_level_kernels(name):
    """lds_levels = 2: the forward up to G = 16 and the sample gradients at G = 4 and 8 of float arithmetic on 16-byte pieces,
    a multi-trip sc rounded down to a multiple of G; declined — asserted — for float64 and the 16-bit operators"""
    for storage in hd.STORAGES:
        info = sweep(name, storage, dict(unit_fwd=0, lds_levels=2), "lds")
        assert info["fwd_variant"] == (1 if storage in ("f32", "f32_vbf16", "f32_vf16") else 0), (storage, info)


@pytest.mark.parametrize("storage", ["f32", "bf16", "f32_vbf16", "f64"])
@pytest.mark.parametrize("name", sl.UNIT_CASES)
def test_one_wave_per_unit_forward_at_its_boundaries(name, storage):
    """unit_fwd = 2: one trip | two at 64 | 65 samples (32 | 33 with two units per wave), eligible at 1024 samples and
    declined at 1025; float64 has no such kernel"""
    S = sl.case_dims(name)[5]
    for waves in (1, 2):
        info = sweep(name, storage, dict(unit_fwd=2, unit_waves=waves, lds_levels=0), f"unit_waves={waves}")
        assert info["fwd_variant"] == (2 if storage != "f64" and S <= 1024 else 0), (waves, info)


@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("name", sl.PLACE_CASES)
def test_place_pass_by_points_per_level(name, storage):
    """value_path = 2: 256 points per level take the 256-thread level-major place pass, 257 and 1024 the 1024-thread one,
    1025 the plane-major pass (strict = 0: its record order is free, its sums on these inputs exact all the same)"""
    P = sl.case_dims(name)[6]
    with options(strict=0):
        sweep(name, storage, dict(BLOCK256, value_path=2), "place", extra=dict(value_path=2, value_place_variant=sl.place_variant(P)))


# ----------------------------------------------------------------------------------------- the fused families
import error_bound_cases as eb  # noqa: E402

NAN = float("nan")
FUSED_KERNELS = {"module2": "fused", "module4_c": "fused_ragged", "levelref4": "fused_levelref", "hfbox": "fused_hfbox",
                 "hfbox_discrete": "fused_hfbox_discrete"}


def run_family(name, fc, pm, ac, vmask=None, qmask=None):
    """The family's public entry point under a KernelTimer, as tests/test_gpu_error_bounds.py runs it (padded pixels and
    padded queries' rows hold NaN) -> the results on the host, the launchers' names"""
    from msda_triton_amd.functional import KernelTimer, fused_hf_box_core, fused_hf_module_core, fused_module_core
    rule, _, _ = eb.fused_entry(name)
    discrete = name in eb.FUSED_DISCRETE
    v, pr, rf = (_dev(fc[k], torch.float32) for k in ("value", "proj", "ref"))
    kw = {}
    if vmask is not None:
        m = torch.from_numpy(vmask).to(DEV)
        v = torch.where(m[:, :, None, None], v, torch.full_like(v, NAN))
        kw["value_mask"] = m
    if qmask is not None:
        m = torch.from_numpy(qmask).to(DEV)
        pr = torch.where(m.reshape(m.shape + (1,) * (pr.dim() - 2)), pr, torch.full_like(pr, NAN))
        rf = torch.where(m.reshape(m.shape + (1,) * (rf.dim() - 2)), rf, torch.full_like(rf, NAN))
        kw["query_mask"] = m
    v.requires_grad_(True)
    pr.requires_grad_(True)
    rf.requires_grad_(not discrete)
    shapes = torch.from_numpy(np.array(fc["shapes"])).to(DEV)
    with KernelTimer() as kt:
        if rule == "hfbox":
            out = fused_hf_box_core(v, shapes, pr, rf, fc["counts"], eb.HFBOX_SCALE, *(() if discrete else (pm, ac)),
                                    sampling_mode="discrete" if discrete else "bilinear", **kw)
        elif rule == "levelref":
            out = fused_hf_module_core(v, shapes, pr, rf, pm, ac, **kw)
        else:
            out = fused_module_core(v, shapes, pr, rf, pm, ac, points_per_level=fc.get("counts"), **kw)
        out.backward(_dev(fc["grad_out"], torch.float32))
        torch.cuda.synchronize()
    got = dict(out=out.detach().cpu(), grad_value=v.grad.cpu(), grad_proj=pr.grad.cpu())
    if not discrete:
        got["grad_ref"] = rf.grad.cpu()
    return got, [r[0] for r in kt.records]


@contextlib.contextmanager
def spied_family(fam, log):
    """records (symbol, status) of every call of the family's float32 entry points, its mask twins included"""
    import re
    from msda_triton_amd import _lib
    lib = _lib.load()
    pat = re.compile(rf"msda_(fwd|bwd)_{fam}(_masked|_qmasked)?_f32")
    real = {n: getattr(lib, n) for n in set(_lib.EXPORTED_SYMBOLS + _lib.QUERY_MASK_SYMBOLS + _lib.MODULE_MASK_SYMBOLS +
                                              _lib.HFBOX_DISCRETE_SYMBOLS)
            if pat.fullmatch(n)}
    assert f"msda_fwd_{fam}_f32" in real and f"msda_bwd_{fam}_f32" in real, sorted(real)

    def spy(n):
        def call(*a):
            rc = real[n](*a)
            log.append((n, int(rc)))
            return rc
        return call

    for n in real:
        setattr(lib, n, spy(n))
    try:
        yield
    finally:
        for n in real:
            setattr(lib, n, real[n])


def assert_route(name, log, what):
    """the fused pair, once each and served — or, where the library declines (S beyond the one-pass limit of the backward's
    records, more levels than the fused level scan serves), no fused backward that was served: whatever the package asked
    the library for was served or answered MSDA_ERR_UNSUPPORTED (tests/test_sample_level_cases.py holds those refusals at
    the C ABI for every family), and it composed the chain rule around the plain operator"""
    base, fused = sl.FUSED_CASES[name][:2]
    fam = FUSED_KERNELS[base]
    if fused:
        assert log == [(f"msda_fwd_{fam}_f32", 0), (f"msda_bwd_{fam}_f32", 0)], (what, log)
    else:
        assert (f"msda_bwd_{fam}_f32", 0) not in log and all(rc in (0, sl.ERR_UNSUPPORTED) for _, rc in log), (what, log)
        if base == "levelref4":  # (this family's Function asks the library itself: served forward, declined backward)
            assert log == [(f"msda_fwd_{fam}_f32", 0), (f"msda_bwd_{fam}_f32", sl.ERR_UNSUPPORTED)], (what, log)


@pytest.mark.parametrize("name", list(sl.FUSED_CASES))
def test_fused_families_at_their_limits(name):
    """S = msda_fused_lp_limit exactly (the one LDS pass, full, at every lane group), S = limit + 1 and L = 9 (composed),
    L = 8 (the bounded level scan reading its last start): within the derived bound of tests/error_bound_cases.py"""
    base, fused, D, S, L = sl.FUSED_CASES[name]
    from msda_triton_amd import _lib
    limit = int(_lib.load().msda_fused_lp_limit(D, 4))
    assert limit == sl.fused_limit(D), (name, limit)
    if "_limit" in name or "_over" in name:
        assert S == limit + (0 if fused else 1), (name, S, limit)
    fc = eb.fused_case(name)
    for pm, ac in sl.fused_modes(name):
        what = f"{name} {pm} {int(ac)}"
        log = []
        with spied_family(FUSED_KERNELS[base], log):
            got, _ = run_family(name, fc, pm, ac)
        info = launch_info()
        assert_route(name, log, what)
        if fused and name not in eb.FUSED_DISCRETE:  # the whole unit in one trip, by the kernels the head dimension names
            g = hd.instantiation("f32", D)[1]
            sl.assert_info(info, dict(fwd_group=g, sample_group=g, fwd_trips=1, sample_trips=1), what)
        assert info["value_path"] in (1, 2), info
        form, keep, _ = eb.fused_formulas(fc, name, pm, ac, "q20" if info["value_path"] == 2 else "float")
        eb.assert_within(got, form, keep, what)


@pytest.mark.parametrize("name", ["module2_g8_limit", "module4_c_g8_limit", "module4_c_l8"])
def test_module_masked_pairs_at_their_limits(name):
    """the module's masked pairs (uniform and per-level counts) with a full LDS pass and at eight levels, against the
    pre-masked problem"""
    from test_gpu_module_masks import spied_symbols
    fc = eb.fused_case(name)
    rng = np.random.default_rng(13)
    vmask = rng.random(fc["value"].shape[:2]) > 0.25
    qmask = np.ones(fc["grad_out"].shape[:2], dtype=bool)
    qmask[:, 1::3] = False  # (a handful of queries: every third one is padding)
    assert vmask.any() and not vmask.all() and qmask.any() and not qmask.all()
    pre = dict(fc, value=np.where(vmask[:, :, None, None], fc["value"], 0.0),
               grad_out=np.where(qmask[:, :, None, None], fc["grad_out"], 0.0))
    log = []
    with spied_symbols(log):
        got, _ = run_family(name, fc, "zeros", False, vmask=vmask, qmask=qmask)
    fam = FUSED_KERNELS[sl.FUSED_CASES[name][0]]
    assert log == [f"msda_fwd_{fam}_masked_f32", f"msda_bwd_{fam}_masked_f32"], log
    info = launch_info()
    form, keep, _ = eb.fused_formulas(pre, name, "zeros", False, "q20" if info["value_path"] == 2 else "float")
    form["out"] = form["out"].where(qmask[:, :, None, None])                 # a padded query's row of `out` is zeros
    form["grad_value"] = form["grad_value"].where(vmask[:, :, None, None])    # a padded pixel's grad_value row is zeros
    eb.assert_within(got, form, keep, f"{name} masked")


LEVELREF_CASES = [n for n in sl.FUSED_CASES if sl.FUSED_CASES[n][0] == "levelref4"]


@pytest.mark.parametrize("masks", ["value_mask", "both_masks"])
@pytest.mark.parametrize("name", LEVELREF_CASES)
def test_levelref_masked_family_at_its_limits(name, masks):
    """the per-level-reference family's mask twins — msda_*_fused_levelref_masked_f32 under a value mask, ..._qmasked_f32
    once a query mask comes with it — with a full LDS pass at every lane group, and at limit + 1, where the
    backward answers MSDA_ERR_UNSUPPORTED and the package composes the chain rule around the masked plain kernels: against
    the pre-masked problem, within the same derived bound.  Padded pixels and padded queries' rows hold NaN."""
    _, fused, D, S, _ = sl.FUSED_CASES[name]
    fc = eb.fused_case(name)
    rng = np.random.default_rng(17)
    vmask = rng.random(fc["value"].shape[:2]) > 0.25
    qmask = None
    if masks == "both_masks":
        qmask = np.ones(fc["grad_out"].shape[:2], dtype=bool)
        qmask[:, 1::3] = False  # (a handful of queries: every third one is padding)
        assert qmask.any() and not qmask.all()
    assert vmask.any() and not vmask.all()
    pre = dict(fc, value=np.where(vmask[:, :, None, None], fc["value"], 0.0))
    if qmask is not None:
        pre["grad_out"] = np.where(qmask[:, :, None, None], fc["grad_out"], 0.0)
    twin = "masked" if qmask is None else "qmasked"
    fwd, bwd = f"msda_fwd_fused_levelref_{twin}_f32", f"msda_bwd_fused_levelref_{twin}_f32"
    for pm, ac in sl.fused_modes(name):
        what = f"{name} {masks} {pm} {int(ac)}"
        log = []
        with spied_family("fused_levelref", log):
            got, _ = run_family(name, fc, pm, ac, vmask=vmask, qmask=qmask)
        info = launch_info()
        if fused:
            assert log == [(fwd, 0), (bwd, 0)], (what, log)
            g = hd.instantiation("f32", D)[1]
            sl.assert_info(info, dict(fwd_group=g, sample_group=g, fwd_trips=1, sample_trips=1), what)
        else:  # the forward's records are smaller, it still serves the unit; the backward declines at the C ABI and is composed
            assert log == [(fwd, 0), (bwd, sl.ERR_UNSUPPORTED)], (what, log)
        assert info["value_path"] in (1, 2), info
        form, keep, _ = eb.fused_formulas(pre, name, pm, ac, "q20" if info["value_path"] == 2 else "float")
        if qmask is not None:
            form["out"] = form["out"].where(qmask[:, :, None, None])              # a padded query's row of `out` is zeros
        form["grad_value"] = form["grad_value"].where(vmask[:, :, None, None])    # a padded pixel's grad_value row is zeros
        eb.assert_within(got, form, keep, what)
