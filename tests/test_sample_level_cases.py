"""The sample-count / level-count sweep proves on the CPU that it reaches what it claims (tests/sample_level_cases.py): the
restated trip rules give the caps the kernels' documentation states and agree with the library where it exposes them, the
case list covers every class of `required()`, every case is exact in float32 in every mode it is run in, and each emulated
wrong kernel — a dropped last trip, a level scan without its shift-by-8 step, a level table cut at 16 levels, a pst[L] that
is one short, a level lookup that skips empty levels, a 4-bit level field — changes a tensor the GPU tests compare."""
import numpy as np
import pytest
import torch

import exact_cases as ec
import head_dim_cases as hd
import sample_level_cases as sl

ALL_RUNS = [(n, pm, ac) for n in sl.ALL_CASES if ec.CASES[n][0] != "discrete" for pm, ac in sl.case_modes(n)]
DISCRETE = [n for n in sl.ALL_CASES if ec.CASES[n][0] == "discrete"]


# ----------------------------------------------------------------------------------------- the restated rules
def test_caps_of_the_256_thread_kernels():
    assert [sl.gather_cap(g) for g in (4, 8, 16, 32, 64)] == [23, 47, 95, 191, 383]          # float32 and 16-bit operators
    assert [sl.gather_cap(g, acc=8) for g in (4, 8, 16, 32, 64)] == [15, 31, 63, 127, 255]   # float64: 48-byte records
    assert sl.plan_gather(8, 47) == (47, 1) and sl.plan_gather(8, 48) == (47, 2) and sl.plan_gather(8, 109) == (47, 3)
    assert sl.plan_gather(64, 1 << 20, acc=8, aux=True)[0] == 48 * 1024 // (4 * 72) - 1


def test_caps_of_the_lds_served_level_kernels():
    # 72 KiB over 1024 / G units: 8, 17, 35 samples in one trip; a multi-trip sc above G drops to a multiple of G
    assert [sl.lds_plan(g, s) for g, s in ((4, 8), (8, 17), (16, 35))] == [(8, 1), (17, 1), (35, 1)]
    assert [sl.lds_plan(g, s) for g, s in ((4, 9), (8, 18), (16, 36))] == [(8, 2), (16, 2), (32, 2)]
    assert sl.lds_plan(8, 34) == (16, 3) and sl.lds_plan(4, 18) == (8, 3)
    # the fused backward's 44-byte records in 100 KiB
    assert sl.lds_plan(8, 1 << 20, aux=True)[0] == (100 * 1024 // (128 * 44) - 1) // 8 * 8


def test_unit_forward_and_place_pass_rules():
    assert [sl.unit_trips(s) for s in (1, 64, 65, 1024)] == [1, 1, 2, 16]
    assert [sl.unit_trips(s, 2) for s in (32, 33, 1024)] == [1, 2, 32]
    assert [sl.place_variant(p) for p in sl.PLACE_POINTS] == [2, 1, 1, 0]
    assert sl.place_variant(256, q_slice=7) == 1  # (a slice of more queries than six rounds of 256-thread workgroups cover)
    e = sl.expect("f32", 32, 1025, unit_fwd=2, lds_levels=0)
    assert e["fwd_variant"] == 0 and e["fwd_trips"] == 22
    assert sl.expect("f32", 256, 64, unit_fwd=2, unit_waves=2, lds_levels=0)["fwd_trips"] == 1  # 64 lanes: one unit per wave
    assert sl.expect("bf16", 8, 65, unit_fwd=2, lds_levels=0)["fwd_group"] == 1                  # one 16-byte lane holds the row
    assert sl.expect("f64", 32, 64, unit_fwd=2, lds_levels=2) == dict(fwd_variant=0, fwd_group=16, fwd_trips=2, sample_variant=0,
                                                                      sample_group=16, sample_trips=2)


def test_restated_rules_equal_the_library():
    """msda_fused_lp_limit is plan_gather's cap with the fused backward's records, for the narrower of the two paths' groups"""
    from msda_triton_amd import _lib
    lib = _lib.load()  # (host code: no GPU needed)
    for D in (5, 8, 17, 32, 33, 64, 68, 128, 132, 256, 260):
        for elem in (2, 4, 8):
            assert sl.fused_limit(D, elem) == hd.fused_lp_limit(D, elem) == int(lib.msda_fused_lp_limit(D, elem)), (D, elem)
    assert set(_lib.LAUNCH_INFO_KEYS) >= {"fwd_trips", "sample_trips"}
    for k in ("fwd_trips", "sample_trips"):
        assert int(lib.msda_last_launch_info(k.encode())) >= 0


def test_the_c_abi_refuses_what_the_kernels_are_never_handed():
    """a count of 0 anywhere in a 32-entry list is MSDA_ERR_BAD_ARG (so the sweep's smallest counts are 1), and the fused
    per-level-count and box families decline 9 levels with MSDA_ERR_UNSUPPORTED while 8 pass the guard"""
    if torch.cuda.is_available():
        pytest.skip("the calls pass host addresses as buffers: safe only where a call that slipped past its guard cannot launch")
    import test_entry_point_contract as epc
    from msda_triton_amd import _lib
    lib = _lib.load()
    for pos in (0, 15, 31):
        counts = [2] * sl.MAX_LEVELS
        counts[pos] = 0
        for direction, kind in (("fwd", "ragged"), ("bwd", "ragged"), ("fwd", "discrete"), ("bwd", "discrete")):
            assert epc._call(lib, direction, kind, "f32", L=sl.MAX_LEVELS, I=64, ppl=counts) == sl.ERR_BAD_ARG, (pos, direction, kind)
    for kind in ("fused_ragged", "fused_hfbox"):
        for direction, over in (("fwd", {}), ("bwd", {"grad_value": None})):
            L = sl.FUSED_RAGGED_MAX_LEVELS
            assert epc._call(lib, direction, kind, "f32", L=L, I=64, ppl=[1] * L, **over) not in (sl.ERR_UNSUPPORTED, sl.ERR_BAD_ARG)
            assert epc._call(lib, direction, kind, "f32", L=L + 1, I=64, ppl=[1] * (L + 1), **over) == sl.ERR_UNSUPPORTED
            assert b"at most 8 levels" in lib.msda_last_error()


def _hfbox_discrete_call(lib, direction, L):
    """msda_{fwd,bwd}_fused_hfbox_discrete_f32 with valid tiny arguments and L one-point levels (no grad_value: no workspace)"""
    import ctypes
    import test_entry_point_contract as epc
    host = epc._Host()
    ppl, scale = host.array(ctypes.c_int32, [1] * L), host.array(ctypes.c_float, [1.0] * L)
    dims = (1, 64, 1, 4, 1, L)  # B, I, H, D, Q, L
    if direction == "fwd":
        return lib.msda_fwd_fused_hfbox_discrete_f32(*[host.p] * 5, *dims, ppl, scale, 0.5, 0, None)
    return lib.msda_bwd_fused_hfbox_discrete_f32(*[host.p] * 5, None, host.p, *dims, ppl, scale, 0.5, 0, 0, None, 0, None)


def test_the_c_abi_declines_what_the_fused_kernels_do_not_take():
    """every fused family's backward — the per-level-reference mask twin among them — takes S = msda_fused_lp_limit past its
    guards and answers MSDA_ERR_UNSUPPORTED for one sample more, at the D of every lane group (the forward likewise at its
    own, larger cap: at limit + 1 the package runs the fused forward and composes the backward); the box rule in
    front of discrete sampling declines 9 levels as its bilinear twin does (the GPU tests see the package compose there)"""
    if torch.cuda.is_available():
        pytest.skip("the calls pass host addresses as buffers: safe only where a call that slipped past its guard cannot launch")
    import test_entry_point_contract as epc
    from msda_triton_amd import _lib
    lib = _lib.load()
    refused = (sl.ERR_UNSUPPORTED, sl.ERR_BAD_ARG)
    for D in sl.FUSED_LIMIT_DIMS.values():
        # the backward's records carry (a, ox, oy) per slot: msda_fused_lp_limit; the forward's are plan_gather's plain ones
        limits = dict(bwd=sl.fused_limit(D), fwd=sl.gather_cap(hd.instantiation("f32", D)[1]))
        assert limits["fwd"] > limits["bwd"]
        for kind in ("fused", "fused_ragged", "fused_levelref", "fused_hfbox", "fused_levelref_masked"):
            for direction, over in (("fwd", {}), ("bwd", {"grad_value": None})):
                def call(S):
                    size = dict(ppl=[S]) if epc._counts(kind) else dict(P=S)
                    return epc._call(lib, direction, kind, "f32", D=D, I=64, **size, **over)
                assert call(limits[direction]) not in refused, (D, kind, direction)
                assert call(limits[direction] + 1) == sl.ERR_UNSUPPORTED, (D, kind, direction)
    assert _lib.has_fused_hfbox_discrete()
    for direction in ("fwd", "bwd"):
        assert _hfbox_discrete_call(lib, direction, sl.FUSED_RAGGED_MAX_LEVELS) not in refused, direction
        assert _hfbox_discrete_call(lib, direction, sl.FUSED_RAGGED_MAX_LEVELS + 1) == sl.ERR_UNSUPPORTED, direction


def test_support_and_workspace_queries_take_every_case():
    """The library's other host queries know nothing of trips: msda_bwd_supported and the workspace sizes depend on the
    planes' pixels and the sorted grad_value pipeline alone, so there is no cap to hold against them.  What they share with
    the restated rules is held: every case of the sweep is supported (a small one needs no workspace: the size may be
    0), with all 32 levels; a count of 0 and a 33rd level are not."""
    import ctypes
    from msda_triton_amd import _lib
    lib = _lib.load()

    def ragged(counts, L, I):  # noqa: E741
        a = (ctypes.c_int32 * len(counts))(*counts)
        p = ctypes.cast(a, ctypes.c_void_p)
        return (int(lib.msda_bwd_ragged_supported(2, I, 2, 32, 13, L, p, 4)),
                int(lib.msda_bwd_ragged_workspace_bytes(2, I, 2, 32, 13, L, p, 4, 4, 0, 0)) >= 0)

    for name in sl.ALL_CASES:
        if ec.CASES[name][0] == "discrete":
            continue
        B, Q, H, D, L, S, P, counts = sl.case_dims(name)
        I = sum(h * w for h, w in ec.CASES[name][1][4])  # noqa: E741
        if counts is None:
            assert lib.msda_bwd_supported(B, I, H, D, Q, L, P, 4) == 1, name
            assert lib.msda_bwd_workspace_bytes(B, I, H, D, Q, L, P, 4, 4, 0, 0) >= 0, name
        else:
            a = (ctypes.c_int32 * L)(*counts)
            assert lib.msda_bwd_ragged_supported(B, I, H, D, Q, L, ctypes.cast(a, ctypes.c_void_p), 4) == 1, name
    I = sum(h * w for h, w in sl.pyramid(sl.MAX_LEVELS))  # noqa: E741
    assert ragged(sl.level_point_counts(sl.MAX_LEVELS), sl.MAX_LEVELS, I) == (1, True)
    for pos in (0, 15, 31):
        counts = sl.level_point_counts(sl.MAX_LEVELS)
        counts[pos] = 0
        assert ragged(counts, sl.MAX_LEVELS, I)[0] == 0, pos
    assert ragged([1] * (sl.MAX_LEVELS + 1), sl.MAX_LEVELS + 1, I)[0] == 0


# ----------------------------------------------------------------------------------------- the case list
def test_case_list_reaches_every_class():
    got, need = sl.reached(), sl.required()
    print(sorted(got, key=str))
    assert need <= got, sorted(need - got, key=str)


def test_sample_cases_sit_on_the_restated_boundaries():
    for tag, D in sl.SAMPLE_DIMS.items():
        G = hd.instantiation("f32", D)[1]
        trips = [sl.plan_gather(G, sl.case_dims(f"sc_{tag}_{c}")[5])[1] for c in sl.SAMPLE_CLASSES]
        assert trips == [1, 2, 2, 3], (tag, trips)
        for c in sl.SAMPLE_CLASSES:  # the per-level-count twin: the same S over two levels
            assert sl.case_dims(f"sc_{tag}_{c}_c")[5] == sl.case_dims(f"sc_{tag}_{c}")[5]
    for tag, D in sl.LDS_DIMS.items():
        G = hd.instantiation("f32", D)[1]
        assert [sl.lds_plan(G, sl.case_dims(f"lds_{tag}_{c}")[5])[1] for c in sl.SAMPLE_CLASSES] == [1, 2, 2, 3], tag
    assert {sl.case_dims(n)[5] for n in sl.UNIT_CASES} == {32, 33, 64, 65, 1024, 1025}
    for n in sl.PLACE_CASES:  # (Q within the six rounds of workgroups that P = 256 allows, whatever the slices)
        assert sl.case_dims(n)[1] <= 6


def test_level_cases():
    assert {5, 9, 16, 32} <= set(sl.LEVEL_COUNTS) and max(sl.LEVEL_COUNTS) == sl.MAX_LEVELS
    lv = sl.pyramid(sl.MAX_LEVELS)
    assert (1, 1) in lv and any(h == 1 < w for h, w in lv) and any(w == 1 < h for h, w in lv)
    assert all(a != b for a, b in zip(lv, lv[1:])) and max(max(s) for s in lv) <= 7
    for L in sl.LEVEL_COUNTS:
        counts = sl.level_point_counts(L)
        assert len(counts) == L and max(counts) > 1 and (L == 1 or counts[0] == 1)
        assert L < 5 or 1 == counts[-1] == counts[L // 2]
        assert ec.CASES[f"lv{L}_c"][1][5] == counts == ec.CASES[f"lv{L}_disc"][1][5]
    B, Q = ec.CASES[sl.LEVEL_ROUNDS_CASE][1][:2]
    assert B % 2 == 0 and Q > 2 * sl.LEVEL_ROUNDS_OPTIONS["q_round"]  # three rounds of queries, two passes over the batch


@pytest.mark.parametrize("name,pm,ac", ALL_RUNS, ids=[f"{n}-{pm}_{int(ac)}" for n, pm, ac in ALL_RUNS])
def test_precondition_holds(name, pm, ac):
    bud = ec.precondition(name, pm, ac)
    assert set(bud) == set(ec.TENSORS) and max(bud.values()) <= ec.F32_BITS
    c = ec.get_case(name)
    for k in ("value", "loc", "attn", "grad_out"):  # the inputs survive every storage type the case is run in
        t = torch.from_numpy(np.array(c[k]))
        for dt in (ec.F16, ec.BF16):
            assert torch.equal(t.to(dt).double(), t), (name, k, dt)


@pytest.mark.parametrize("name", DISCRETE)
def test_precondition_holds_discrete(name):
    bud = ec.precondition(name)
    assert set(bud) == {"out", "grad_value", "grad_attn"} and max(bud.values()) <= ec.F32_BITS


@pytest.mark.parametrize("name", ["lv32_p2", "sc_g8_3trips+", "uf_s33"])
def test_masked_references_are_exact(name):
    """(both assert float32 == float64 themselves)"""
    import query_mask_cases as qmc
    from test_gpu_value_mask import make_mask
    B, _, _, _, levels, _ = ec.CASES[name][1]
    qm = sl.query_mask(name)
    assert 0 < int(qm.sum()) < qm.numel()
    for pm, ac in sl.case_modes(name):
        ec.masked_reference(name, pm, ac, make_mask("bernoulli", B, levels, seed=len(levels)).numpy())
        qmc.exact_reference(name, pm, ac, qm.numpy())


# ----------------------------------------------------------------------------------------- mutants
def _ref(name, pm, ac):
    return ec.checked_reference(name, pm, ac)


@pytest.mark.parametrize("name", ["lv32_p2", "lv9_c", "sc_g8_3trips+_c"])
def test_the_gather_formulation_is_the_oracle(name):
    """`gather_out` and `gather_grad_value` with no mutation ARE the reference (fp64 sums of exact terms: bit for bit)"""
    c = ec.get_case(name)
    for pm, ac in sl.SAMPLE_MODES:
        assert np.array_equal(sl.gather_out(c, pm, ac), _ref(name, pm, ac)["out"])
        assert np.array_equal(sl.gather_grad_value(c, pm, ac), _ref(name, pm, ac)["grad_value"])


@pytest.mark.parametrize("name,G", [("sc_g4_cap+1", 4), ("sc_g8_3trips+", 8), ("sc_g8_3trips+_c", 8), ("sc_g64_3trips+", 64),
                                    ("sc_scalar_cap+1_c", 8)])
def test_mutant_dropped_last_trip(name, G):
    c = ec.get_case(name)
    sc, trips = sl.plan_gather(G, sl.case_dims(name)[5])
    assert trips >= 2
    for pm, ac in sl.SAMPLE_MODES:
        out = sl.gather_out(c, pm, ac, keep=sl.keep_without_last_trip(c, sc))
        assert not np.array_equal(out, _ref(name, pm, ac)["out"]), (name, pm, ac)


@pytest.mark.parametrize("name", ["lv9_p2", "lv16_p2", "lv9_d5", "lv16_c"])
def test_mutant_level_scan_without_the_shift_by_eight(name):
    c = ec.get_case(name)
    start = sl.scan_without_shift(c["shapes"], 8)
    true = sl.level_starts(c["shapes"])
    assert np.array_equal(sl.scan_without_shift(c["shapes"], None), true)
    assert np.array_equal(start[:8], true[:8]) and (start[8:] != true[8:]).all()  # wrong from level 8 on, and only there
    for pm, ac in ec.MODES:
        assert not np.array_equal(sl.gather_out(c, pm, ac, start=start), _ref(name, pm, ac)["out"]), (name, pm, ac)


@pytest.mark.parametrize("name", ["lv17_p2", "lv32_p2", "lv32_c", "lv17_d5"])
def test_mutant_level_table_of_sixteen_levels(name):
    """levels from 16 on read the table rows of levels 0 ..."""
    c = ec.get_case(name)
    row = np.arange(len(c["shapes"])) % 16
    for pm, ac in ec.MODES:
        assert not np.array_equal(sl.gather_out(c, pm, ac, row=row), _ref(name, pm, ac)["out"]), (name, pm, ac)


@pytest.mark.parametrize("name", ["lv32_c", "lv9_c", "lv5_c", "sc_g8_cap_c"])
def test_mutant_last_level_start_one_short(name):
    c = ec.get_case(name)
    for pm, ac in sl.SAMPLE_MODES:
        assert not np.array_equal(sl.gather_out(c, pm, ac, keep=sl.keep_without_last_sample(c)), _ref(name, pm, ac)["out"]), (name, pm, ac)


def test_mutant_level_lookup_that_skips_empty_levels():
    """On a count list WITH empty levels — which only the CPU can evaluate: the C ABI answers MSDA_ERR_BAD_ARG (above)."""
    c = sl.zero_count_case()
    counts = c["counts"]
    assert counts[0] == 0 == counts[-1] and 0 in counts[1:-1] and counts[-2] > 0
    wrong = sl.skipping_zero_counts(c)
    assert wrong["counts"] != counts and sum(wrong["counts"]) == sum(counts)
    for pm, ac in ec.MODES:
        good, bad = (ec._oracle_all(ec._oracle(), x, pm, ac, np.float64) for x in (c, wrong))
        assert not np.array_equal(good["out"], bad["out"]) and not np.array_equal(good["grad_value"], bad["grad_value"])


@pytest.mark.parametrize("name", ["lv17_p2", "lv32_p2", "lv32_c"])
def test_mutant_four_bit_level_field(name):
    c = ec.get_case(name)
    lv = np.arange(len(c["shapes"])) & 15
    for pm, ac in ec.MODES:
        assert not np.array_equal(sl.gather_grad_value(c, pm, ac, cell_level=lv), _ref(name, pm, ac)["grad_value"]), (name, pm, ac)


# ----------------------------------------------------------------------------------------- the fused families
def test_fused_cases_sit_on_the_library_limits():
    import error_bound_cases as eb
    from msda_triton_amd import _lib
    lib = _lib.load()
    groups = set()
    for name, (base, fused, D, S, L) in sl.FUSED_CASES.items():
        _, _, P = eb.fused_entry(name)
        assert S == (L * P if isinstance(P, int) else sum(P)) and len(eb.FUSED_SHAPES[name][1]) == L, name
        if name.endswith(("_limit", "_over")):
            limit = int(lib.msda_fused_lp_limit(D, 4))
            assert S == limit + (0 if fused else 1) and fused == name.endswith("_limit"), (name, S, limit)
            groups.add((base, hd.instantiation("f32", D)[1], fused))
        else:
            assert L == sl.FUSED_RAGGED_MAX_LEVELS + (0 if fused else 1) and S <= int(lib.msda_fused_lp_limit(D, 4)), name
    assert groups == {(b, g, f) for b in sl.FUSED_BASES for g in (4, 8, 16, 32, 64) for f in (True, False)}
    assert {n for n in sl.FUSED_CASES if "_l" in n and n[-1] in "89"} == {f"{b}_l{L}" for b in sl.FUSED_LEVEL_BASES for L in (8, 9)}


@pytest.mark.parametrize("name", list(sl.FUSED_CASES))
def test_fused_bound_covers_the_case(name):
    """The derivation of tests/error_bound_cases.py as written covers these shapes: its fp64 values are autograd's, and a
    float32 composition on the host stays inside the bound (all kept elements), with the kink share under its cap."""
    import error_bound_cases as eb
    fc = eb.fused_case(name)
    for pm, ac in sl.fused_modes(name):
        form, keep, kink = eb.fused_formulas(fc, name, pm, ac)
        r64 = eb.fused_torch(fc, name, pm, ac, torch.float64)
        assert set(r64) == set(form)
        for k, r in r64.items():
            assert np.abs(form[k].val - r.numpy()).max() <= 1e-12 * max(float(r.abs().max()), 1.0), (name, pm, ac, k)
        res = eb.ratios(eb.fused_torch(fc, name, pm, ac, torch.float32), form, keep)
        print(name, pm, ac, {k: round(r, 3) for k, (_, r) in res.items()})
        assert all(n == 0 and r <= 1.0 for n, r in res.values()), (name, pm, ac, res)
        assert kink.mean() <= eb.MAX_EXCLUDED, (name, pm, ac, kink.mean())
