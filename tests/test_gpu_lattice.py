"""The kernels ON the pixel lattice: sampling points whose pixel coordinate is an integer (or a half), where grad_loc is
discontinuous, "border" padding switches its gradient off (px <= 0, px >= n - 1) and "zeros" drops corners (px = -1,
n - 1, n) — the places a `>` for a `>=`, a `ceil - 1` for a `floor`, a clamp on the wrong side of the fraction or a
masked corner left in the derivative give another answer.  The rest of the suite masks these samples out (kink_mask) or
avoids them by construction; here nothing is masked and no sample is excluded.

First part: the lattice cases of tests/exact_cases.py (kind "lattice"; tests/test_lattice_cases.py shows on the CPU that
the C oracle, grid_sample's autograd and the gather formulation agree there bit for bit, that every class of position is
among the inputs and that emulated wrong kernels differ) through the plain operator: out, grad_value, grad_loc and
grad_attn EQUAL the fp64 oracle, rounded once for 16-bit results, in every storage type, on both grad_value routes and in
every forced variant, `msda_last_launch_info` naming what ran.  Second part: the fused module-core families on points
their prologues form exactly.  Run with ``-m gpu``."""
import pytest
import torch

import exact_cases as ec
import head_dim_cases as hd
from test_gpu_exact_numerics import STORAGE, assert_exact, launch_info, options, run
from test_gpu_value_mask import make_mask

pytestmark = pytest.mark.gpu

PLAIN = [n for n in ec.LATTICE if "_c" not in n and "_d4" not in n]  # lat_{f,t,u}_{d32,d5}
WIDE = [n for n in PLAIN if n.endswith("d32")]                       # 16-byte pieces: what the forced variants exist for
COUNTS = [n for n in ec.LATTICE if n.endswith("_c")]
ROUTES = {"sorted_gather": (2, 2), "single_launch": (3, 1)}          # name: (option value_path, launch info value_path)


def runs(names):
    return [(n, pm, ac) for n, pm, ac in ec.LATTICE_RUNS if n in names]


def ids(names):
    return [f"{n}-{pm}_{int(ac)}" for n, pm, ac in runs(names)]


def check(name, pm, ac, storage, layout="dense", mask=None):
    """One forward + backward of the case: every tensor equals the reference, every sample compared.  -> launch info"""
    vdt, cdt = STORAGE[storage]
    ref = ec.checked_reference(name, pm, ac) if mask is None else ec.masked_reference(name, pm, ac, mask.numpy())
    got = run(ec.get_case(name), pm, ac, vdt, cdt, layout, mask=mask)
    info = launch_info()
    assert_exact(got, ref, f"{name} {pm} {int(ac)} {storage} {layout}{'' if mask is None else ' masked'}")
    return info


def check_modes(name, storage, **kw):
    return [check(name, pm, ac, storage, **kw) for pm, ac in ec.lattice_modes(name)]


# ----------------------------------------------------------------------------------------- storages x modes
@pytest.mark.parametrize("storage", list(STORAGE))
@pytest.mark.parametrize("name,pm,ac", runs(PLAIN), ids=ids(PLAIN))
def test_lattice_is_exact(name, pm, ac, storage):
    """The six storages x the four modes, at a 16-byte D (32) and a scalar-path D (5)."""
    info = check(name, pm, ac, storage)
    D = ec.CASES[name][1][3]
    hd.assert_info(info, hd.expect_info(storage, D), f"{name} {storage}")
    assert (info["fwd_vec"] == 1) == (D == 5), info


# ----------------------------------------------------------------------------------------- both grad_value routes
@pytest.mark.parametrize("storage", ["f32", "bf16", "f32_vbf16"])
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name", PLAIN)
def test_both_grad_value_routes_are_exact(name, route, storage):
    """... behind the 256-thread forward (the matrix above takes the one-wave-per-unit forward where the shape admits it)."""
    opt, path = ROUTES[route]
    with options(value_path=opt, unit_fwd=0):
        for info in check_modes(name, storage):
            assert info["value_path"] == path and info["fwd_variant"] == 0 and info["sample_variant"] == 0, info


# ----------------------------------------------------------------------------------------- forced variants
@pytest.mark.parametrize("storage", ["f32", "f32_vbf16"])
@pytest.mark.parametrize("planes", [1, 2], ids=["one_plane", "two_planes"])
@pytest.mark.parametrize("name", WIDE)
def test_lds_served_levels_are_exact(name, planes, storage):
    """Forward and sample gradients from the LDS copy of the levels: its row of zeros serves every corner "zeros" drops."""
    with options(unit_fwd=0, lds_levels=2, lds_planes=planes):
        for info in check_modes(name, storage):
            assert info["fwd_variant"] == 1 and info["fwd_lds_planes"] == planes and info["sample_variant"] == 1, info


@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("name", WIDE)
def test_one_wave_per_unit_forward_is_exact(name, storage):
    with options(unit_fwd=2):
        for info in check_modes(name, storage):
            assert info["fwd_variant"] == 2, info


@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("name", WIDE)
def test_padded_value_rows_are_exact(name, storage):
    check_modes(name, storage, layout="padded")


@pytest.mark.parametrize("storage", ["f32", "f32_vbf16", "bf16"])
@pytest.mark.parametrize("name", WIDE)
def test_four_byte_aligned_view_is_exact(name, storage):
    """Rows that start 4 bytes into a 16-byte unit take the scalar kernels, also where the LDS-served levels are forced."""
    with options(unit_fwd=0, lds_levels=2):
        for info in check_modes(name, storage, layout="unaligned"):
            assert info["fwd_variant"] == 0 and info["fwd_vec"] == 1 and info["sample_vec"] == 1, info


@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("name", WIDE)
def test_two_passes_over_the_batch_are_exact(name, storage):
    with options(value_path=2, ws_passes=2):
        for info in check_modes(name, storage):
            assert info["value_path"] == 2 and info["value_passes"] == 2, info


# ----------------------------------------------------------------------------------------- per-level point counts
@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("value_path", [0, 2, 3])
@pytest.mark.parametrize("name", COUNTS)
def test_points_per_level_is_exact(name, value_path, storage):
    with options(value_path=value_path):
        for info in check_modes(name, storage):
            assert not value_path or info["value_path"] == (2 if value_path == 2 else 1), info


# ----------------------------------------------------------------------------------------- value-mask twins
@pytest.mark.parametrize("storage", ["f32", "bf16", "f32_vbf16"])
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name", PLAIN)
def test_value_mask_twins_are_exact_on_a_poisoned_pyramid(name, route, storage):
    """NaN in every padding pixel: a corner the mask drops must stay out of the DERIVATIVE too, also where its weight is 0."""
    B, levels = ec.CASES[name][1][0], ec.CASES[name][1][4]
    mask = make_mask("bernoulli", B, levels, seed=len(name) + 7)
    assert 0 < int(mask.sum()) < mask.numel()
    opt, path = ROUTES[route]
    with options(value_path=opt):
        for info in check_modes(name, storage, mask=mask):
            assert info["value_path"] == path and info["fwd_variant"] == 0, info


# ----------------------------------------------------------------------------------------- the fused module-core families
from msda_triton_amd import _ext, _lib  # noqa: E402
from test_gpu_head_dim import _worst, assert_16_bit_close, fused_run  # noqa: E402
from test_gpu_parity import BWD_TOL, FWD_TOL  # noqa: E402

FUSED_IDS = [f"{f}-{s}-d{d}-ref{rd}{'-universal' if u else ''}" for f, s, d, rd, u in hd.fused_lattice_case_list()]


@pytest.mark.parametrize("family,storage,D,ref_dim,universal", hd.fused_lattice_case_list(), ids=FUSED_IDS)
def test_fused_families_on_the_lattice(family, storage, D, ref_dim, universal):
    """Uniform, per-level counts, per-level reference points (and the masked twin on a NaN-poisoned pyramid) and the HF box
    rule on the draws of head_dim_cases.fused_lattice_inputs: the prologue forms every sampling point exactly, so kernels and
    reference sample the same lattice points and NO offset gradient is left out of the comparison (elsewhere up to 2 % are).
    universal: levels of arbitrary size under the zero-initialised module with reference points of 0, 0.5, 1 and -0.
    float64 at 1e-8 and float32 at FWD_TOL / BWD_TOL against head_dim_cases.fused_reference; 16-bit storage against the
    float32 kernels on the same inputs with the bounds of tests/test_gpu_fused_storage.py."""
    want_info = hd.expect_info(hd.FUSED_ARITH[storage], D)
    if storage in hd.SIXTEEN_BIT:  # their grad_value passes are the float32 pipeline on 16-bit rows: VEC = 4
        want_info.update({k: v for k, v in hd.expect_info("f32", D).items() if k.startswith("value_")})
    elem = hd.fused_elem_size(storage)
    limit = int(_lib.load().msda_fused_lp_limit(D, elem))
    ext = _ext.load()
    S = max(sum(hd.LATTICE_COUNTS), sum(hd.UNIVERSAL_COUNTS), hd.LATTICE_P * len(ec.LATTICE_LEVELS[False]))
    assert S <= limit and (ext is None or int(ext.fused_lp_limit(D, elem)) == limit)
    for pm, ac in hd.LATTICE_FUSED_MODES:
        inp = hd.fused_lattice_inputs(family, storage, D, ref_dim, ac, universal)
        what = f"{family} {storage} D={D} ref_dim={ref_dim} {pm} {int(ac)}{' universal' if universal else ''}"
        got, names, info = fused_run(inp, pm, ac)
        assert names == hd.FUSED_NAMES[family], (what, names)  # the fused kernels, no composition
        hd.assert_info(info, want_info, what)
        if storage in hd.FUSED_AGAINST_FP64:
            want = hd.fused_reference(inp, pm, ac)
            td = inp["proj"].dtype
            tols = [FWD_TOL[td], BWD_TOL[td], BWD_TOL[td], BWD_TOL[td]]
            print(what, "error / bound:", [round(_worst(g, w, **t), 4) for g, w, t in zip(got, want, tols)])
            for name, g, w, t in zip(("out", "grad_value", "grad_proj", "grad_ref"), got, want, tols):
                torch.testing.assert_close(g, w.to(td), msg=lambda m: f"{what} {name}: {m}", **t)  # every element
            continue
        w32, names32, _ = fused_run(inp, pm, ac, cast=torch.float32)
        assert names32 == hd.FUSED_NAMES[family], (what, names32)
        assert_16_bit_close(storage, got, w32, inp["value"].dtype, what)
