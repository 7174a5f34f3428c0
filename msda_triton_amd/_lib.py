"""ctypes binding of ``libmsda_hip.so`` — the C ABI declared in ``include/msda_hip.h``.

The library is built in-tree by ``msda_triton_amd/csrc/Makefile`` (``__graft_entry__.build()``)
and lives next to this file.  There is no fallback: if it is missing, every GPU call raises.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_NAME = "libmsda_hip.so"
LIB_PATH = os.path.join(_HERE, LIB_NAME)
CSRC_DIR = os.path.join(_HERE, "csrc")

ABI_VERSION = 12
PADDING_MODES = {"border": 0, "zeros": 1}
WS_RECORDS_IN_GRADS = 1  # msda_bwd_workspace_bytes flag (include/msda_hip.h)


def ws_passes(n: int) -> int:
    """msda_bwd_workspace_bytes flag MSDA_WS_PASSES(n): the size for n passes over the batch (include/msda_hip.h)."""
    return (int(n) & 0xFF) << 8


# one storage type for every tensor, then the mixed ones: value / grad_value in 16 bits, everything else fp32
DTYPE_SUFFIXES = ("f32", "f16", "bf16", "f64", "f32_vbf16", "f32_vf16")
# module storage (fused entry points only): value, projection, out and their gradients in 16 bits, reference points fp32
FUSED_STORAGE_SUFFIXES = ("f32_sbf16", "f32_sf16")

# every symbol include/msda_hip.h declares
EXPORTED_SYMBOLS = tuple(
    [f"msda_{d}_{s}" for d in ("fwd", "bwd", "fwd_fused", "bwd_fused") for s in DTYPE_SUFFIXES]
    + [f"msda_{d}_{s}" for d in ("fwd_fused", "bwd_fused") for s in FUSED_STORAGE_SUFFIXES]
    + [f"msda_{d}_ragged_{s}" for d in ("fwd", "bwd") for s in DTYPE_SUFFIXES]
    + ["msda_bwd_ragged_workspace_bytes", "msda_bwd_ragged_supported"]
    + [f"msda_{d}_discrete_{s}" for d in ("fwd", "bwd") for s in DTYPE_SUFFIXES]
    + ["msda_bwd_discrete_workspace_bytes", "msda_bwd_discrete_supported"]
    + [f"msda_{d}_fused_ragged_{s}" for d in ("fwd", "bwd") for s in DTYPE_SUFFIXES + FUSED_STORAGE_SUFFIXES]
    + ["msda_bwd_fused_ragged_workspace_bytes"]
    + [f"msda_{d}_fused_levelref_{s}" for d in ("fwd", "bwd") for s in DTYPE_SUFFIXES + FUSED_STORAGE_SUFFIXES]
    + [f"msda_{d}_fused_hfbox_{s}" for d in ("fwd", "bwd") for s in DTYPE_SUFFIXES + FUSED_STORAGE_SUFFIXES]
    + [f"msda_{d}_masked_{s}" for d in ("fwd", "bwd") for s in DTYPE_SUFFIXES]
    + [f"msda_{d}_fused_levelref_masked_{s}" for d in ("fwd", "bwd") for s in DTYPE_SUFFIXES + FUSED_STORAGE_SUFFIXES]
    + ["msda_abi_version", "msda_last_error", "msda_set_option", "msda_get_option", "msda_bwd_workspace_bytes",
       "msda_bwd_fused_workspace_bytes", "msda_bwd_supported", "msda_fused_lp_limit", "msda_profile_read",
       "msda_last_launch_info"]
)

# ... and the query-mask entry points (has_query_mask): the _masked_ families' kernels with `query_mask` behind `value_mask`
QUERY_MASK_SYMBOLS = tuple(
    [f"msda_{d}_qmasked_{s}" for d in ("fwd", "bwd") for s in DTYPE_SUFFIXES]
    + [f"msda_{d}_fused_levelref_qmasked_{s}" for d in ("fwd", "bwd") for s in DTYPE_SUFFIXES + FUSED_STORAGE_SUFFIXES]
)

# ... and Hugging Face's box rule in front of discrete sampling (has_fused_hfbox_discrete): the hfbox pair's suffixes
HFBOX_DISCRETE_SYMBOLS = tuple(
    [f"msda_{d}_fused_hfbox_discrete_{s}" for d in ("fwd", "bwd") for s in DTYPE_SUFFIXES + FUSED_STORAGE_SUFFIXES]
    + ["msda_bwd_fused_hfbox_discrete_workspace_bytes"]
)

# ... and both padding masks inside the module's own fused pairs (has_module_masks): the fused and the fused ragged pairs'
# lists with `value_mask`, `query_mask` behind `value`
MODULE_MASK_SYMBOLS = tuple(
    [f"msda_{d}_fused_masked_{s}" for d in ("fwd", "bwd") for s in DTYPE_SUFFIXES + FUSED_STORAGE_SUFFIXES]
    + [f"msda_{d}_fused_ragged_masked_{s}" for d in ("fwd", "bwd") for s in DTYPE_SUFFIXES + FUSED_STORAGE_SUFFIXES]
)

# ... and the reference module's own rule in front of discrete sampling (has_module_discrete): the same suffixes
MODULE_DISCRETE_SYMBOLS = tuple(
    [f"msda_{d}_fused_discrete_{s}" for d in ("fwd", "bwd") for s in DTYPE_SUFFIXES + FUSED_STORAGE_SUFFIXES]
    + ["msda_bwd_fused_discrete_workspace_bytes"]
)

# ... and the per-level-reference pair on split projections (has_levelref_split): `offsets`, `logits` in place of `proj`
LEVELREF_SPLIT_SYMBOLS = tuple(
    f"msda_{d}_fused_levelref_split_{s}" for d in ("fwd", "bwd") for s in DTYPE_SUFFIXES + FUSED_STORAGE_SUFFIXES
)

_lib = None
_lock = threading.Lock()


class MSDALibraryError(RuntimeError):
    """libmsda_hip.so is missing/unloadable, or a call into it failed."""


def build(verbose: bool = False, jobs: int = 5) -> str:
    """Compile the HIP sources for gfx950 with hipcc (cross-compiles without a GPU)."""
    cmd = ["make", "-C", CSRC_DIR, f"-j{jobs}"]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if verbose or res.returncode != 0:
        print(res.stdout)
    if res.returncode != 0:
        raise MSDALibraryError(f"building {LIB_NAME} failed (exit {res.returncode})")
    return LIB_PATH


def load():
    """Load (once) and return the ctypes handle; raises MSDALibraryError if unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise MSDALibraryError(
                f"{LIB_PATH} not found: the HIP extension has not been built. Run "
                f"`python -c 'import __graft_entry__ as g; g.build()'` or `make -C {CSRC_DIR}`. "
                "There is no CPU fallback for GPU tensors."
            )
        try:
            lib = ctypes.CDLL(LIB_PATH)
        except OSError as e:  # e.g. libamdhip64 missing
            raise MSDALibraryError(f"cannot load {LIB_PATH}: {e}") from e
        i64, vp, ci = ctypes.c_int64, ctypes.c_void_p, ctypes.c_int
        for suf in DTYPE_SUFFIXES:
            f = getattr(lib, f"msda_fwd_{suf}")
            f.restype = ci
            # (..., padding_mode, align_corners, value_row_stride, stream)
            f.argtypes = [vp] * 5 + [i64] * 7 + [ci, ci, i64, vp]
            ff = getattr(lib, f"msda_fwd_fused_{suf}")
            ff.restype = ci
            ff.argtypes = [vp] * 5 + [i64] * 7 + [ci, ci, ci, i64, vp]
            # the backward: (..., max_level_cells, value_row_stride, workspace, workspace_bytes, stream)
            g = getattr(lib, f"msda_bwd_{suf}")
            g.restype = ci
            g.argtypes = [vp] * 8 + [i64] * 7 + [ci, ci, i64, i64, vp, i64, vp]
            gf = getattr(lib, f"msda_bwd_fused_{suf}")
            gf.restype = ci
            gf.argtypes = [vp] * 8 + [i64] * 7 + [ci, ci, ci, i64, i64, vp, i64, vp]
            # per-level point counts (ABI 12): P becomes a host int32 array of L counts
            fr = getattr(lib, f"msda_fwd_ragged_{suf}")
            fr.restype = ci
            fr.argtypes = [vp] * 5 + [i64] * 6 + [vp, ci, ci, i64, vp]
            gr = getattr(lib, f"msda_bwd_ragged_{suf}")
            gr.restype = ci
            gr.argtypes = [vp] * 8 + [i64] * 6 + [vp, ci, ci, i64, i64, vp, i64, vp]
        for suf in FUSED_STORAGE_SUFFIXES:
            ff = getattr(lib, f"msda_fwd_fused_{suf}")
            ff.restype = ci
            ff.argtypes = [vp] * 5 + [i64] * 7 + [ci, ci, ci, i64, vp]
            gf = getattr(lib, f"msda_bwd_fused_{suf}")
            gf.restype = ci
            gf.argtypes = [vp] * 8 + [i64] * 7 + [ci, ci, ci, i64, i64, vp, i64, vp]
        lib.msda_bwd_workspace_bytes.restype = i64
        lib.msda_bwd_workspace_bytes.argtypes = [i64] * 7 + [ci, ci, i64, ci]
        lib.msda_bwd_fused_workspace_bytes.restype = i64
        lib.msda_bwd_fused_workspace_bytes.argtypes = [i64] * 7 + [ci, ci, i64, ci]
        lib.msda_bwd_supported.restype = ci
        lib.msda_bwd_supported.argtypes = [i64] * 7 + [ci]
        lib.msda_bwd_ragged_workspace_bytes.restype = i64
        lib.msda_bwd_ragged_workspace_bytes.argtypes = [i64] * 6 + [vp, ci, ci, i64, ci]
        lib.msda_bwd_ragged_supported.restype = ci
        lib.msda_bwd_ragged_supported.argtypes = [i64] * 6 + [vp, ci]
        # discrete sampling: additions within ABI 12, so a library built before them lacks the symbols (has_discrete)
        if hasattr(lib, "msda_bwd_discrete_supported"):
            for suf in DTYPE_SUFFIXES:
                fd = getattr(lib, f"msda_fwd_discrete_{suf}")
                fd.restype = ci
                # (value, shapes, loc, attn, out, B, I, H, D, Q, L, points_per_level, value_row_stride, stream)
                fd.argtypes = [vp] * 5 + [i64] * 6 + [vp, i64, vp]
                gd = getattr(lib, f"msda_bwd_discrete_{suf}")
                gd.restype = ci
                # (grad_out, value, shapes, loc, attn, grad_value, grad_attn, B ... L, points_per_level, max_level_cells,
                #  value_row_stride, workspace, workspace_bytes, stream)
                gd.argtypes = [vp] * 7 + [i64] * 6 + [vp, i64, i64, vp, i64, vp]
            lib.msda_bwd_discrete_workspace_bytes.restype = i64
            lib.msda_bwd_discrete_workspace_bytes.argtypes = [i64] * 6 + [vp, ci, ci, i64, ci]
            lib.msda_bwd_discrete_supported.restype = ci
            lib.msda_bwd_discrete_supported.argtypes = [i64] * 6 + [vp, ci]
        # the module's fused pair with per-level point counts: additions within ABI 12 too (has_fused_ragged)
        if hasattr(lib, "msda_bwd_fused_ragged_workspace_bytes"):
            for suf in DTYPE_SUFFIXES + FUSED_STORAGE_SUFFIXES:
                ffr = getattr(lib, f"msda_fwd_fused_ragged_{suf}")
                ffr.restype = ci
                # (value, shapes, proj, ref, out, B, I, H, D, Q, L, points_per_level, ref_dim, padding_mode, align_corners,
                #  value_row_stride, stream)
                ffr.argtypes = [vp] * 5 + [i64] * 6 + [vp, ci, ci, ci, i64, vp]
                gfr = getattr(lib, f"msda_bwd_fused_ragged_{suf}")
                gfr.restype = ci
                gfr.argtypes = [vp] * 8 + [i64] * 6 + [vp, ci, ci, ci, i64, i64, vp, i64, vp]
            lib.msda_bwd_fused_ragged_workspace_bytes.restype = i64
            lib.msda_bwd_fused_ragged_workspace_bytes.argtypes = [i64] * 6 + [vp, ci, ci, i64, ci]
        # the module's fused pair for per-level reference points (transformers' prologue): additions within ABI 12 as
        # well (has_fused_levelref); the argument lists of the uniform fused pair
        if hasattr(lib, "msda_bwd_fused_levelref_f32"):
            for suf in DTYPE_SUFFIXES + FUSED_STORAGE_SUFFIXES:
                ffl = getattr(lib, f"msda_fwd_fused_levelref_{suf}")
                ffl.restype = ci
                ffl.argtypes = [vp] * 5 + [i64] * 7 + [ci, ci, ci, i64, vp]
                gfl = getattr(lib, f"msda_bwd_fused_levelref_{suf}")
                gfl.restype = ci
                gfl.argtypes = [vp] * 8 + [i64] * 7 + [ci, ci, ci, i64, i64, vp, i64, vp]
        # the module's fused pair for Hugging Face's box rule with per-level counts (D-FINE, DEIMv2, RT-DETRv2): additions
        # within ABI 12 (has_fused_hfbox); the fused ragged pair's lists with (level_scale, offset_scale) behind the counts
        if hasattr(lib, "msda_bwd_fused_hfbox_f32"):
            cd = ctypes.c_double
            for suf in DTYPE_SUFFIXES + FUSED_STORAGE_SUFFIXES:
                ffh = getattr(lib, f"msda_fwd_fused_hfbox_{suf}")
                ffh.restype = ci
                ffh.argtypes = [vp] * 5 + [i64] * 6 + [vp, vp, cd, ci, ci, ci, i64, vp]
                gfh = getattr(lib, f"msda_bwd_fused_hfbox_{suf}")
                gfh.restype = ci
                gfh.argtypes = [vp] * 8 + [i64] * 6 + [vp, vp, cd, ci, ci, ci, i64, i64, vp, i64, vp]
        # the value-mask twins: additions within ABI 12 (has_value_mask); the twins' lists with `value_mask` behind `value`
        if hasattr(lib, "msda_bwd_masked_f32"):
            for suf in DTYPE_SUFFIXES:
                fm = getattr(lib, f"msda_fwd_masked_{suf}")
                fm.restype = ci
                fm.argtypes = [vp] * 6 + [i64] * 7 + [ci, ci, i64, vp]
                gm = getattr(lib, f"msda_bwd_masked_{suf}")
                gm.restype = ci
                gm.argtypes = [vp] * 9 + [i64] * 7 + [ci, ci, i64, i64, vp, i64, vp]
            for suf in DTYPE_SUFFIXES + FUSED_STORAGE_SUFFIXES:
                flm = getattr(lib, f"msda_fwd_fused_levelref_masked_{suf}")
                flm.restype = ci
                flm.argtypes = [vp] * 6 + [i64] * 7 + [ci, ci, ci, i64, vp]
                glm = getattr(lib, f"msda_bwd_fused_levelref_masked_{suf}")
                glm.restype = ci
                glm.argtypes = [vp] * 9 + [i64] * 7 + [ci, ci, ci, i64, i64, vp, i64, vp]
        # the query-mask entry points: additions within ABI 12 (has_query_mask); the _masked_ twins' lists with `query_mask`
        # behind `value_mask`
        if hasattr(lib, "msda_bwd_qmasked_f32"):
            for suf in DTYPE_SUFFIXES:
                fq = getattr(lib, f"msda_fwd_qmasked_{suf}")
                fq.restype = ci
                fq.argtypes = [vp] * 7 + [i64] * 7 + [ci, ci, i64, vp]
                gq = getattr(lib, f"msda_bwd_qmasked_{suf}")
                gq.restype = ci
                gq.argtypes = [vp] * 10 + [i64] * 7 + [ci, ci, i64, i64, vp, i64, vp]
            for suf in DTYPE_SUFFIXES + FUSED_STORAGE_SUFFIXES:
                flq = getattr(lib, f"msda_fwd_fused_levelref_qmasked_{suf}")
                flq.restype = ci
                flq.argtypes = [vp] * 7 + [i64] * 7 + [ci, ci, ci, i64, vp]
                glq = getattr(lib, f"msda_bwd_fused_levelref_qmasked_{suf}")
                glq.restype = ci
                glq.argtypes = [vp] * 10 + [i64] * 7 + [ci, ci, ci, i64, i64, vp, i64, vp]
        # the box rule in front of discrete sampling: additions within ABI 12 (has_fused_hfbox_discrete); the hfbox pair's
        # lists without ref_dim, padding_mode, align_corners and grad_ref_partial
        if hasattr(lib, "msda_bwd_fused_hfbox_discrete_workspace_bytes"):
            cd = ctypes.c_double
            for suf in DTYPE_SUFFIXES + FUSED_STORAGE_SUFFIXES:
                fhd = getattr(lib, f"msda_fwd_fused_hfbox_discrete_{suf}")
                fhd.restype = ci
                # (value, shapes, proj, ref, out, B ... L, points_per_level, level_scale, offset_scale, value_row_stride, stream)
                fhd.argtypes = [vp] * 5 + [i64] * 6 + [vp, vp, cd, i64, vp]
                ghd = getattr(lib, f"msda_bwd_fused_hfbox_discrete_{suf}")
                ghd.restype = ci
                # (grad_out, value, shapes, proj, ref, grad_value, grad_proj, B ... L, points_per_level, level_scale,
                #  offset_scale, max_level_cells, value_row_stride, workspace, workspace_bytes, stream)
                ghd.argtypes = [vp] * 7 + [i64] * 6 + [vp, vp, cd, i64, i64, vp, i64, vp]
            lib.msda_bwd_fused_hfbox_discrete_workspace_bytes.restype = i64
            lib.msda_bwd_fused_hfbox_discrete_workspace_bytes.argtypes = [i64] * 6 + [vp, ci, ci, i64, ci]
        # the module's own rule in front of discrete sampling: additions within ABI 12 (has_module_discrete); the
        # hfbox-discrete pair's lists with `int ref_dim` in place of (level_scale, offset_scale)
        if hasattr(lib, "msda_bwd_fused_discrete_workspace_bytes"):
            for suf in DTYPE_SUFFIXES + FUSED_STORAGE_SUFFIXES:
                fmd = getattr(lib, f"msda_fwd_fused_discrete_{suf}")
                fmd.restype = ci
                # (value, shapes, proj, ref, out, B ... L, points_per_level, ref_dim, value_row_stride, stream)
                fmd.argtypes = [vp] * 5 + [i64] * 6 + [vp, ci, i64, vp]
                gmd = getattr(lib, f"msda_bwd_fused_discrete_{suf}")
                gmd.restype = ci
                # (grad_out, value, shapes, proj, ref, grad_value, grad_proj, B ... L, points_per_level, ref_dim,
                #  max_level_cells, value_row_stride, workspace, workspace_bytes, stream)
                gmd.argtypes = [vp] * 7 + [i64] * 6 + [vp, ci, i64, i64, vp, i64, vp]
            lib.msda_bwd_fused_discrete_workspace_bytes.restype = i64
            lib.msda_bwd_fused_discrete_workspace_bytes.argtypes = [i64] * 6 + [vp, ci, ci, i64, ci]
        # both masks inside the module's own fused pairs: additions within ABI 12 (has_module_masks); the fused / fused
        # ragged pairs' lists with `value_mask`, `query_mask` behind `value`
        if hasattr(lib, "msda_bwd_fused_ragged_masked_f32"):
            for suf in DTYPE_SUFFIXES + FUSED_STORAGE_SUFFIXES:
                fmm = getattr(lib, f"msda_fwd_fused_masked_{suf}")
                fmm.restype = ci
                fmm.argtypes = [vp] * 7 + [i64] * 7 + [ci, ci, ci, i64, vp]
                gmm = getattr(lib, f"msda_bwd_fused_masked_{suf}")
                gmm.restype = ci
                gmm.argtypes = [vp] * 10 + [i64] * 7 + [ci, ci, ci, i64, i64, vp, i64, vp]
                frm = getattr(lib, f"msda_fwd_fused_ragged_masked_{suf}")
                frm.restype = ci
                frm.argtypes = [vp] * 7 + [i64] * 6 + [vp, ci, ci, ci, i64, vp]
                grm = getattr(lib, f"msda_bwd_fused_ragged_masked_{suf}")
                grm.restype = ci
                grm.argtypes = [vp] * 10 + [i64] * 6 + [vp, ci, ci, ci, i64, i64, vp, i64, vp]
        # the per-level-reference pair on split projections: additions within ABI 12 (has_levelref_split); that pair's
        # lists with (offsets, logits) in place of `proj` and (grad_offsets, grad_logits) in place of `grad_proj`
        if hasattr(lib, "msda_bwd_fused_levelref_split_f32"):
            for suf in DTYPE_SUFFIXES + FUSED_STORAGE_SUFFIXES:
                fls = getattr(lib, f"msda_fwd_fused_levelref_split_{suf}")
                fls.restype = ci
                fls.argtypes = [vp] * 6 + [i64] * 7 + [ci, ci, ci, i64, vp]
                gls = getattr(lib, f"msda_bwd_fused_levelref_split_{suf}")
                gls.restype = ci
                gls.argtypes = [vp] * 10 + [i64] * 7 + [ci, ci, ci, i64, i64, vp, i64, vp]
        lib.msda_profile_read.restype = ci
        lib.msda_profile_read.argtypes = [ctypes.c_char_p, ci]
        lib.msda_fused_lp_limit.restype = i64
        lib.msda_fused_lp_limit.argtypes = [i64, ci]
        lib.msda_abi_version.restype = ci
        lib.msda_last_error.restype = ctypes.c_char_p
        lib.msda_set_option.restype = ci
        lib.msda_set_option.argtypes = [ctypes.c_char_p, ci]
        lib.msda_get_option.restype = ci
        lib.msda_get_option.argtypes = [ctypes.c_char_p]
        lib.msda_last_launch_info.restype = ci
        lib.msda_last_launch_info.argtypes = [ctypes.c_char_p]
        got = lib.msda_abi_version()
        if got != ABI_VERSION:
            raise MSDALibraryError(f"{LIB_NAME} has ABI version {got}, this package expects {ABI_VERSION}; rebuild it")
        _lib = lib
    return _lib


def load_discrete():
    """The handle, for a discrete-sampling call: raises when the loaded library predates those entry points (they are
    additions within ABI 12, found by symbol)."""
    lib = load()
    if not hasattr(lib, "msda_bwd_discrete_supported"):
        raise MSDALibraryError(f"{LIB_PATH} has no discrete-sampling entry points (msda_fwd_discrete_<dtype> ...): it "
                               "was built from older sources; rebuild the library")
    return lib


def has_fused_ragged() -> bool:
    """Does the loaded library have the fused module pair for per-level point counts (msda_fwd_fused_ragged_<dtype> ...,
    additions within ABI 12, found by symbol)?  Without them the caller composes the prologue around the ragged operator."""
    return hasattr(load(), "msda_bwd_fused_ragged_workspace_bytes")


def has_fused_levelref() -> bool:
    """Does the loaded library have the fused module pair for per-level reference points
    (msda_fwd_fused_levelref_<dtype> ..., additions within ABI 12, found by symbol)?  Without them the caller composes
    transformers' prologue around the plain operator."""
    return hasattr(load(), "msda_bwd_fused_levelref_f32")


def has_fused_hfbox() -> bool:
    """Does the loaded library have the fused module pair for Hugging Face's box rule with per-level point counts
    (msda_fwd_fused_hfbox_<dtype> ..., additions within ABI 12, found by symbol)?  Without them the caller composes
    transformers' prologue around the ragged operator."""
    return hasattr(load(), "msda_bwd_fused_hfbox_f32")


def has_fused_hfbox_discrete() -> bool:
    """Does the loaded library have the box rule's pair for discrete sampling (msda_fwd_fused_hfbox_discrete_<dtype> ...,
    additions within ABI 12, found by symbol)?  Without them the caller composes transformers' prologue around the
    discrete operator."""
    return hasattr(load(), "msda_bwd_fused_hfbox_discrete_workspace_bytes")


def has_module_discrete() -> bool:
    """Does the loaded library have the reference module's rule in front of discrete sampling
    (msda_fwd_fused_discrete_<dtype> ..., additions within ABI 12, found by symbol)?  Without them the caller composes the
    module's prologue around the discrete operator."""
    return hasattr(load(), "msda_bwd_fused_discrete_workspace_bytes")


def has_levelref_split() -> bool:
    """Does the loaded library have the per-level-reference pair on split projections
    (msda_fwd_fused_levelref_split_<dtype> ..., additions within ABI 12, found by symbol)?  Without them the caller
    interleaves offsets and logits and takes the pair it has."""
    return hasattr(load(), "msda_bwd_fused_levelref_split_f32")


def has_value_mask() -> bool:
    """Does the loaded library have the value-mask twins (msda_fwd_masked_<dtype> ..., msda_fwd_fused_levelref_masked_<dtype>
    ..., additions within ABI 12, found by symbol)?  Without them a masked call composes ``masked_fill`` with the unmasked
    route."""
    return hasattr(load(), "msda_bwd_masked_f32")


def has_query_mask() -> bool:
    """Does the loaded library have the query-mask entry points (msda_fwd_qmasked_<dtype> ...,
    msda_fwd_fused_levelref_qmasked_<dtype> ..., additions within ABI 12, found by symbol)?  Without them a call with a
    query mask composes ``functional.apply_query_mask`` with its route."""
    return hasattr(load(), "msda_bwd_qmasked_f32")


def has_module_masks() -> bool:
    """Does the loaded library have the module's own fused pairs with both padding masks (msda_fwd_fused_masked_<dtype> ...,
    msda_fwd_fused_ragged_masked_<dtype> ..., additions within ABI 12, found by symbol)?  Without them a masked module call
    composes ``apply_value_mask`` / ``apply_query_mask`` with the unmasked fused route."""
    return hasattr(load(), "msda_bwd_fused_ragged_masked_f32")


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().msda_last_error().decode(errors="replace")
        if rc < 0:
            raise ValueError(f"{what}: rejected arguments ({rc}): {msg}")
        raise MSDALibraryError(f"{what}: HIP error {rc}: {msg}")


OPTION_EPOCH = 0  # bumped by set_option: callers that cache option-dependent values (workspace sizes) key on it


def set_option(key: str, value: int) -> None:
    global OPTION_EPOCH
    check(load().msda_set_option(key.encode(), int(value)), f"msda_set_option({key})")
    OPTION_EPOCH += 1


def get_option(key: str) -> int:
    return int(load().msda_get_option(key.encode()))


LAUNCH_INFO_KEYS = ("fwd_variant", "fwd_lds_level_bytes", "fwd_lds_planes", "fwd_workgroups", "sample_variant",
                    "sample_lds_level_bytes", "value_path", "value_passes", "fwd_vec", "fwd_group", "fwd_chunks",
                    "sample_vec", "sample_group", "sample_chunks", "value_vec", "value_group", "value_chunks",
                    "fwd_trips", "sample_trips",
                    "value_cell_cap", "value_place_cells", "value_place_variant", "value_slices", "value_rounds", "value_win",
                    "grid_xcd3d_launches", "grid_linear2d_launches", "grid_flat_launches")
# the last three are counters (launches per grid form since the process started): callers take differences around a call
GRID_FORM_KEYS = LAUNCH_INFO_KEYS[-3:]


def last_launch_info() -> dict:
    """Which variants the most recent launches took (measurement only; include/msda_hip.h msda_last_launch_info)."""
    lib = load()
    return {k: int(lib.msda_last_launch_info(k.encode())) for k in LAUNCH_INFO_KEYS}


def profile_read() -> dict:
    """{kernel name: (launches, mean microseconds)} of the kernels launched (by any thread) since the last read while
    option "profile" was 1 (measurement only; synchronises on the recorded events)."""
    lib = load()
    buf = ctypes.create_string_buffer(1 << 16)  # (one call: the read consumes the records)
    lib.msda_profile_read(buf, len(buf))
    out = {}
    for line in buf.value.decode().splitlines():
        name, launches, total = line.rsplit(" ", 2)
        out[name] = (int(launches), float(total) / max(int(launches), 1))
    return out
