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

_ALL_SUFFIXES = DTYPE_SUFFIXES + FUSED_STORAGE_SUFFIXES
_I64, _VP, _CI, _CD = ctypes.c_int64, ctypes.c_void_p, ctypes.c_int, ctypes.c_double
_P, _COUNTS = _I64, _VP            # behind B, I, H, D, Q, L: `int64 P`, or the host array `points_per_level`
_SAMPLING, _DISCRETE = (_CI, _CI), ()  # padding_mode, align_corners — discrete sampling has neither
_WS, _WS_SUPPORTED = ("workspace_bytes",), ("workspace_bytes", "supported")

# Every kernel family of include/msda_hip.h, once: msda_fwd_<infix>_<suffix> / msda_bwd_<infix>_<suffix>, the size queries
# msda_bwd_<infix>_<query> that go with them, and how the argument lists are composed (_signatures).  A row is
#   (infix, probe, suffixes, forward pointers, backward pointers, P or counts, extras, mode, queries)
# probe:    the symbol whose presence means the library has the family (additions within ABI 12); None: the ABI-12 base set
# pointers: the leading buffers — value, masks, shapes, sampling inputs, out / grad_out ... the gradients
# extras:   what the family puts between the dimensions and the mode — ref_dim; level_scale, offset_scale
_FAMILIES = (
    ("", None, DTYPE_SUFFIXES, 5, 8, _P, (), _SAMPLING, _WS_SUPPORTED),
    ("fused", None, _ALL_SUFFIXES, 5, 8, _P, (_CI,), _SAMPLING, _WS),
    ("ragged", None, DTYPE_SUFFIXES, 5, 8, _COUNTS, (), _SAMPLING, _WS_SUPPORTED),
    ("discrete", "msda_bwd_discrete_supported", DTYPE_SUFFIXES, 5, 7, _COUNTS, (), _DISCRETE, _WS_SUPPORTED),
    ("fused_ragged", "msda_bwd_fused_ragged_workspace_bytes", _ALL_SUFFIXES, 5, 8, _COUNTS, (_CI,), _SAMPLING, _WS),
    ("fused_levelref", "msda_bwd_fused_levelref_f32", _ALL_SUFFIXES, 5, 8, _P, (_CI,), _SAMPLING, ()),
    ("fused_hfbox", "msda_bwd_fused_hfbox_f32", _ALL_SUFFIXES, 5, 8, _COUNTS, (_VP, _CD, _CI), _SAMPLING, ()),
    # `value_mask` behind `value` ...
    ("masked", "msda_bwd_masked_f32", DTYPE_SUFFIXES, 6, 9, _P, (), _SAMPLING, ()),
    ("fused_levelref_masked", "msda_bwd_masked_f32", _ALL_SUFFIXES, 6, 9, _P, (_CI,), _SAMPLING, ()),
    # ... and `query_mask` behind that
    ("qmasked", "msda_bwd_qmasked_f32", DTYPE_SUFFIXES, 7, 10, _P, (), _SAMPLING, ()),
    ("fused_levelref_qmasked", "msda_bwd_qmasked_f32", _ALL_SUFFIXES, 7, 10, _P, (_CI,), _SAMPLING, ()),
    # the prologues in front of discrete sampling: no grad_ref_partial
    ("fused_hfbox_discrete", "msda_bwd_fused_hfbox_discrete_workspace_bytes", _ALL_SUFFIXES, 5, 7, _COUNTS, (_VP, _CD),
     _DISCRETE, _WS),
    ("fused_discrete", "msda_bwd_fused_discrete_workspace_bytes", _ALL_SUFFIXES, 5, 7, _COUNTS, (_CI,), _DISCRETE, _WS),
    # the module's own pairs with both masks behind `value`
    ("fused_masked", "msda_bwd_fused_ragged_masked_f32", _ALL_SUFFIXES, 7, 10, _P, (_CI,), _SAMPLING, ()),
    ("fused_ragged_masked", "msda_bwd_fused_ragged_masked_f32", _ALL_SUFFIXES, 7, 10, _COUNTS, (_CI,), _SAMPLING, ()),
    # (offsets, logits) in place of `proj`, (grad_offsets, grad_logits) in place of `grad_proj`
    ("fused_levelref_split", "msda_bwd_fused_levelref_split_f32", _ALL_SUFFIXES, 6, 10, _P, (_CI,), _SAMPLING, ()),
)
_PROBES = {infix: probe for infix, probe, *_ in _FAMILIES}
_SUFFIXES_OF = {infix: suffixes for infix, _, suffixes, *_ in _FAMILIES}


def _pair(infix: str) -> list:
    return [f"msda_{d}_{infix}_{s}" for d in ("fwd", "bwd") for s in _SUFFIXES_OF[infix]]


# every symbol include/msda_hip.h declares
EXPORTED_SYMBOLS = tuple(
    [f"msda_{d}_{s}" for d in ("fwd", "bwd", "fwd_fused", "bwd_fused") for s in DTYPE_SUFFIXES]
    + [f"msda_{d}_{s}" for d in ("fwd_fused", "bwd_fused") for s in FUSED_STORAGE_SUFFIXES]
    + _pair("ragged") + ["msda_bwd_ragged_workspace_bytes", "msda_bwd_ragged_supported"]
    + _pair("discrete") + ["msda_bwd_discrete_workspace_bytes", "msda_bwd_discrete_supported"]
    + _pair("fused_ragged") + ["msda_bwd_fused_ragged_workspace_bytes"]
    + _pair("fused_levelref") + _pair("fused_hfbox") + _pair("masked") + _pair("fused_levelref_masked")
    + ["msda_abi_version", "msda_last_error", "msda_set_option", "msda_get_option", "msda_bwd_workspace_bytes",
       "msda_bwd_fused_workspace_bytes", "msda_bwd_supported", "msda_fused_lp_limit", "msda_profile_read",
       "msda_last_launch_info"]
)
# ... and the additions within ABI 12 that came after it, each found by its probe:
# the query-mask entry points (has_query_mask)
QUERY_MASK_SYMBOLS = tuple(_pair("qmasked") + _pair("fused_levelref_qmasked"))
# Hugging Face's box rule in front of discrete sampling (has_fused_hfbox_discrete)
HFBOX_DISCRETE_SYMBOLS = tuple(_pair("fused_hfbox_discrete") + ["msda_bwd_fused_hfbox_discrete_workspace_bytes"])
# both padding masks inside the module's own fused pairs (has_module_masks)
MODULE_MASK_SYMBOLS = tuple(_pair("fused_masked") + _pair("fused_ragged_masked"))
# the reference module's own rule in front of discrete sampling (has_module_discrete)
MODULE_DISCRETE_SYMBOLS = tuple(_pair("fused_discrete") + ["msda_bwd_fused_discrete_workspace_bytes"])
# the per-level-reference pair on split projections (has_levelref_split)
LEVELREF_SPLIT_SYMBOLS = tuple(_pair("fused_levelref_split"))


def _signatures(lib):
    """(symbol, restype, argtypes) of every kernel entry point and size query the loaded library has."""
    for infix, probe, suffixes, fwd_ptrs, bwd_ptrs, last_dim, extras, mode, queries in _FAMILIES:
        if probe is not None and not hasattr(lib, probe):
            continue
        dims = [_I64] * 6 + [last_dim]  # B, I, H, D, Q, L, P | points_per_level
        middle = dims + list(extras) + list(mode)
        stem = f"{infix}_" if infix else ""
        for suf in suffixes:
            # (..., value_row_stride, stream)
            yield f"msda_fwd_{stem}{suf}", _CI, [_VP] * fwd_ptrs + middle + [_I64, _VP]
            # (..., max_level_cells, value_row_stride, workspace, workspace_bytes, stream)
            yield f"msda_bwd_{stem}{suf}", _CI, [_VP] * bwd_ptrs + middle + [_I64, _I64, _VP, _I64, _VP]
        if "workspace_bytes" in queries:  # (dims, elem_size, value_elem_size, max_level_cells, flags)
            yield f"msda_bwd_{stem}workspace_bytes", _I64, dims + [_CI, _CI, _I64, _CI]
        if "supported" in queries:  # (dims, elem_size)
            yield f"msda_bwd_{stem}supported", _CI, dims + [_CI]


def _has(infix: str) -> bool:
    return hasattr(load(), _PROBES[infix])


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
        for name, restype, argtypes in _signatures(lib):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
        ci = ctypes.c_int
        lib.msda_profile_read.restype = ci
        lib.msda_profile_read.argtypes = [ctypes.c_char_p, ci]
        lib.msda_fused_lp_limit.restype = ctypes.c_int64
        lib.msda_fused_lp_limit.argtypes = [ctypes.c_int64, ci]
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
    if not hasattr(lib, _PROBES["discrete"]):
        raise MSDALibraryError(f"{LIB_PATH} has no discrete-sampling entry points (msda_fwd_discrete_<dtype> ...): it "
                               "was built from older sources; rebuild the library")
    return lib


def has_fused_ragged() -> bool:
    """Does the loaded library have the fused module pair for per-level point counts (msda_fwd_fused_ragged_<dtype> ...,
    additions within ABI 12, found by symbol)?  Without them the caller composes the prologue around the ragged operator."""
    return _has("fused_ragged")


def has_fused_levelref() -> bool:
    """Does the loaded library have the fused module pair for per-level reference points
    (msda_fwd_fused_levelref_<dtype> ..., additions within ABI 12, found by symbol)?  Without them the caller composes
    transformers' prologue around the plain operator."""
    return _has("fused_levelref")


def has_fused_hfbox() -> bool:
    """Does the loaded library have the fused module pair for Hugging Face's box rule with per-level point counts
    (msda_fwd_fused_hfbox_<dtype> ..., additions within ABI 12, found by symbol)?  Without them the caller composes
    transformers' prologue around the ragged operator."""
    return _has("fused_hfbox")


def has_fused_hfbox_discrete() -> bool:
    """Does the loaded library have the box rule's pair for discrete sampling (msda_fwd_fused_hfbox_discrete_<dtype> ...,
    additions within ABI 12, found by symbol)?  Without them the caller composes transformers' prologue around the
    discrete operator."""
    return _has("fused_hfbox_discrete")


def has_module_discrete() -> bool:
    """Does the loaded library have the reference module's rule in front of discrete sampling
    (msda_fwd_fused_discrete_<dtype> ..., additions within ABI 12, found by symbol)?  Without them the caller composes the
    module's prologue around the discrete operator."""
    return _has("fused_discrete")


def has_levelref_split() -> bool:
    """Does the loaded library have the per-level-reference pair on split projections
    (msda_fwd_fused_levelref_split_<dtype> ..., additions within ABI 12, found by symbol)?  Without them the caller
    interleaves offsets and logits and takes the pair it has."""
    return _has("fused_levelref_split")


def has_value_mask() -> bool:
    """Does the loaded library have the value-mask twins (msda_fwd_masked_<dtype> ..., msda_fwd_fused_levelref_masked_<dtype>
    ..., additions within ABI 12, found by symbol)?  Without them a masked call composes ``masked_fill`` with the unmasked
    route."""
    return _has("masked")


def has_query_mask() -> bool:
    """Does the loaded library have the query-mask entry points (msda_fwd_qmasked_<dtype> ...,
    msda_fwd_fused_levelref_qmasked_<dtype> ..., additions within ABI 12, found by symbol)?  Without them a call with a
    query mask composes ``functional.apply_query_mask`` with its route."""
    return _has("qmasked")


def has_module_masks() -> bool:
    """Does the loaded library have the module's own fused pairs with both padding masks (msda_fwd_fused_masked_<dtype> ...,
    msda_fwd_fused_ragged_masked_<dtype> ..., additions within ABI 12, found by symbol)?  Without them a masked module call
    composes ``apply_value_mask`` / ``apply_query_mask`` with the unmasked fused route."""
    return _has("fused_ragged_masked")


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
