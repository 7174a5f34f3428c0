"""Generators, slice arithmetic and references for tests/test_gpu_large_offsets.py: tensors whose bytes cross 2^31 and
2^32.  A helper module, not a conftest.

Batch elements are independent, and so are queries for everything but grad_value.  So a tensor that crosses a mark is
held to the fp64 CPU oracle only on a handful of slices — the first, the last, and the slices before, at and behind each
mark, computed HERE from the shapes (`mark_slices`, which asserts that they exist) — while the rest is checked cheaply
on the device.  Inputs are the dyadic numbers of tests/exact_cases.py, generated on the GPU for the big tensors, so the
compared slices can be held with `torch.equal` wherever the float32 oracle equals the float64 oracle bitwise (asserted
per slice by `reference`); a slice that cannot meet that takes the fp32 tolerances of tests/test_gpu_parity.py."""
import math

import numpy as np
import pytest
import torch

import exact_cases as ec

MARKS = (1 << 31, 1 << 32)
BUDGET = 32 << 30  # bytes of device memory one test may hold
FWD_TOL = dict(atol=1e-4, rtol=1e-3)   # tests/test_gpu_parity.py: FWD_TOL / BWD_TOL for float32
BWD_TOL = dict(atol=1e-3, rtol=1e-2)
MODES = [("zeros", False), ("border", True)]
DEV = "cuda:0"


# ----------------------------------------------------------------------------------------- memory
def nbytes(shape, elem):
    return math.prod(shape) * elem


def claim_memory(need, what):
    """`need`: bytes the test holds at once, computed from its shapes.  Asserts the budget; skips only when the device
    reports less free memory than that."""
    assert need <= BUDGET, f"{what}: needs {need} bytes, the budget is {BUDGET}"
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip(f"{what}: needs {need} bytes of device memory, {free} are free")


# ----------------------------------------------------------------------------------------- slices at the marks
def mark_slices(n, slice_bytes, marks, what):
    """A tensor of `n` equal slices of `slice_bytes` bytes: the indices of the first and the last slice and, for each
    mark, of the slice that holds the mark's byte (it straddles the mark, or starts on it) and its two neighbours.
    Asserts that the tensor crosses every mark it is said to cross, with a whole slice on either side."""
    keep = {0, n - 1}
    for m in marks:
        k = m // slice_bytes
        assert 1 <= k and k + 1 <= n - 1, f"{what}: {n} slices of {slice_bytes} bytes do not cross {m} with a slice on either side"
        assert (k - 1) * slice_bytes < m and (k + 1) * slice_bytes >= m  # before / behind the mark
        keep |= {k - 1, k, k + 1}
    return sorted(keep)


def queries_at_marks(B, Q, tensors, what):
    """`tensors`: {name: (bytes per (b, q) slice, marks it crosses)}.  -> {b: sorted query indices}: the (b, q) slices
    of mark_slices for every tensor, plus the first and the last query of every batch element."""
    picked = {b: {0, Q - 1} for b in range(B)}
    for name, (qbytes, marks) in tensors.items():
        for g in mark_slices(B * Q, qbytes, marks, f"{what}: {name}"):
            picked[g // Q].add(g % Q)
    return {b: sorted(q) for b, q in picked.items()}


# ----------------------------------------------------------------------------------------- dyadic inputs on the device
def dev_odd_multiples(shape, bits, lo, hi, gen, chunks=1):
    """exact_cases._odd_multiples on the device, float32: odd multiples of 2^-bits in [lo, hi].  `chunks`: slices of the
    leading axis generated at a time (keeps the integer temporaries small)."""
    scale = 2 ** bits
    kmin, kmax = math.ceil((lo * scale - 1) / 2), math.floor((hi * scale - 1) / 2)
    out = torch.empty(shape, dtype=torch.float32, device=DEV)
    for part in out.chunk(chunks, 0):
        k = torch.randint(kmin, kmax + 1, part.shape, dtype=torch.int32, device=DEV, generator=gen)
        torch.mul(k, 2.0 / scale, out=part)
        part += 1.0 / scale
    return out


def dev_grid(shape, vmax, bits, gen, dtype=torch.float32, chunks=1):
    """exact_cases._grid on the device: multiples of 2^-bits in [-vmax, vmax]."""
    scale = 2 ** bits
    out = torch.empty(shape, dtype=dtype, device=DEV)
    for part in out.chunk(chunks, 0):
        k = torch.randint(-vmax * scale, vmax * scale + 1, part.shape, dtype=torch.int32, device=DEV, generator=gen)
        part.copy_(k.to(torch.float32) / scale)
    return out


def dev_weights(shape, bits, gen, chunks=1):
    """Attention weights: multiples of 2^-bits in [0, 1]."""
    scale = 2 ** bits
    out = torch.empty(shape, dtype=torch.float32, device=DEV)
    for part in out.chunk(chunks, 0):
        k = torch.randint(0, scale + 1, part.shape, dtype=torch.int32, device=DEV, generator=gen)
        torch.mul(k, 1.0 / scale, out=part)
    return out


def generator(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


# ----------------------------------------------------------------------------------------- the reference of a slice
def _np64(t):
    return t.detach().to("cpu", torch.float64).numpy()


def reference(value, shapes, loc, attn, grad_out, pm, ac, counts=None):
    """fp64 oracle results of a small (sub-)problem given as tensors or arrays, as {out, grad_value, grad_loc, grad_attn},
    and whether the float32 oracle reproduces them bitwise (the exact_cases precondition: then a correct float32 kernel
    must EQUAL them).  `counts`: per-level point counts (loc [B, Q, H, S, 2])."""
    c = dict(value=_np64(value), shapes=np.asarray(shapes, dtype=np.int64), loc=_np64(loc), attn=_np64(attn),
             grad_out=_np64(grad_out), bits=dict(loc=7, attn=0, value=0, grad=0))  # (loc: where `dense` puts a ragged case's padding)
    if counts is not None:
        c["counts"] = [int(p) for p in counts]
    oracle = ec._oracle()
    r64 = ec._oracle_all(oracle, c, pm, ac, np.float64)
    r32 = ec._oracle_all(oracle, c, pm, ac, np.float32)
    exact = all(np.array_equal(r32[k].astype(np.float64), r64[k]) for k in r64)
    return r64, exact


def assert_matches(got, ref64, exact, what, forward=False):
    """`got` (a device or host tensor) against the fp64 reference: equal to it rounded once to got's type where the
    slice is exact, within the parity file's float32 tolerance where it is not."""
    got = got.detach().cpu()
    want = torch.from_numpy(np.ascontiguousarray(ref64))
    assert tuple(got.shape) == tuple(want.shape), (what, got.shape, want.shape)
    if exact:
        want = want.to(torch.float32).to(got.dtype)
        if not torch.equal(got, want):
            ne = got != want
            raise AssertionError(f"{what}: {int(ne.sum())} of {ne.numel()} elements differ from the exact reference, "
                                 f"largest difference {float((got.double() - want.double()).abs().max())}")
    else:
        assert got.dtype == torch.float32, (what, got.dtype)
        np.testing.assert_allclose(got.double().numpy(), want.numpy(), err_msg=what, **(FWD_TOL if forward else BWD_TOL))


def touched_rows(loc, levels, ac, counts=None):
    """[B, I, H] bool on the device: the pixels whose (b, pixel, h) row some sample of `loc` can touch — the four corners
    of its bilinear cell, clamped to the level (what "border" padding reads; "zeros" touches a subset)."""
    B, Q, H = loc.shape[:3]
    I = sum(h * w for h, w in levels)  # noqa: E741
    hit = torch.zeros(B * I * H, dtype=torch.bool, device=loc.device)
    bidx = torch.arange(B, device=loc.device).reshape(B, 1, 1, 1)
    hidx = torch.arange(H, device=loc.device).reshape(1, 1, H, 1)
    start = s0 = 0
    for lvl, (h, w) in enumerate(levels):
        pts = loc[:, :, :, lvl] if counts is None else loc[:, :, :, s0:s0 + counts[lvl]]
        x = pts[..., 0].double() * (w - 1) if ac else pts[..., 0].double() * w - 0.5
        y = pts[..., 1].double() * (h - 1) if ac else pts[..., 1].double() * h - 0.5
        x0, y0 = torch.floor(x).long(), torch.floor(y).long()
        for oy in (0, 1):
            for ox in (0, 1):
                pix = start + (y0 + oy).clamp(0, h - 1) * w + (x0 + ox).clamp(0, w - 1)
                hit[((bidx * I + pix) * H + hidx).reshape(-1)] = True
        start += h * w
        s0 += 0 if counts is None else counts[lvl]
    return hit.reshape(B, I, H)
