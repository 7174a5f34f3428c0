"""Guarded allocation rig: where do the launchers' kernels write, and do they write everything?

Every device buffer the Python launchers allocate (``out``, the gradients, the per-head ``grad_ref`` partials, the
backward workspace) is a ``torch.empty(..., device=...)``.  Inside ``with GuardedAlloc(fill, device) as rig:`` each such
call on ``device`` is served from the INTERIOR of a larger buffer instead:

    [ front band >= 64 KiB | interior, starts at a multiple of 256 bytes, pre-filled with `fill` | back band >= 64 KiB ]

The bands hold a fixed non-zero byte pattern.  After a device synchronisation ``rig.report()`` says, per allocation, its
shape / dtype / bytes and for either band ``None`` (intact) or the offset of the first modified byte (negative: that many
bytes in front of the interior; non-negative: that many bytes behind its end); ``rig.interiors`` are the tensors handed
out.  Pre-fills: 0xFF (a NaN in every float type here) and 0x5A.

``contract_violations(call, n_alloc, device)`` runs ``call`` three times — plain, rigged with 0xFF, rigged with 0x5A — and
lists everything that breaks the buffer contract: a modified band, a rig that served another number of allocations than
the launcher makes (a rig that was bypassed proves nothing: that is a failure, not a pass), a returned tensor that is not
bit-identical in the three runs (an element that was never written keeps its pre-fill; a scratch table read before it
was written makes the result depend on the pre-fill), a byte of a returned tensor that still holds BOTH pre-fills, and
a non-finite result.

Limit: a band sees a stray store only within 64 KiB of the interior.  A store farther away than that (a wild index,
a wrapped 32-bit offset) lands outside the rig's buffer and is not seen here.
"""
import contextlib

import torch

BAND = 1 << 16  # bytes of guard band on either side, at least
ALIGN = 256     # the interior starts at a multiple of this
FILLS = (0xFF, 0x5A)


def _pattern(lo, hi, device):
    """bytes lo .. hi of the band pattern: position dependent, never 0 (a kernel storing zeros or one repeated byte shows)"""
    return (torch.arange(lo, hi, device=device, dtype=torch.int64) % 251 + 1).to(torch.uint8)


def _size_of(args):
    if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
        return tuple(int(s) for s in args[0])
    return tuple(int(s) for s in args)


class Allocation:
    __slots__ = ("shape", "dtype", "nbytes", "backing", "start", "interior")

    def __init__(self, shape, dtype, nbytes, backing, start, interior):
        self.shape, self.dtype, self.nbytes = shape, dtype, nbytes
        self.backing, self.start, self.interior = backing, start, interior

    def bands(self):
        """(front, back): None when intact, else the first modified byte's offset (see the module docstring)"""
        end, total, dev = self.start + self.nbytes, self.backing.numel(), self.backing.device
        bad_f = (self.backing[:self.start] != _pattern(0, self.start, dev)).nonzero()
        bad_b = (self.backing[end:] != _pattern(end, total, dev)).nonzero()
        front = int(bad_f[-1]) - self.start if bad_f.numel() else None  # (the nearest to the interior comes first)
        back = int(bad_b[0]) if bad_b.numel() else None
        return front, back

    def describe(self):
        return dict(shape=self.shape, dtype=self.dtype, bytes=self.nbytes)


class GuardedAlloc(contextlib.AbstractContextManager):
    """Serve every ``torch.empty(size, dtype=..., device=<device>)`` made inside the context from a guarded buffer."""

    def __init__(self, fill=0xFF, device="cuda:0", band=BAND):
        assert band >= BAND and 0 <= fill <= 0xFF
        self.fill, self.device, self.band = int(fill), torch.device(device), int(band)
        self.served = []
        self._real = None

    # -- the interposer
    def _matches(self, device):
        if device is None:
            return False
        d = torch.device(device)
        return d.type == self.device.type and (d.index is None or self.device.index is None or d.index == self.device.index)

    def _empty(self, *args, **kw):
        if not self._matches(kw.get("device")):
            return self._real(*args, **kw)
        extra = set(kw) - {"dtype", "device"}
        if extra:
            raise AssertionError(f"GuardedAlloc: torch.empty with arguments the rig does not model: {sorted(extra)}")
        return self.allocate(_size_of(args), kw.get("dtype") or torch.get_default_dtype())

    def allocate(self, shape, dtype):
        numel = 1
        for s in shape:
            numel *= s
        nbytes = numel * torch.empty((), dtype=dtype).element_size()
        backing = self._real(self.band + ALIGN + nbytes + self.band, dtype=torch.uint8, device=self.device)
        start = self.band + (-(backing.data_ptr() + self.band)) % ALIGN
        backing[:start] = _pattern(0, start, self.device)
        backing[start + nbytes:] = _pattern(start + nbytes, backing.numel(), self.device)
        backing[start:start + nbytes] = self.fill
        interior = backing[start:start + nbytes].view(dtype).view(shape)
        assert interior.data_ptr() % ALIGN == 0 and interior.is_contiguous()
        assert start >= self.band and backing.numel() - (start + nbytes) >= self.band
        self.served.append(Allocation(shape, dtype, nbytes, backing, start, interior))
        return interior

    def __enter__(self):
        assert self._real is None
        self._real = torch.empty
        torch.empty = self._empty
        return self

    def __exit__(self, *exc):
        torch.empty = self._real
        return False

    # -- the report (call after the device has been synchronised)
    def _sync(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    @property
    def allocations(self):
        return [a.describe() for a in self.served]

    @property
    def interiors(self):
        return [a.interior for a in self.served]

    def report(self):
        self._sync()
        out = []
        for i, a in enumerate(self.served):
            front, back = a.bands()
            out.append(dict(a.describe(), index=i, front=front, back=back))
        return out

    def band_violations(self):
        return [f"allocation {r['index']} {r['shape']} {r['dtype']} ({r['bytes']} bytes): {side} band modified, first at "
                f"offset {r[side]} (bytes {'from the interior start' if side == 'front' else 'behind the interior end'})"
                for r in self.report() for side in ("front", "back") if r[side] is not None]

    def find(self, t):
        """the allocation a (returned) tensor is, or None"""
        for a in self.served:
            if a.nbytes and t.data_ptr() == a.interior.data_ptr() and t.numel() * t.element_size() == a.nbytes:
                return a
        return None


def as_bytes(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(as_bytes(a), as_bytes(b)))


def _flat(result):
    if result is None:
        return []
    if torch.is_tensor(result):
        return [result]
    return [t for t in result if t is not None]


def contract_violations(call, n_alloc, device="cuda:0", finite=True, names=None):
    """Run ``call`` plain and under both pre-fills; -> (violations, rigs, results).  ``call`` returns a tensor or a tuple of
    tensors (None entries are skipped); ``n_alloc``: the allocations the launcher makes per call."""
    device = torch.device(device)
    sync = (lambda: torch.cuda.synchronize(device)) if device.type == "cuda" else (lambda: None)
    plain = _flat(call())
    sync()
    names = names or [f"result {i}" for i in range(len(plain))]
    bad, rigs, results = [], [], [plain]
    for fill in FILLS:
        with GuardedAlloc(fill, device) as rig:
            res = _flat(call())
        sync()
        rigs.append(rig)
        results.append(res)
        tag = f"pre-fill 0x{fill:02X}"
        bad += [f"{tag}: {v}" for v in rig.band_violations()]
        if len(rig.served) != n_alloc:
            bad.append(f"{tag}: the rig served {len(rig.served)} allocations, the launcher makes {n_alloc}: {rig.allocations}")
        if len(res) != len(plain):
            bad.append(f"{tag}: {len(res)} results, {len(plain)} without the rig")
            continue
        for nm, t, p in zip(names, res, plain):
            if not bits_equal(t, p):
                ne = (as_bytes(t) != as_bytes(p)).nonzero() if t.shape == p.shape and t.dtype == p.dtype else None
                where = f", first differing byte {int(ne[0])} of {ne.numel()}" if ne is not None and ne.numel() else ""
                bad.append(f"{tag}: {nm} {tuple(t.shape)} {t.dtype} differs from the run without the rig{where}")
            if finite and t.is_floating_point() and not bool(torch.isfinite(t).all()):
                first = int((~torch.isfinite(t.reshape(-1))).nonzero()[0])
                bad.append(f"{tag}: {nm} {tuple(t.shape)} {t.dtype} is not finite, first at element {first}")
    # a byte of a returned tensor that holds 0xFF after the 0xFF run AND 0x5A after the 0x5A run was never written
    if len(results[1]) == len(results[2]):
        for nm, a, b in zip(names, results[1], results[2]):
            if a.shape == b.shape and a.dtype == b.dtype and rigs[0].find(a) is not None and rigs[1].find(b) is not None:
                kept = ((as_bytes(a) == FILLS[0]) & (as_bytes(b) == FILLS[1])).nonzero()
                if kept.numel():
                    bad.append(f"{nm} {tuple(a.shape)} {a.dtype}: {kept.numel()} bytes still hold the pre-fill, first at byte "
                               f"{int(kept[0])} (element {int(kept[0]) // a.element_size()})")
    if finite:
        for nm, p in zip(names, plain):
            if p.is_floating_point() and not bool(torch.isfinite(p).all()):
                bad.append(f"without the rig: {nm} is not finite")
    return bad, rigs, results
