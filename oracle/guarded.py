"""Guard-banded, poisoned buffers for kernel tests.

Production packs saved activations, statistics partials, coefficient tables and weight-gradient partials back to back at 256-byte
granularity (nets.Arena.alloc) and keeps every parameter gradient in one flat buffer at 64-float alignment.  A test that hands a kernel
a tensor of its own from the caching allocator sees neither a write that lands beside the tensor nor an element the kernel never wrote.

    Guarded(numel, dtype, device)   one byte buffer  [front guard | payload | back guard]
        payload   starts on a 256-byte boundary, exactly numel * itemsize bytes, pre-filled with a recognisable bit pattern
                  (a quiet NaN with a fixed payload for the float types, 0x5A bytes for the integer types; poison=False: zeros,
                  for a buffer whose documented contract is "zeroed by the caller")
        guards    256 KiB each, filled with the byte 0x5A
    flat_with_gaps(sizes)           several payload ranges at 64-float alignment inside one Guarded: the flat gradient buffer;
                                    the alignment gaps are poisoned and checked like guards

Nothing here is GPU-specific: the same object works on CPU tensors (tests/test_guarded_cpu.py).
"""
from __future__ import annotations

import torch

GUARD_BYTES = 256 * 1024
GUARD_BYTE = 0x5A
ALIGN_BYTES = 256
MAX_LISTED = 8

# dtype -> (integer view type, poison value as that signed integer)
_F32_POISON = 0x7FC5A5A5
_BF16_POISON = 0x7FC5
_F64_POISON = 0x7FF85A5A5A5A5A5A
_INT_VIEW = {
    torch.float32: (torch.int32, _F32_POISON),
    torch.bfloat16: (torch.int16, _BF16_POISON),
    torch.float64: (torch.int64, _F64_POISON),
    torch.uint8: (torch.uint8, 0x5A),
    torch.int8: (torch.int8, 0x5A),
    torch.int16: (torch.int16, 0x5A5A),
    torch.int32: (torch.int32, 0x5A5A5A5A),
    torch.int64: (torch.int64, 0x5A5A5A5A5A5A5A5A),
}


class GuardError(AssertionError):
    """A check of a guarded buffer failed.  `violations`: one dict per finding (see Guarded.guard_violations / unwritten)."""

    def __init__(self, message, violations):
        super().__init__(message)
        self.violations = violations


class Guarded:
    def __init__(self, numel, dtype=torch.float32, device="cpu", poison=True, name="buffer"):
        if dtype not in _INT_VIEW:
            raise TypeError(f"Guarded: unsupported dtype {dtype}")
        self.numel, self.dtype, self.device, self.poison, self.name = int(numel), dtype, torch.device(device), bool(poison), name
        self.itemsize = torch.empty((), dtype=dtype).element_size()
        self.nbytes = self.numel * self.itemsize
        self._buf = torch.empty(2 * GUARD_BYTES + self.nbytes + ALIGN_BYTES, dtype=torch.uint8, device=self.device)
        base = self._buf.data_ptr()
        self._start = GUARD_BYTES + (-(base + GUARD_BYTES)) % ALIGN_BYTES          # byte offset of the payload inside the buffer
        assert (base + self._start) % ALIGN_BYTES == 0 and self._start % self.itemsize == 0
        self.repoison()

    # ------------------------------------------------------------------------------------------------ views
    def _front(self):
        return self._buf[self._start - GUARD_BYTES:self._start]

    def _back(self):
        return self._buf[self._start + self.nbytes:self._start + self.nbytes + GUARD_BYTES]

    def _payload_bytes(self):
        return self._buf[self._start:self._start + self.nbytes]

    def bits(self):
        """the payload as a flat tensor of the integer type of the same width (a view)"""
        return self._payload_bytes().view(_INT_VIEW[self.dtype][0])

    def flat(self):
        """the payload as a flat tensor of its dtype (a view)"""
        return self._payload_bytes().view(self.dtype)

    def view(self, shape, channels_last=False):
        """The tensor the kernel sees.  channels_last: `shape` is the logical (n, c, h, w) of a tensor whose memory is NHWC."""
        shape = tuple(int(s) for s in shape)
        if channels_last:
            n, c, h, w = shape
            return self.flat().view(n, h, w, c).permute(0, 3, 1, 2)
        return self.flat().view(shape)

    @property
    def ptr(self):
        return self._buf.data_ptr() + self._start

    # ------------------------------------------------------------------------------------------------ fill
    def repoison(self):
        """restore both guards and the payload (poison bits, or zeros with poison=False)"""
        self._front().fill_(GUARD_BYTE)
        self._back().fill_(GUARD_BYTE)
        self.poison_range(0, self.numel)
        return self

    def poison_range(self, lo, hi):
        b = self.bits()[lo:hi]
        if not self.poison:
            b.zero_()
        else:
            b.fill_(_INT_VIEW[self.dtype][1])

    # ------------------------------------------------------------------------------------------------ checks
    def guard_violations(self):
        """[{side, first, last, count}] for every guard that no longer holds its pattern; `first` / `last` are byte offsets relative to the
        start of the payload (negative in the front guard, >= nbytes in the back guard), `count` the number of bytes that differ."""
        out = []
        for side, g, origin in (("front", self._front(), -GUARD_BYTES), ("back", self._back(), self.nbytes)):
            bad = torch.nonzero(g != GUARD_BYTE).flatten()
            if bad.numel():
                out.append(dict(side=side, first=origin + int(bad[0]), last=origin + int(bad[-1]), count=int(bad.numel())))
        return out

    def check_guards(self):
        v = self.guard_violations()
        if v:
            msg = "; ".join(f"{x['side']} guard: {x['count']} byte(s) touched, payload-relative offsets {x['first']} .. {x['last']}" for x in v)
            raise GuardError(f"{self.name} ({self.numel} x {self.dtype}, {self.nbytes} bytes): {msg}", v)

    def unwritten(self):
        """flat indices of the payload elements that still carry the poison bits"""
        if not self.poison:
            raise RuntimeError("check_written needs a poisoned payload (poison=True)")
        return torch.nonzero(self.bits() == _INT_VIEW[self.dtype][1]).flatten()

    def check_written(self):
        idx = self.unwritten()
        if idx.numel():
            first = [int(i) for i in idx[:MAX_LISTED]]
            raise GuardError(f"{self.name} ({self.numel} x {self.dtype}): {int(idx.numel())} element(s) never written, first indices {first}",
                             [dict(side="payload", count=int(idx.numel()), indices=first)])

    def snapshot(self):
        """a copy of the payload bits, for the run-to-run comparison"""
        return self.bits().clone()


class FlatWithGaps:
    """`sizes[i]` floats at offset `offsets[i]` (a multiple of align_f) of one guarded buffer; everything between the ranges is a gap."""

    def __init__(self, sizes, align_f=64, dtype=torch.float32, device="cpu", name="flat"):
        self.sizes = [int(s) for s in sizes]
        self.offsets, off = [], 0
        for s in self.sizes:
            self.offsets.append(off)
            off += -(-s // align_f) * align_f
        self.total = off
        self.buf = Guarded(self.total, dtype, device, poison=True, name=name)
        self.name = name

    @property
    def ptr(self):
        return self.buf.ptr

    def flat(self):
        return self.buf.flat()

    def range(self, i, shape=None):
        t = self.buf.flat()[self.offsets[i]:self.offsets[i] + self.sizes[i]]
        return t if shape is None else t.view(shape)

    def range_ptr(self, i):
        return self.buf.ptr + self.offsets[i] * self.buf.itemsize

    def gap_mask(self):
        m = torch.ones(self.total, dtype=torch.bool, device=self.buf.device)
        for o, s in zip(self.offsets, self.sizes):
            m[o:o + s] = False
        return m

    def repoison(self):
        self.buf.repoison()
        return self

    def gap_violations(self):
        """[{side: 'gap', after_range, first, last, count}]: float indices (into the flat buffer) of gap elements that lost the poison bits"""
        bad = torch.nonzero(self.gap_mask() & (self.buf.bits() != _INT_VIEW[self.buf.dtype][1])).flatten()
        out = []
        for i, (o, s) in enumerate(zip(self.offsets, self.sizes)):
            end = self.offsets[i + 1] if i + 1 < len(self.offsets) else self.total
            sel = bad[(bad >= o + s) & (bad < end)]
            if sel.numel():
                out.append(dict(side="gap", after_range=i, first=int(sel[0]), last=int(sel[-1]), count=int(sel.numel())))
        return out

    def check_guards(self):
        """both guards of the whole buffer and every alignment gap"""
        self.buf.check_guards()
        v = self.gap_violations()
        if v:
            msg = "; ".join(f"gap after range {x['after_range']}: {x['count']} element(s) written, flat indices {x['first']} .. {x['last']}" for x in v)
            raise GuardError(f"{self.name}: {msg}", v)

    def check_written(self, i):
        t = self.buf.bits()[self.offsets[i]:self.offsets[i] + self.sizes[i]]
        idx = torch.nonzero(t == _INT_VIEW[self.buf.dtype][1]).flatten()
        if idx.numel():
            first = [int(k) for k in idx[:MAX_LISTED]]
            raise GuardError(f"{self.name}: range {i}: {int(idx.numel())} element(s) never written, first indices {first}",
                             [dict(side="payload", range=i, count=int(idx.numel()), indices=first)])


def flat_with_gaps(sizes, align_f=64, dtype=torch.float32, device="cpu", name="flat"):
    return FlatWithGaps(sizes, align_f, dtype, device, name)


class GuardedCall:
    """The steps every guard-band case takes, around one callable that issues the kernel launches:

        gc = GuardedCall(device)
        y = gc.out("y", numel)                      # a poisoned Guarded; written=False: guards only (a buffer with padding nobody reads)
        acc = gc.out("acc", numel, init=fill)       # fill(buffer) runs after every (re)poison: an accumulator's previous contents
        gc.run(launch)                              # launch(); guards of every buffer; check_written of the `written` ones; snapshot
        ... compare the views with the reference ...
        gc.rerun(launch)                            # repoison, launch() again: guards, written, and bit-identical payloads

    A poisoned element that a consumer reads surfaces as a NaN in the comparison with the reference."""

    def __init__(self, device="cpu"):
        self.device = torch.device(device)
        self.bufs, self.written, self.inits, self.first = {}, {}, {}, None

    def out(self, name, numel, dtype=torch.float32, written=True, poison=True, init=None):
        g = Guarded(numel, dtype, self.device, poison=poison, name=name)
        return self._add(name, g, bool(written) and poison, init)

    def flat(self, name, sizes, written=(), align_f=64, init=None):
        """a flat_with_gaps buffer; `written`: the indices of the ranges the call must fill completely"""
        f = FlatWithGaps(sizes, align_f, torch.float32, self.device, name=name)
        return self._add(name, f, list(written), init)

    def _add(self, name, buf, written, init):
        assert name not in self.bufs, name
        self.bufs[name], self.written[name], self.inits[name] = buf, written, init
        if init is not None:
            init(buf)
        return buf

    def _check(self):
        for name, b in self.bufs.items():
            b.check_guards()
            w = self.written[name]
            if isinstance(b, FlatWithGaps):
                for i in w:
                    b.check_written(i)
            elif w:
                b.check_written()

    def _snap(self):
        return {name: (b.buf if isinstance(b, FlatWithGaps) else b).snapshot() for name, b in self.bufs.items()}

    def run(self, launch):
        launch()
        self._check()
        self.first = self._snap()
        return self

    def rerun(self, launch):
        assert self.first is not None, "rerun before run"
        for name, b in self.bufs.items():
            b.repoison()
            if self.inits[name] is not None:
                self.inits[name](b)
        launch()
        self._check()
        for name, s in self._snap().items():
            diff = torch.nonzero(s != self.first[name]).flatten()
            if diff.numel():
                raise GuardError(f"{name}: the second run differs from the first in {int(diff.numel())} element(s), first indices "
                                 f"{[int(i) for i in diff[:MAX_LISTED]]}", [dict(side="rerun", count=int(diff.numel()))])
        return self
