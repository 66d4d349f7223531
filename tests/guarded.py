"""Guarded buffers for the memory-contract tests (tests/test_memory_contract_*.py, tests/test_streams_gpu.py).

An Arena is one large uint8 allocation on any torch device, filled with a poison byte.  Buffers are cut from it with
exactly the bytes asked for -- no rounding, no minimum -- and a guard band of at least GUARD bytes of poison before and
after each.  A kernel that writes one byte outside a buffer hits a guard; a kernel that reads outside one, or that reads a
scratch or output buffer before writing it, sees a different value under each poison, so its result changes from run to
run.  The conditions of the tests are stated here and nowhere else:

  GUARD    4096 bytes on each side of every buffer;
  POISONS  0x00, 0xFF and 0x5A, in that order (zeros first: the mildest; then all ones: -1 in every integer type and the
           "empty" value several workspace pieces are cleared to; then a pattern that is neither).

Every comparison the tests make on these buffers is exact.

Alignment: alloc(..., align=A, misalign=M) puts the buffer at an address that is M modulo 2 A; the default M = A gives
the weakest address that still is A-aligned (a multiple of A and of nothing larger), and align = 1 an odd address.  The
tests give every pointer of the C ABI the weakest alignment include/genie_smem.h allows: 256 but not 512 for workspaces
and scratch, 16 but not 32 for int32 rows, 2 but not 4 for 6-byte rows, the element size of a typed array (int32: 4 but not
8; int64 and double: 8 but not 16), and an odd address for uint8 inputs with no stated alignment.
"""
import hashlib

import numpy as np
import torch

GUARD = 4096
POISONS = (0x00, 0xFF, 0x5A)


class Arena:
    def __init__(self, device, poison, capacity=32 << 20):
        self.device = torch.device(device)
        self.poison = int(poison)
        assert 0 <= self.poison <= 255
        self.mem = torch.full((int(capacity),), self.poison, dtype=torch.uint8, device=self.device)
        self.base = self.mem.data_ptr()
        self.at = 0                  # everything below is handed out or guard
        self.bufs = []               # (name, front-guard start, buffer start, buffer end, back-guard end)
        self.frozen = []             # (name, tensor, digest)

    # ------------------------------------------------------------------ buffers
    def alloc(self, name, nbytes, align=1, misalign=None):
        """A uint8 view of exactly `nbytes` bytes (0 allowed) whose address is `misalign` modulo 2 * align
        (default: align), with at least GUARD bytes of poison on each side."""
        nbytes, align = int(nbytes), int(align)
        misalign = align if misalign is None else int(misalign)
        assert nbytes >= 0 and align >= 1 and 0 <= misalign < 2 * align and misalign % align == 0
        start = self.at + GUARD
        start += (misalign - (self.base + start)) % (2 * align)
        end = start + nbytes
        if end + GUARD > self.mem.numel():
            raise MemoryError(f"arena of {self.mem.numel()} bytes is full at buffer '{name}' ({nbytes} bytes)")
        self.bufs.append((name, self.at, start, end, end + GUARD))
        self.at = end + GUARD
        return self.mem[start:end]

    def addr(self, name):
        """The address of the newest buffer called `name` (an empty tensor has no data pointer of its own)."""
        for bname, _, start, _, _ in reversed(self.bufs):
            if bname == name:
                return self.base + start
        raise KeyError(name)

    def put(self, name, array, align=1, misalign=None):
        """A buffer holding the bytes of the numpy `array`."""
        raw = np.ascontiguousarray(array).reshape(-1).view(np.uint8)
        t = self.alloc(name, raw.size, align, misalign)
        if raw.size:
            t.copy_(torch.from_numpy(raw.copy()))
        return t

    def check(self):
        """Every guard byte still holds the poison."""
        for name, g0, start, end, g1 in self.bufs:
            for what, a, b in (("front", g0, start), ("back", end, g1)):
                changed = torch.nonzero(self.mem[a:b] != self.poison)
                if changed.numel():
                    # the nearest changed byte: the last one of a front guard, the first one of a back guard
                    at = int(changed[-1 if what == "front" else 0].item())
                    where = f"{b - a - at} bytes before its start" if what == "front" else f"{at} bytes past its end"
                    raise AssertionError(f"{what} guard of buffer '{name}' ({end - start} bytes) was written: offset {at} "
                                         f"of the guard, {where}, value {int(self.mem[a + at].item()):#04x}, "
                                         f"poison {self.poison:#04x}")

    def holds_poison(self, t):
        """True when every byte of the uint8 view `t` still holds the poison."""
        return bool((t == self.poison).all().item())

    # ------------------------------------------------------------------ read-only tensors
    @staticmethod
    def _digest(t):
        raw = t.detach().contiguous().cpu().reshape(-1).view(torch.uint8).numpy()
        return hashlib.sha256(raw.tobytes()).hexdigest()

    def freeze(self, t, name=None):
        """Remember the contents of the read-only tensor `t` (of this arena or not)."""
        self.frozen.append((name or f"input {len(self.frozen)}", t, self._digest(t)))
        return t

    def check_frozen(self):
        for name, t, digest in self.frozen:
            if self._digest(t) != digest:
                raise AssertionError(f"read-only tensor '{name}' ({t.numel() * t.element_size()} bytes) was changed")


def as_numpy(t, dtype, shape=None):
    """The bytes of the uint8 view `t` as a numpy array of `dtype` (a host copy)."""
    a = t.detach().cpu().numpy().copy().view(dtype)
    return a if shape is None else a.reshape(shape)
