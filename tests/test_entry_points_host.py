"""CPU-only tests of the return codes of the device-first SMEM entry points (genie_find_smems, genie_find_smems_csr,
genie_find_smems_packed / packed6): they check the handle's device before their arguments, so on a host-only handle every
call with a handle answers GENIE_E_NO_DEVICE, whatever its arguments.  The argument-first entry points (both, split, long)
are pinned by their own host tests."""
import ctypes as C

import numpy as np
import pytest

INVALID, NO_DEVICE = -1, -4


@pytest.fixture(scope="module")
def env():
    import genie_smem_amd as g
    g._native.build()
    ix = g.GenieIndex.build(np.asarray([0, 1, 2, 3] * 64, np.uint8), 4)        # host arrays only, no device image
    return g._native.lib(), ix


P = C.c_void_p(1 << 20)                                                          # never dereferenced: checks fail first


def test_find_smems_codes(env):
    lib, ix = env
    ws = lib.genie_find_smems_workspace_bytes(10, 150)

    def call(h=ix._h, mode=1, reads=P, lens=None, n=10, stride=150, fixed=150, counts=P, slots=P, cap=8, status=None,
             wsp=P, wsb=ws):
        return lib.genie_find_smems(h, mode, reads, lens, n, stride, fixed, 1, counts, slots, cap, status, wsp, wsb, None)

    assert call(h=None) == INVALID
    assert call(h=None, n=-1) == INVALID
    assert call() == NO_DEVICE
    # bad arguments: the device check still answers first
    assert call(n=-1) == NO_DEVICE
    assert call(cap=0) == NO_DEVICE
    assert call(slots=None) == NO_DEVICE
    assert call(mode=3) == NO_DEVICE
    assert call(fixed=8193, stride=8193) == NO_DEVICE
    assert call(slots=C.c_void_p((1 << 20) + 4)) == NO_DEVICE
    assert call(n=0, reads=None, counts=None, slots=None, wsp=None, wsb=0) == NO_DEVICE


def test_find_smems_csr_codes(env):
    lib, ix = env
    ws = lib.genie_find_smems_workspace_bytes(10, 150)

    def call(h=ix._h, mode=1, reads=P, lens=None, n=10, stride=150, fixed=150, offsets=P, rows=P, cap=100, status=None,
             wsp=P, wsb=ws):
        return lib.genie_find_smems_csr(h, mode, reads, lens, n, stride, fixed, 1, offsets, rows, cap, status, wsp, wsb, None)

    assert call(h=None) == INVALID
    assert call(h=None, offsets=None) == INVALID
    assert call() == NO_DEVICE
    assert call(n=-1) == NO_DEVICE
    assert call(offsets=None) == NO_DEVICE
    assert call(rows=None) == NO_DEVICE
    assert call(cap=-1) == NO_DEVICE
    assert call(mode=-1) == NO_DEVICE
    assert call(stride=149) == NO_DEVICE
    assert call(fixed=8193, stride=8193) == NO_DEVICE
    assert call(rows=C.c_void_p((1 << 20) + 4)) == NO_DEVICE
    assert call(wsb=0) == NO_DEVICE
    assert call(n=0, reads=None, rows=None, wsp=None, wsb=0) == NO_DEVICE


@pytest.mark.parametrize("name", ["genie_find_smems_packed", "genie_find_smems_packed6"])
def test_find_smems_packed_codes(env, name):
    lib, ix = env
    f = getattr(lib, name)
    ws = lib.genie_find_smems_workspace_bytes(10, 150)

    def call(h=ix._h, mode=1, reads=P, lens=None, n=10, stride=40, fixed=150, counts=P, status=P, rows=P, cap=100, totals=P,
             esc=P, cap_esc=16, wsp=P, wsb=ws):
        return f(h, mode, reads, lens, n, stride, fixed, 1, counts, status, rows, cap, totals, esc, cap_esc, wsp, wsb, None)

    assert call(h=None) == INVALID
    assert call(h=None, totals=None) == INVALID
    assert call() == NO_DEVICE
    assert call(n=-1) == NO_DEVICE
    assert call(totals=None) == NO_DEVICE
    assert call(esc=None) == NO_DEVICE
    assert call(cap_esc=-1) == NO_DEVICE
    assert call(mode=3) == NO_DEVICE
    assert call(fixed=256) == NO_DEVICE
    assert call(stride=38) == NO_DEVICE
    assert call(rows=C.c_void_p((1 << 20) + 1)) == NO_DEVICE
    assert call(n=0, reads=None, counts=None, status=None, rows=None, wsp=None, wsb=0) == NO_DEVICE
