"""CPU-only tests of the both-strand call (genie_find_smems_both): the exported symbols, the workspace size, the C ABI's
argument checks (they come before the device check, so a host-only handle reaches them) and packing.reverse_complement."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def pkg():
    import genie_smem_amd as g
    g._native.build()
    return g


def test_both_symbols_exported(pkg):
    lib = pkg._native.lib()
    for name in ("genie_find_smems_both", "genie_find_smems_both_workspace_bytes"):
        assert name in pkg._native.SYMBOLS
        getattr(lib, name)
    assert pkg._native.ABI_VERSION == 2 and lib.genie_abi_version() == 2


def test_both_workspace_bytes(pkg):
    lib = pkg._native.lib()
    wb = lib.genie_find_smems_both_workspace_bytes
    assert wb(-1, 150) == -1                                   # GENIE_E_INVALID
    assert wb(10, -1) == -1
    assert wb(10, pkg._native.MAX_READ_LEN + 1) == -6          # GENIE_E_TOO_LONG
    for n in (0, 1, 7, 1000, 123457):
        for L in (0, 1, 100, 150, 255, 256, 1000, 8192):
            assert wb(n, L) >= lib.genie_find_smems_workspace_bytes(2 * n, L), (n, L)
    assert 0 < wb(0, 150) < wb(1000, 150) < wb(2000, 150)
    assert wb(1000, 150) < wb(1000, 255) < wb(1000, 1000) < wb(1000, 8192)


def test_both_argument_checks(pkg):
    lib = pkg._native.lib()
    ix = pkg.GenieIndex.build(np.asarray([0, 1, 2, 3] * 64, np.uint8), 4)        # host arrays only, no device image
    p = C.c_void_p(1 << 20)                                                       # never dereferenced: checks fail first
    ws = lib.genie_find_smems_both_workspace_bytes(10, 150)
    f = lib.genie_find_smems_both

    def call(h=ix._h, mode=1, reads=p, lens=None, n=10, stride=150, fixed=150, offsets=p, rows=p, cap=100, status=None,
             wsp=p, wsb=ws):
        return f(h, mode, reads, lens, n, stride, fixed, 1, offsets, rows, cap, status, wsp, wsb, None)

    assert call(h=None) == -1                          # GENIE_E_INVALID
    assert call(n=-1) == -1
    assert call(offsets=None) == -1
    assert call(reads=None) == -1
    assert call(rows=None) == -1
    assert call(wsp=None) == -1
    assert call(cap=-1) == -1
    assert call(stride=-1) == -1
    assert call(fixed=-1) == -1
    assert call(mode=3) == -1
    assert call(mode=-1) == -1
    assert call(stride=149) == -1                      # stride < fixed_len
    assert call(rows=C.c_void_p((1 << 20) + 4)) == -1  # rows not 16-byte aligned
    assert call(fixed=8193, stride=8193) == -6         # GENIE_E_TOO_LONG
    assert call(wsb=ws - 1) == -10                     # GENIE_E_CAPACITY: too small
    assert call(wsb=lib.genie_find_smems_workspace_bytes(20, 150) - 1) == -10
    assert call(wsp=C.c_void_p((1 << 20) + 16)) == -10  # misaligned
    assert call(n=11) == -10                           # the workspace is for 10 reads
    # every argument good: the device check answers (GENIE_E_NO_DEVICE), on any machine
    assert call() == -4
    assert call(n=0, reads=None, rows=None, wsp=None, wsb=0) == -4


def test_reverse_complement(pkg):
    rc = pkg.packing.reverse_complement
    rng = np.random.default_rng(5)
    a = rng.integers(0, 4, size=(50, 37), dtype=np.uint8)
    r = rc(a)
    assert r.dtype == np.uint8 and r.shape == a.shape
    assert (r == 3 - a[:, ::-1]).all()
    assert (rc(r) == a).all()
    # with lengths: the first lens[i] codes reversed and complemented, the rest left alone
    lens = rng.integers(0, 38, size=50).astype(np.int32)
    lens[:3] = (0, 1, 37)
    b = a.copy()
    b[:, -1] = 200                                     # a bad code: stays bad (c ^ 3 > 3)
    r = rc(b, lens)
    for i in range(50):
        L = int(lens[i])
        assert r[i, :L].tolist() == (b[i, :L][::-1] ^ 3).tolist(), i
        assert r[i, L:].tolist() == b[i, L:].tolist(), i
    assert (rc(r, lens) == b).all()
    assert (r[2, 0] == (200 ^ 3)) and r[2, 0] > 3
    # one read
    assert rc(np.asarray([0, 0, 1, 2], np.uint8)).tolist() == [1, 2, 3, 3]
    assert rc(np.asarray([0, 0, 1, 2], np.uint8), 3).tolist() == [2, 3, 3, 2]
    with pytest.raises(ValueError):
        rc(a, np.full(50, 38, np.int32))
    with pytest.raises(ValueError):
        rc(a, np.full(49, 3, np.int32))
