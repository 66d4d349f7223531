"""CPU-only tests of genie_match_stats (matching statistics of every read position): the symbols, the workspace function,
the C ABI's argument checks (before the device check, so a host-only handle reaches them), and the Python restatement of the
specification (tests/match_stats_util.py) against the SMEM brute force of tests/smem_util.py: the rows that the traversal
derives from the restated lengths, with the restated intervals, are smems(ref, read, 1)."""
import ctypes as C
import os

import numpy as np
import pytest

import lookup_util as U
import match_stats_util as MS
import smem_util as SM

BOTH, SPLIT = MS.BOTH, MS.SPLIT
FLAGS = (0, BOTH, SPLIT, BOTH | SPLIT)
INVALID, NO_DEVICE, CAPACITY = -1, -4, -10


@pytest.fixture(scope="module")
def pkg():
    import genie_smem_amd as g
    g._native.build()
    return g


def test_match_stats_symbols_exported(pkg):
    lib = pkg._native.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "genie_smem.h")).read()
    for name, nargs, res in (("genie_match_stats", 13, C.c_int), ("genie_match_stats_workspace_bytes", 4, C.c_int64)):
        assert name in pkg._native.SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is res and len(fn.argtypes) == nargs
        assert name + "(" in header
    assert lib.genie_abi_version() == 2                            # an addition: the version stays


def test_match_stats_workspace_bytes(pkg):
    lib = pkg._native.lib()
    ws, ex = lib.genie_match_stats_workspace_bytes, lib.genie_find_smems_long_ex_workspace_bytes
    for fl in FLAGS:
        assert ws(-1, 100, 10, fl) == INVALID
        assert ws(1, -1, 10, fl) == INVALID
        assert ws(1, 100, -1, fl) == INVALID
        assert ws(1, 100, 2**31, fl) == INVALID
    for fl in (4, 8, -1, 1 << 30, BOTH | 4):
        assert ws(1, 100, 10, fl) == INVALID
    ns = [0, 1, 2, 3, 1000, 10**6]
    ts = [0, 1, 31, 32, 33, 255, 256, 10**4, 10**6, 10**8]
    for fl in FLAGS:
        grid = [[ws(n, t, 2**31 - 1, fl) for t in ts] for n in ns]
        for i, n in enumerate(ns):
            for j, t in enumerate(ts):
                assert grid[i][j] > 0 and grid[i][j] % 256 == 0
                assert grid[i][j] <= ex(n, t, 2**31 - 1, fl), (fl, n, t)
                assert grid[i][j] == ws(n, t, 0, fl)               # max_len is a bound for the check, not a size
                if i:
                    assert grid[i][j] >= grid[i - 1][j], (fl, i, j)
                if j:
                    assert grid[i][j] >= grid[i][j - 1], (fl, i, j)
    # two of the five stages: the packed stream and fwd[], 4.25 bytes per position
    assert ws(10, 10**8, 10**8, 0) < 4.3 * 10**8
    assert ws(10, 10**8, 10**8, BOTH) < 2 * 4.3 * 10**8


def test_match_stats_argument_checks_before_device(pkg):
    lib = pkg._native.lib()
    ref = np.random.default_rng(1).integers(0, 4, 2000).astype(np.uint8)
    h = C.c_void_p(0)
    assert lib.genie_index_create(ref.ctypes.data_as(C.POINTER(C.c_uint8)), ref.size, 8, 0, C.byref(h)) == 0
    try:
        buf = np.zeros(1 << 16, np.uint8)
        al = (buf.ctypes.data + 255) & ~255
        p = C.c_void_p(al)
        for fl in FLAGS:
            bytes_ok = lib.genie_match_stats_workspace_bytes(2, 100, 100, fl)
            assert 0 < bytes_ok <= (1 << 16) - 256

            def call(ix=h, flags=fl, bases=p, offs=p, n=2, total=100, max_len=100, ms=p, lohi=p, st=p, wsp=p, wsb=bytes_ok):
                return lib.genie_match_stats(ix, flags, bases, offs, n, total, max_len, ms, lohi, st, wsp, wsb, None)

            assert call(ix=None) == INVALID
            assert call(n=-1) == INVALID
            assert call(total=-1) == INVALID
            assert call(max_len=-1) == INVALID
            assert call(max_len=2**31) == INVALID
            assert call(wsb=-1) == INVALID
            assert call(offs=None) == INVALID
            assert call(bases=None) == INVALID
            assert call(ms=None) == INVALID
            assert call(flags=fl | 4) == INVALID                    # an unknown flag bit
            assert call(flags=fl | (1 << 20)) == INVALID
            assert call(flags=-1) == INVALID
            assert call(ms=C.c_void_p(al + 2)) == INVALID           # d_ms 4-byte aligned
            assert call(lohi=C.c_void_p(al + 4)) == INVALID         # d_lohi 8-byte aligned
            assert call(lohi=C.c_void_p(al + 1)) == INVALID
            assert call(wsp=None) == CAPACITY
            assert call(wsp=C.c_void_p(al + 16)) == CAPACITY        # workspace 256-byte aligned
            assert call(wsb=bytes_ok - 1) == CAPACITY
            assert call(wsb=0) == CAPACITY
            assert call(ms=None, wsp=None) == INVALID               # a bad argument is reported before a capacity
            assert call() == NO_DEVICE                              # every argument was fine
            assert call(lohi=None) == NO_DEVICE and call(st=None) == NO_DEVICE and call(lohi=None, st=None) == NO_DEVICE
            assert call(ms=C.c_void_p(al + 4), lohi=C.c_void_p(al + 8)) == NO_DEVICE
            assert call(n=0, offs=None, wsp=None, wsb=0, total=0, bases=None, ms=None, lohi=None, st=None) == NO_DEVICE
            assert call(n=0, offs=None, wsp=None, wsb=0) == NO_DEVICE                # bases that belong to no read
    finally:
        lib.genie_index_destroy(h)


def test_python_layer_refuses_a_host_only_handle(pkg):
    ref = np.random.default_rng(2).integers(0, 4, 3000).astype(np.uint8)
    ix = pkg.GenieIndex.build(ref, 8)                               # host-only: no device was touched
    assert callable(ix.match_stats) and callable(pkg.SMEM.match_stats) and callable(pkg.SMEM.match_stats_text)
    with pytest.raises(Exception):
        ix.match_stats(np.zeros(10, np.uint8), np.asarray([0, 10], np.int64))


# ------------------------------------------------------------------ the restatement against the SMEM brute force
@pytest.mark.parametrize("name", ["rand5", "rand37", "tail_AAAAAAAA", "tail_C", "tandem3", "tandem7", "noT", "rand4096"])
def test_restated_lengths_and_intervals_give_the_smems(name):
    ref = U.family()[name]
    b = SM.batches(name)
    reads = [r for L in (1, 2, 7, 16, 33, 64, 150) for r in b["short"][L]] + b["mid"][705][:4] + MS.window_reads(ref)[1:3]
    checked = 0
    for read in reads:
        ms, lohi, st = MS.expected_one(ref, read, False)
        want, flagged = SM.smems(ref, read, 1)
        if (read > 3).any():
            assert st == MS.READ_BAD_BASE and (ms == -1).all() and (lohi == -1).all()
            continue
        assert (st == MS.READ_ABSENT_BASE) == flagged == bool((ms == 0).any())
        assert (ms[1:] >= ms[:-1] - 1).all() and (ms <= len(read) - np.arange(len(read))).all()
        assert ((lohi[:, 0] < 0) == (ms == 0)).all()
        if flagged:
            # the split form cuts at the absent bases and agrees everywhere else
            ms2, lohi2, st2 = MS.expected_one(ref, read, True)
            assert st2 == MS.READ_OK and np.array_equal(ms2, ms) and np.array_equal(lohi2, lohi)
            continue
        rows = np.asarray([(s, e) + tuple(lohi[s]) for s, e in MS.rows_from_lengths(ms)], np.int32).reshape(-1, 4)
        assert np.array_equal(rows, want)
        checked += 1
    assert checked >= 20


def test_restated_layout_breaks_and_strands():
    ref = U.family()["noT"]
    reads = MS.break_reads(ref)
    for fl in FLAGS:
        strands = 2 if fl & BOTH else 1
        ms, lohi, st = MS.expected(ref, reads, fl, lead=5, tail=3)
        total = sum(len(r) for r in reads) + 8
        assert ms.shape == (strands * total,) and lohi.shape == (strands * total, 2) and st.shape == (strands * len(reads),)
        assert (ms[:strands * 5] == 0).all() and (ms[-strands * 3:] == 0).all() and (lohi[:strands * 5] == -1).all()
        # both strands = the explicit interleaved batch
        if fl & BOTH:
            one = MS.expected(ref, MS.strand_reads(reads, 2), fl & SPLIT, lead=10, tail=6)
            assert all(np.array_equal(x, y) for x, y in zip((ms, lohi, st), one))
        if fl & SPLIT:
            assert not st.any() and (ms >= 0).all()
        else:
            assert set(st.tolist()) == {0, 1, 3}
            for q, r in enumerate(MS.strand_reads(reads, strands)):
                assert (st[q] == 1) == bool((r > 3).any())
    # strand 1 of a read without A or T on the reference without T: C <-> G, nothing is lost
    r = np.asarray([1, 2, 2, 1, 1, 2], np.uint8)
    ms, lohi, st = MS.expected(ref, [r], BOTH)
    assert st.tolist() == [0, 0] and (ms > 0).all()
    # ... and a read with A has T on strand 1: flagged there, its other positions still correct
    r = np.asarray([1, 0, 2], np.uint8)
    ms, lohi, st = MS.expected(ref, [r], BOTH)
    assert st.tolist() == [0, 3] and ms[3 + 1] == 0 and ms[3] > 0 and ms[5] > 0
