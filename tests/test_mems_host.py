"""CPU-only tests of genie_find_mems (every maximal exact match of a read batch): the symbols, the workspace function, the C
ABI's argument checks (before the device check, so a host-only handle reaches them), and the brute force of
tests/mems_util.py against hand-written cases, against the definition base by base, and against the matching statistics
restated in tests/match_stats_util.py."""
import ctypes as C
import os

import numpy as np
import pytest

import lookup_util as U
import match_stats_util as MS
import mems_util as MM
import smem_util as SM

BOTH, SPLIT = MM.BOTH, MM.SPLIT
FLAGS = (0, BOTH, SPLIT, BOTH | SPLIT)
INVALID, NO_DEVICE, CAPACITY = -1, -4, -10


@pytest.fixture(scope="module")
def pkg():
    import genie_smem_amd as g
    g._native.build()
    return g


def test_find_mems_symbols_exported(pkg):
    lib = pkg._native.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "genie_smem.h")).read()
    for name, nargs, res in (("genie_find_mems", 17, C.c_int), ("genie_find_mems_workspace_bytes", 4, C.c_int64)):
        assert name in pkg._native.SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is res and len(fn.argtypes) == nargs
        assert name + "(" in header
    assert lib.genie_abi_version() == 2 and pkg._native.ABI_VERSION == 2      # an addition: the version stays
    assert "#define GENIE_ABI_VERSION 2" in header


def test_find_mems_workspace_bytes(pkg):
    lib = pkg._native.lib()
    ws, stats = lib.genie_find_mems_workspace_bytes, lib.genie_match_stats_workspace_bytes
    for fl in FLAGS:
        assert ws(-1, 100, 10, fl) == INVALID
        assert ws(1, -1, 10, fl) == INVALID
        assert ws(1, 100, -1, fl) == INVALID
        assert ws(1, 100, 2**31, fl) == INVALID
    for fl in (4, 8, -1, 1 << 30, BOTH | 4):
        assert ws(1, 100, 10, fl) == INVALID
    ns = [0, 1, 2, 3, 1000, 10**6]
    ts = [0, 1, 31, 32, 33, 255, 256, 257, 10**4, 10**6, 10**8]
    for fl in FLAGS:
        grid = [[ws(n, t, 2**31 - 1, fl) for t in ts] for n in ns]
        for i, n in enumerate(ns):
            for j, t in enumerate(ts):
                assert grid[i][j] > 0 and grid[i][j] % 256 == 0
                assert grid[i][j] >= stats(n, t, 2**31 - 1, fl), (fl, n, t)
                assert grid[i][j] == ws(n, t, 0, fl)               # max_len is a bound for the check, not a size
                if i:
                    assert grid[i][j] >= grid[i - 1][j], (fl, i, j)
                if j:
                    assert grid[i][j] >= grid[i][j - 1], (fl, i, j)
    # the header's figures: 33 bytes per virtual position and 8 per 64 of them on top of the matching statistics' workspace
    for fl in FLAGS:
        strands = 2 if fl & BOTH else 1
        extra = ws(10, 10**8, 10**8, fl) - stats(10, 10**8, 10**8, fl)
        assert 33.125 * strands * 10**8 <= extra < 33.2 * strands * 10**8


def test_find_mems_argument_checks_before_device(pkg):
    lib = pkg._native.lib()
    ref = np.random.default_rng(1).integers(0, 4, 2000).astype(np.uint8)
    h = C.c_void_p(0)
    assert lib.genie_index_create(ref.ctypes.data_as(C.POINTER(C.c_uint8)), ref.size, 8, 0, C.byref(h)) == 0
    try:
        buf = np.zeros(1 << 16, np.uint8)
        al = (buf.ctypes.data + 255) & ~255
        p = C.c_void_p(al)
        for fl in FLAGS:
            bytes_ok = lib.genie_find_mems_workspace_bytes(2, 100, 100, fl)
            assert 0 < bytes_ok <= (1 << 16) - 256

            def call(ix=h, flags=fl, bases=p, offs=p, n=2, total=100, max_len=100, m=5, occ=0, out=p, rows=p, cap=10, st=p, tt=p,
                     wsp=p, wsb=bytes_ok):
                return lib.genie_find_mems(ix, flags, bases, offs, n, total, max_len, m, occ, out, rows, cap, st, tt, wsp, wsb, None)

            assert call(ix=None) == INVALID
            assert call(out=None) == INVALID
            assert call(offs=None) == INVALID
            assert call(bases=None) == INVALID
            assert call(n=-1) == INVALID
            assert call(total=-1) == INVALID
            assert call(max_len=-1) == INVALID
            assert call(max_len=2**31) == INVALID
            assert call(cap=-1) == INVALID
            assert call(wsb=-1) == INVALID
            assert call(m=0) == INVALID
            assert call(m=-3) == INVALID
            assert call(occ=-1) == INVALID
            assert call(flags=fl | 4) == INVALID                    # an unknown flag bit
            assert call(flags=fl | (1 << 20)) == INVALID
            assert call(flags=-1) == INVALID
            assert call(rows=C.c_void_p(al + 8)) == INVALID         # d_rows 16-byte aligned
            assert call(out=C.c_void_p(al + 4)) == INVALID          # d_offsets, d_totals 8-byte aligned
            assert call(tt=C.c_void_p(al + 4)) == INVALID
            assert call(st=C.c_void_p(al + 2)) == INVALID           # d_status 4-byte aligned
            assert call(wsp=None) == CAPACITY
            assert call(wsp=C.c_void_p(al + 16)) == CAPACITY        # workspace 256-byte aligned
            assert call(wsb=bytes_ok - 1) == CAPACITY
            assert call(wsb=0) == CAPACITY
            assert call(m=0, wsp=None) == INVALID                   # a bad argument is reported before a capacity
            assert call() == NO_DEVICE                              # every argument was fine
            assert call(rows=None) == NO_DEVICE and call(rows=None, cap=0) == NO_DEVICE      # the sizing call
            assert call(st=None) == NO_DEVICE and call(tt=None) == NO_DEVICE and call(st=None, tt=None, rows=None) == NO_DEVICE
            assert call(m=2**31 - 1, occ=2**31 - 1) == NO_DEVICE
            assert call(out=C.c_void_p(al + 8), tt=C.c_void_p(al + 8), st=C.c_void_p(al + 4), rows=C.c_void_p(al + 16)) == NO_DEVICE
            assert call(n=0, wsp=None, wsb=0, total=0, bases=None) == NO_DEVICE
            assert call(n=0, offs=None, wsp=None, wsb=0) == INVALID      # the offsets hold N + 1 entries: one at least
    finally:
        lib.genie_index_destroy(h)


def test_python_layer_refuses_a_host_only_handle(pkg):
    ref = np.random.default_rng(2).integers(0, 4, 3000).astype(np.uint8)
    ix = pkg.GenieIndex.build(ref, 8)                               # host-only: no device was touched
    assert callable(ix.find_mems) and callable(pkg.SMEM.find_mems)
    with pytest.raises(Exception):
        ix.find_mems(np.zeros(10, np.uint8), np.asarray([0, 10], np.int64), 5)


# ------------------------------------------------------------------ the brute force against hand-written cases
def _codes(s):
    return np.asarray(["ACGTN".index(c) if c != "N" else 7 for c in s], np.uint8)


def _rows(ref, read, m, split=False, max_occ=0):
    rows, status, skipped = MM.expected_one(_codes(ref), _codes(read), m, split, max_occ)
    return rows.tolist(), status, skipped


def test_brute_force_on_hand_written_cases():
    # suffix rows of ACGTAC: '' AC ACGTAC C CGTAC GTAC TAC
    assert U.suffix_rows(_codes("ACGTAC")).tolist() == [6, 4, 0, 5, 1, 2, 3]
    # a read equal to the reference: the main diagonal, touching t == 0, p == 0, t + l == n and p + l == L at once
    assert _rows("ACGTAC", "ACGTAC", 3) == ([[0, 6, 1, 2]], 0, 0)
    # ... and with m = 2 the AC that ends the reference (t + l == n, p == 0) and the AC that ends the read (t == 0, p + l == L)
    assert _rows("ACGTAC", "ACGTAC", 2) == ([[0, 2, 5, 1], [0, 6, 1, 2], [4, 6, 1, 2]], 0, 0)
    # a homopolymer: one MEM per diagonal; suffix rows of AAAA: '' A AA AAA AAAA
    assert _rows("AAAA", "AAA", 2) == ([[0, 2, 3, 2], [0, 3, 2, 3], [0, 3, 1, 4], [1, 3, 1, 4]], 0, 0)
    assert _rows("AAAA", "AAA", 3) == ([[0, 3, 2, 3], [0, 3, 1, 4]], 0, 0)
    assert _rows("AAAA", "AAA", 4) == ([], 0, 0)
    # max_occ: AA occurs three times; positions 0 and 1 start with it
    assert _rows("AAAA", "AAA", 2, max_occ=2) == ([], 0, 2)
    assert _rows("AAAA", "AAA", 2, max_occ=3)[2] == 0
    assert _rows("AAAA", "AAA", 3, max_occ=1) == ([], 0, 1)
    # suffix rows of GGACGTCC: '' ACGTCC C CC CGTCC GACGTCC GGACGTCC GTCC TCC
    assert U.suffix_rows(_codes("GGACGTCC")).tolist() == [8, 2, 7, 6, 3, 1, 0, 4, 5]
    # a break on either side of a match: inside the read, neither at t == 0 nor at t + l == n
    assert _rows("GGACGTCC", "NACGTN", 3, split=True) == ([[1, 5, 3, 1]], 0, 0)
    assert _rows("GGACGTCC", "NACGTN", 3, split=False) == ([], MM.READ_BAD_BASE, 0)
    # without the break the match would reach from t = 1; with it the rest is a MEM of its own
    assert _rows("GGACGTCC", "GACGTC", 3) == ([[0, 6, 2, 5]], 0, 0)
    assert _rows("GGACGTCC", "GNCGTC", 3, split=True) == ([[2, 6, 4, 4]], 0, 0)
    assert _rows("GGACGTCC", "GACGNC", 3, split=True) == ([[0, 4, 2, 5]], 0, 0)
    # a base the reference lacks ends a match like a break, flags the read without SPLIT and leaves the rows alone
    assert _rows("GGACGGCC", "ACGTACG", 3) == ([[0, 3, 3, 1], [4, 7, 3, 1]], MM.READ_ABSENT_BASE, 0)
    assert _rows("GGACGGCC", "ACGTACG", 3, split=True) == ([[0, 3, 3, 1], [4, 7, 3, 1]], 0, 0)
    # a read longer than the reference, and the empty read
    assert _rows("ACG", "GGACGCC", 3) == ([[2, 5, 1, 1]], 0, 0)
    assert _rows("ACG", "GGACGCC", 1) == ([[0, 1, 3, 3], [1, 2, 3, 3], [2, 5, 1, 1], [5, 6, 2, 2], [6, 7, 2, 2]], 0, 0)
    assert _rows("ACG", "", 1) == ([], 0, 0)


@pytest.mark.parametrize("name", ["rand5", "rand37", "tail_AAAAAAAA", "tandem3", "noT"])
def test_brute_force_rows_meet_the_definition(name):
    ref = U.family()[name]
    rng = np.random.default_rng(3)
    reads = MS.break_reads(ref)[2:9] + [r for L in (2, 7, 33) for r in SM.batches(name)["short"][L][:2]]
    checked = 0
    for read in reads:
        for split in (False, True):
            for m in (1, 3, 12):
                rows, status, _ = MM.expected_one(ref, read, m, split)
                assert (rows[:, 1] - rows[:, 0] >= m).all()
                key = rows[:, 0].astype(np.int64) * (len(ref) + 1) + rows[:, 3]
                assert (np.diff(key) > 0).all()                      # (start, row) ascending, no row twice
                for row in rows[rng.permutation(len(rows))[:40]]:
                    assert MM.is_mem(ref, read, row, split), (name, m, row)
                    checked += 1
    assert checked > 100


# ------------------------------------------------------------------ consequence 1: the matching statistics
@pytest.mark.parametrize("name", ["rand37", "tail_C", "tandem7", "noT", "rand4096"])
def test_longest_rows_are_the_left_maximal_rows_of_lohi(name):
    ref = U.family()[name]
    sa = U.suffix_rows(ref)
    reads = MS.break_reads(ref)[2:6] + SM.batches(name)["short"][33][:2] + [MS.window_reads(ref)[0]]
    seen = 0
    for read in reads:
        for split in (False, True):
            ms, lohi, st = MS.expected_one(ref, read, split)
            brk = MM.breaks_of(ref, read, split)
            for m in (3, 20):
                rows, status, _ = MM.expected_one(ref, read, m, split)
                assert status == st
                for p in np.flatnonzero(ms >= m).tolist():
                    got = rows[(rows[:, 0] == p) & (rows[:, 1] - rows[:, 0] == ms[p])][:, 3].tolist()
                    want = [r for r in range(lohi[p, 0], lohi[p, 1] + 1)
                            if p == 0 or sa[r] == 0 or brk[p - 1] or read[p - 1] != ref[sa[r] - 1]]
                    assert got == want, (name, split, m, p)
                    seen += len(want)
                # and no row starts where the longest match is shorter than m, or is longer than it
                assert (ms[rows[:, 0]] >= rows[:, 1] - rows[:, 0]).all()
    assert seen > 20
