"""CPU-only tests of genie_exact_match (suffix-array intervals of CSR patterns of any length, on one strand or both): the
symbols, the workspace function, the C ABI's argument checks (before the device check, so a host-only handle reaches them),
and the Python restatement of the specification (tests/exact_match_util.py) against hand-made cases."""
import ctypes as C
import os

import numpy as np
import pytest

import exact_match_util as EM
import lookup_util as U

BOTH, SPLIT = EM.BOTH, EM.SPLIT
INVALID, NO_DEVICE, CAPACITY = -1, -4, -10


@pytest.fixture(scope="module")
def pkg():
    import genie_smem_amd as g
    g._native.build()
    return g


def test_exact_match_symbols_exported(pkg):
    lib = pkg._native.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "genie_smem.h")).read()
    for name, nargs, res in (("genie_exact_match", 13, C.c_int), ("genie_exact_match_workspace_bytes", 4, C.c_int64)):
        assert name in pkg._native.SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is res and len(fn.argtypes) == nargs
        assert name + "(" in header
    assert lib.genie_abi_version() == 2                            # an addition: the version stays


def test_exact_match_workspace_bytes(pkg):
    lib = pkg._native.lib()
    ws, ms = lib.genie_exact_match_workspace_bytes, lib.genie_match_stats_workspace_bytes
    for fl in (0, BOTH):
        assert ws(-1, 100, 10, fl) == INVALID
        assert ws(1, -1, 10, fl) == INVALID
        assert ws(1, 100, -1, fl) == INVALID
        assert ws(1, 100, 2**31, fl) == INVALID
    for fl in (SPLIT, BOTH | SPLIT, 4, 8, -1, 1 << 30, BOTH | 4):
        assert ws(1, 100, 10, fl) == INVALID
    ns = [0, 1, 2, 3, 1000, 10**6]
    ts = [0, 1, 31, 32, 33, 255, 256, 10**4, 10**6, 10**8]
    for fl in (0, BOTH):
        grid = [[ws(n, t, 2**31 - 1, fl) for t in ts] for n in ns]
        for i, n in enumerate(ns):
            for j, t in enumerate(ts):
                assert grid[i][j] > 0 and grid[i][j] % 256 == 0
                assert grid[i][j] <= ms(n, t, 2**31 - 1, fl), (fl, n, t)
                assert grid[i][j] == ws(n, t, 0, fl)               # max_len is a bound for the check, not a size
                if i:
                    assert grid[i][j] >= grid[i - 1][j], (fl, i, j)
                if j:
                    assert grid[i][j] >= grid[i][j - 1], (fl, i, j)
    # what the header says: the packed stream alone, 0.25 bytes per position; 28 bytes per pattern, 88 with both strands
    assert ws(10, 10**8, 10**8, 0) < 0.26 * 10**8
    assert ws(10, 10**8, 10**8, BOTH) < 2 * 0.26 * 10**8
    assert 28 * 10**6 <= ws(10**6, 0, 0, 0) < 28.1 * 10**6
    assert 88 * 10**6 <= ws(10**6, 0, 0, BOTH) < 88.1 * 10**6


def test_exact_match_argument_checks_before_device(pkg):
    lib = pkg._native.lib()
    ref = np.random.default_rng(1).integers(0, 4, 2000).astype(np.uint8)
    h = C.c_void_p(0)
    assert lib.genie_index_create(ref.ctypes.data_as(C.POINTER(C.c_uint8)), ref.size, 8, 0, C.byref(h)) == 0
    try:
        buf = np.zeros(1 << 16, np.uint8)
        al = (buf.ctypes.data + 255) & ~255
        p = C.c_void_p(al)
        for fl in (0, BOTH):
            bytes_ok = lib.genie_exact_match_workspace_bytes(2, 100, 100, fl)
            assert 0 < bytes_ok <= (1 << 16) - 256

            def call(ix=h, flags=fl, bases=p, offs=p, n=2, total=100, max_len=100, lohi=p, cnt=p, st=p, wsp=p, wsb=bytes_ok):
                return lib.genie_exact_match(ix, flags, bases, offs, n, total, max_len, lohi, cnt, st, wsp, wsb, None)

            assert call(ix=None) == INVALID
            assert call(n=-1) == INVALID
            assert call(total=-1) == INVALID
            assert call(max_len=-1) == INVALID
            assert call(max_len=2**31) == INVALID
            assert call(wsb=-1) == INVALID
            assert call(offs=None) == INVALID
            assert call(lohi=None) == INVALID
            assert call(bases=None) == INVALID
            assert call(flags=fl | SPLIT) == INVALID                # a pattern with a break has no interval
            assert call(flags=fl | 4) == INVALID                    # an unknown flag bit
            assert call(flags=fl | (1 << 20)) == INVALID
            assert call(flags=-1) == INVALID
            assert call(lohi=C.c_void_p(al + 4)) == INVALID         # d_lohi 8-byte aligned
            assert call(lohi=C.c_void_p(al + 1)) == INVALID
            assert call(cnt=C.c_void_p(al + 2)) == INVALID          # d_counts 4-byte aligned
            assert call(st=C.c_void_p(al + 2)) == INVALID           # d_status 4-byte aligned
            assert call(st=C.c_void_p(al + 1)) == INVALID
            assert call(wsp=None) == CAPACITY
            assert call(wsp=C.c_void_p(al + 16)) == CAPACITY        # workspace 256-byte aligned
            assert call(wsb=bytes_ok - 1) == CAPACITY
            assert call(wsb=0) == CAPACITY
            assert call(lohi=None, wsp=None) == INVALID             # a bad argument is reported before a capacity
            assert call(flags=fl | SPLIT, wsb=0) == INVALID
            assert call() == NO_DEVICE                              # every argument was fine
            assert call(cnt=None) == NO_DEVICE and call(st=None) == NO_DEVICE and call(cnt=None, st=None) == NO_DEVICE
            assert call(lohi=C.c_void_p(al + 8), cnt=C.c_void_p(al + 4), st=C.c_void_p(al + 12)) == NO_DEVICE
            assert call(total=0, bases=None) == NO_DEVICE           # empty patterns only
            assert call(n=0, offs=None, lohi=None, wsp=None, wsb=0, total=0, bases=None, cnt=None, st=None) == NO_DEVICE
            assert call(n=0, offs=None, lohi=None, wsp=None, wsb=0) == NO_DEVICE     # bases that belong to no pattern
    finally:
        lib.genie_index_destroy(h)


def test_python_layer_refuses_a_host_only_handle(pkg):
    ref = np.random.default_rng(2).integers(0, 4, 3000).astype(np.uint8)
    ix = pkg.GenieIndex.build(ref, 8)                               # host-only: no device was touched
    assert callable(ix.exact_match) and callable(pkg.ExactMatch.exact_match_text)
    with pytest.raises(Exception):
        ix.exact_match(np.zeros(10, np.uint8), np.asarray([0, 10], np.int64))


# ------------------------------------------------------------------ the restatement against hand-made cases
def _codes(s):
    return np.asarray(["ACGT".index(c) if c in "ACGT" else 4 for c in s], np.uint8)


def _sa(ref_str):
    """Suffix rows of a short string by sorting the suffixes here ('$' smallest)."""
    return sorted(range(len(ref_str) + 1), key=lambda s: ref_str[s:])


def test_restatement_on_hand_made_cases():
    ref_str = "ACGTACGAATTC"                                        # holds the palindrome GAATTC and AATT
    ref = _codes(ref_str)
    rows = U.suffix_rows(ref)
    n = len(ref)
    assert rows.tolist() == _sa(ref_str)

    def rows_of(s):                                                  # by hand: the rows whose suffix starts with s
        hit = [r for r, at in enumerate(rows.tolist()) if ref_str[at:].startswith(s)]
        assert hit == list(range(hit[0], hit[-1] + 1)) if hit else True
        return (hit[0], hit[-1]) if hit else (-1, -1)

    pats = ["ACG", "GAATTC", "AATT", "", "TTT", "NCG", "ACN", "N", "C", "ACGTACGAATTC", "ACGTACGAATTCA", "CGT"]
    for flags in (0, BOTH):
        strands = 2 if flags else 1
        lohi, cnt, st = EM.expected(ref, [_codes(p) for p in pats], flags)
        assert lohi.shape == (strands * len(pats), 2) and cnt.shape == st.shape == (strands * len(pats),)
        for i, p in enumerate(pats):
            q = strands * i
            if "N" in p:
                assert tuple(lohi[q]) == EM.BAD and cnt[q] == 0 and st[q] == EM.READ_BAD_BASE
                continue
            want = (0, n) if p == "" else rows_of(p)
            assert tuple(lohi[q]) == want and st[q] == EM.READ_OK
            assert cnt[q] == ref_str.count(p) if p else cnt[q] == n + 1
    lohi, cnt, st = EM.expected(ref, [_codes(p) for p in pats], BOTH)
    by = {p: i for i, p in enumerate(pats)}
    # a palindrome is its own reverse complement: both strands give the same rows
    for p in ("GAATTC", "AATT", ""):
        assert EM.rc(_codes(p)).tolist() == _codes(p).tolist()
        assert tuple(lohi[2 * by[p]]) == tuple(lohi[2 * by[p] + 1]) and cnt[2 * by[p]] == cnt[2 * by[p] + 1] > 0
    # rc(CGT) = ACG: strand 1 of one is strand 0 of the other
    assert tuple(lohi[2 * by["CGT"] + 1]) == tuple(lohi[2 * by["ACG"]]) == rows_of("ACG") and cnt[2 * by["ACG"]] == 2
    assert tuple(lohi[2 * by["ACG"] + 1]) == rows_of("CGT")
    # a code > 3 at the first or the last base is bad on both strands, and stays a code > 3 when reversed
    for p in ("NCG", "ACN", "N"):
        assert EM.rc(_codes(p)).tolist() == [4 if c == "N" else 3 - "ACGT".index(c) for c in reversed(p)]
        for s in (0, 1):
            q = 2 * by[p] + s
            assert tuple(lohi[q]) == EM.BAD and cnt[q] == 0 and st[q] == EM.READ_BAD_BASE
    # the interleaved batch: BOTH is the call without it on [p0, rc(p0), ...]
    one = EM.expected(ref, EM.strand_patterns([_codes(p) for p in pats], 2), 0)
    assert all(np.array_equal(x, y) for x, y in zip((lohi, cnt, st), one))


def test_restatement_on_a_reference_without_t():
    ref = _codes("ACGGCAACCGAGA")
    n = len(ref)
    pats = [_codes("AAAA"), _codes("A"), _codes("T"), _codes("TC"), _codes("GGC"), _codes("")]
    lohi, cnt, st = EM.expected(ref, pats, BOTH)
    assert not st.any()                                             # a base the reference lacks is no bad base
    assert tuple(lohi[0]) == (-1, -1) and tuple(lohi[1]) == (-1, -1) and cnt[0] == cnt[1] == 0      # AAAA, TTTT
    assert cnt[2] == 5 and tuple(lohi[3]) == (-1, -1) and cnt[3] == 0          # A occurs, its complement T does not
    assert tuple(lohi[4]) == (-1, -1) and cnt[5] == 5                          # T absent, rc(T) = A
    assert cnt[6] == 0 and cnt[7] == 2                                         # TC absent, rc(TC) = GA twice
    assert cnt[8] == 1 and cnt[9] == 0                                         # GGC once, rc(GGC) = GCC nowhere
    assert tuple(lohi[10]) == tuple(lohi[11]) == (0, n) and cnt[10] == cnt[11] == n + 1
    # counts are occurrences, whatever the strand
    for q, p in enumerate(EM.strand_patterns(pats, 2)):
        assert cnt[q] == len(EM.occurrences(ref, p))
