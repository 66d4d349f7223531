"""CPU-only tests of genie_match_stats_min_occ and genie_find_smems_min_occ: the symbols, the size functions, the C ABI's
argument checks (before the device check, so a host-only handle reaches them), the facts of the header and the two
restatements of tests/min_occ_util.py against each other on every case the GPU tests run, a guard against a vacuous suite,
and the ACGTACGTTT / ACGTT example as a known answer."""
import ctypes as C
import os

import numpy as np
import pytest

import lookup_util as U
import match_stats_util as MS
import min_occ_util as MO
import smem_util as SM

BOTH, SPLIT, FLAGS, KS = MO.BOTH, MO.SPLIT, MO.FLAGS, MO.KS
INVALID, NO_DEVICE, CAPACITY = -1, -4, -10
CASES = list(MO.cases())


@pytest.fixture(scope="module")
def pkg():
    import genie_smem_amd as g
    g._native.build()
    return g


def test_min_occ_symbols_exported(pkg):
    lib = pkg._native.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "genie_smem.h")).read()
    for name, nargs, res in (("genie_match_stats_min_occ", 15, C.c_int), ("genie_match_stats_min_occ_workspace_bytes", 4, C.c_int64),
                             ("genie_find_smems_min_occ", 18, C.c_int), ("genie_find_smems_min_occ_workspace_bytes", 4, C.c_int64)):
        assert name in pkg._native.SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is res and len(fn.argtypes) == nargs
        assert name + "(" in header
    assert lib.genie_abi_version() == 2 and pkg._native.ABI_VERSION == 2      # additions: the version stays
    assert "#define GENIE_ABI_VERSION 2" in header


def test_size_functions(pkg):
    lib = pkg._native.lib()
    for ws, parent in ((lib.genie_match_stats_min_occ_workspace_bytes, lib.genie_match_stats_workspace_bytes),
                       (lib.genie_find_smems_min_occ_workspace_bytes, lib.genie_find_smems_long_ex_workspace_bytes)):
        for fl in FLAGS:
            assert ws(-1, 100, 10, fl) == INVALID
            assert ws(1, -1, 10, fl) == INVALID
            assert ws(1, 100, -1, fl) == INVALID
            assert ws(1, 100, 2**31, fl) == INVALID
        for fl in (4, 8, -1, BOTH | 4):
            assert ws(1, 100, 10, fl) == INVALID
        ns, ts = [0, 1, 3, 1000, 10**6], [0, 1, 255, 256, 257, 10**4, 10**8]
        for fl in FLAGS:
            grid = np.asarray([[ws(n, t, 2**31 - 1, fl) for t in ts] for n in ns], np.int64)
            want = np.asarray([[parent(n, t, 2**31 - 1, fl) for t in ts] for n in ns], np.int64)
            assert (grid > 0).all() and (grid % 256 == 0).all() and (grid >= want).all()
            assert (np.diff(grid, axis=0) >= 0).all() and (np.diff(grid, axis=1) >= 0).all()
            assert ws(1000, 10**4, 0, fl) == ws(1000, 10**4, 2**31 - 1, fl)      # max_len is a bound for the checks alone


def test_argument_checks_before_device(pkg):
    lib = pkg._native.lib()
    ref = np.random.default_rng(1).integers(0, 4, 2000).astype(np.uint8)
    h = C.c_void_p(0)
    assert lib.genie_index_create(ref.ctypes.data_as(C.POINTER(C.c_uint8)), ref.size, 8, 0, C.byref(h)) == 0
    try:
        buf = np.zeros(1 << 17, np.uint8)
        al = (buf.ctypes.data + 255) & ~255
        p = C.c_void_p(al)
        odd8, odd4, odd16 = C.c_void_p(al + 4), C.c_void_p(al + 2), C.c_void_p(al + 8)
        for fl in FLAGS:
            ms_ok = lib.genie_match_stats_min_occ_workspace_bytes(2, 100, 100, fl)
            assert 0 < ms_ok <= (1 << 17) - 256

            def ms(ix=h, flags=fl, k=2, bases=p, offs=p, n=2, total=100, max_len=100, out=p, lohi=p, st=p, tt=p, wsp=p, wsb=ms_ok):
                return lib.genie_match_stats_min_occ(ix, flags, k, bases, offs, n, total, max_len, out, lohi, st, tt, wsp, wsb, None)

            assert ms() == NO_DEVICE and ms(k=1) == NO_DEVICE and ms(k=2**31 - 1) == NO_DEVICE      # every argument was fine
            for bad in (dict(ix=None), dict(offs=None), dict(bases=None), dict(out=None), dict(n=-1), dict(total=-1), dict(max_len=-1),
                        dict(max_len=2**31), dict(wsb=-1), dict(flags=fl | 4), dict(flags=-1), dict(out=odd4), dict(lohi=odd8),
                        dict(tt=odd8), dict(k=0), dict(k=-3)):
                assert ms(**bad) == INVALID, bad
            assert ms(wsp=None) == CAPACITY and ms(wsp=C.c_void_p(al + 16)) == CAPACITY and ms(wsb=ms_ok - 1) == CAPACITY
            assert ms(k=0, wsp=None) == INVALID and ms(tt=odd8, wsb=0) == INVALID      # a bad argument comes before a capacity
            assert ms(n=0, offs=None, wsp=None, wsb=0) == NO_DEVICE
            assert ms(lohi=None) == NO_DEVICE and ms(st=None, tt=None) == NO_DEVICE

            sm_ok = lib.genie_find_smems_min_occ_workspace_bytes(2, 100, 100, fl)
            assert ms_ok <= sm_ok <= (1 << 17) - 256

            def sm(ix=h, mode=0, flags=fl, bases=p, offs=p, n=2, total=100, max_len=100, m=1, k=2, out=p, rows=p, cap=10, st=p, tt=p,
                   wsp=p, wsb=sm_ok):
                return lib.genie_find_smems_min_occ(ix, mode, flags, bases, offs, n, total, max_len, m, k, out, rows, cap, st, tt, wsp, wsb,
                                                    None)

            assert sm() == NO_DEVICE and sm(k=1) == NO_DEVICE
            # the parent's checks: a missing or misaligned workspace is a bad argument there, a small one a capacity
            for bad in (dict(ix=None), dict(out=None), dict(offs=None), dict(bases=None), dict(rows=None), dict(n=-1), dict(total=-1),
                        dict(max_len=-1), dict(max_len=2**31), dict(cap=-1), dict(mode=-1), dict(mode=3), dict(flags=fl | 4),
                        dict(flags=-1), dict(rows=odd16), dict(wsp=None), dict(wsp=C.c_void_p(al + 16)), dict(tt=odd8), dict(k=0),
                        dict(k=-1)):
                assert sm(**bad) == INVALID, bad
            if fl & SPLIT:
                assert sm(mode=1) == INVALID and sm(mode=2) == INVALID      # SPLIT_BREAKS has the BWA traversal alone
            else:
                assert sm(mode=1) == NO_DEVICE and sm(mode=2) == NO_DEVICE  # the tables a mode needs are looked at last
            assert sm(wsb=sm_ok - 1) == CAPACITY and sm(wsb=sm_ok - 1, k=0) == INVALID
            assert sm(n=0, offs=None, rows=None, wsp=None, wsb=0) == NO_DEVICE and sm(n=0, out=None, wsp=None, wsb=0) == INVALID
            assert sm(st=None, tt=None) == NO_DEVICE and sm(cap=0) == NO_DEVICE
    finally:
        lib.genie_index_destroy(h)


def test_python_layer_refuses_a_host_only_handle(pkg):
    ix = pkg.GenieIndex.build(U.family()["rand4096"][:500], 8)     # host-only: no device was touched
    for fn in (ix.match_stats_min_occ, ix.find_smems_min_occ, pkg.SMEM.match_stats_min_occ, pkg.SMEM.find_smems_min_occ):
        assert callable(fn)
    with pytest.raises(Exception):
        ix.match_stats_min_occ(np.zeros(10, np.uint8), np.asarray([0, 10], np.int64), 2)
    with pytest.raises(Exception):
        ix.find_smems_min_occ("bwa", np.zeros(10, np.uint8), np.asarray([0, 10], np.int64), 2)


# ------------------------------------------------------------------ the brute force
KNOWN_REF, KNOWN_READ = "ACGTACGTTT", "ACGTT"
KNOWN = {1: ([5, 4, 3, 2, 1], [[0, 5]]), 2: ([4, 3, 2, 2, 1], [[0, 4], [3, 5]])}      # k -> (ms_k, the SMEMs' (start, end))


def test_the_example_of_the_header():
    """Reference ACGTACGTTT, read ACGTT.  The read occurs once, at position 4, so ms = 5, 4, 3, 2, 1 with the single SMEM
    (0, 5); ACGT and TT occur twice and GTT once, so k = 2 gives 4, 3, 2, 2, 1 and the SMEMs (0, 4) and (3, 5).  (The request
    for this feature wrote 1, 4, 3, 2, 1 and (1, 5) for k = 1, which no reading of its own definition gives: ms_1 = ms, and
    ms[0] = 5 by plain substring search, asserted below without any of the restatements.)"""
    ref, read = U._codes(KNOWN_REF), U._codes(KNOWN_READ)
    assert KNOWN_REF.find(KNOWN_READ) == 4 and KNOWN_REF.count("ACGT") == 2 and KNOWN_REF.count("GTT") == 1
    rows = U.suffix_rows(ref)
    for ms_k in (MO.ms_k_naive, MO.ms_k_by_rows):
        ms, lohi, status, short = MO.expected_one(ref, read, False, 1, ms_k)
        assert ms.tolist() == KNOWN[1][0] and status == 0 and short == 0
        ms, lohi, status, short = MO.expected_one(ref, read, False, 2, ms_k)
        assert ms.tolist() == KNOWN[2][0] and status == 0 and short == 3
        assert lohi.tolist() == [list(U.interval(ref, rows, read[p:p + l])) for p, l in enumerate(KNOWN[2][0])]
    assert MS.expected_one(ref, read, False)[0].tolist() == KNOWN[1][0]
    assert MO.smems_one(ref, read, False, 1)[0][:, :2].tolist() == KNOWN[1][1]
    got, status, short = MO.smems_one(ref, read, False, 2)
    assert got[:, :2].tolist() == [[0, 4], [3, 5]] and status == 0 and short == 3
    assert ((got[:, 3] - got[:, 2] + 1) >= 2).all()


def _units(c, split, k):
    """Every break-free run of every strand-read of the case that is not flagged GENIE_READ_BAD_BASE."""
    for q in MS.strand_reads(c.reads, 2):
        if not split and (q > 3).any():
            continue
        for a, b in MO._runs(q, c.ref, split, k):
            yield q[a:b]


def _occ(ref, pat):
    r, p = U._bytes(ref), U._bytes(pat)
    return sum(r.startswith(p, t) for t in range(len(r) - len(p) + 1))


@pytest.mark.parametrize("name", CASES)
def test_the_facts_and_the_two_restatements(name):
    c = MO.case(name)
    for split in (False, True):
        before = {}
        for k in KS:
            for i, run in enumerate(_units(c, False, k)) if not split else ():
                a, b = MO.ms_k_naive(c.ref, run, k), MO.ms_k_by_rows(c.ref, run, k)
                assert np.array_equal(a, b), (name, k)                          # facts 3 and 5
                ms = SM.matching_stats(c.ref, run) - np.arange(len(run))
                assert (a <= ms).all() and (k > 1 or np.array_equal(a, ms))     # fact 1
                assert np.array_equal(a == 0, ~np.isin(run, MO.usable(c.ref, k)))
                assert (a <= before.get(i, a)).all()                            # ... non-increasing in k
                before[i] = a
                assert (a[1:] >= a[:-1] - 1).all()                              # fact 2
            for run in _units(c, True, k) if split else ():
                a = MO.ms_k_naive(c.ref, run, k)
                assert np.array_equal(a, MO.ms_k_by_rows(c.ref, run, k)) and (a >= 1).all() and (a[1:] >= a[:-1] - 1).all()
    for k in KS:
        for flags in FLAGS:
            x = MO.expected_ms(c.ref, c.reads, flags, k)
            y = MO.expected_ms(c.ref, c.reads, flags, k, ms_k=MO.ms_k_by_rows)
            assert all(np.array_equal(p, q) for p, q in zip(x[:3], y[:3])) and x[3] == y[3]
            offs, rows, st, short = MO.expected_smems(c.ref, c.reads, flags, k)
            assert ((rows[:, 3] - rows[:, 2] + 1) >= k).all()
            if k == 1:                                                          # k = 1 is the parents
                assert all(np.array_equal(p, q) for p, q in zip(x[:3], MS.expected(c.ref, c.reads, flags))) and x[3] == 0
                w = SM.expected_batch(c.ref, MS.strand_reads(c.reads, 2 if flags & BOTH else 1), "bwa", 1, split=bool(flags & SPLIT))
                assert np.array_equal(offs, w[0]) and np.array_equal(rows, w[1]) and np.array_equal(st, w[2]) and short == 0


def test_the_defining_properties_on_the_restatement():
    """One base more occurs fewer than k times wherever ms_k < ms, and no SMEM row extends by a base on either side."""
    c = MO.case("iid")
    for k in (2, 3):
        for q in MS.strand_reads(c.reads[6:9], 2):
            ms_k = MO.ms_k_naive(c.ref, q, k)
            ms = SM.matching_stats(c.ref, q) - np.arange(len(q))
            for p in np.flatnonzero(ms_k < ms)[::7]:
                assert _occ(c.ref, q[p:p + ms_k[p]]) >= k > _occ(c.ref, q[p:p + ms_k[p] + 1])
            rows, status, _ = MO.smems_one(c.ref, q, False, k)
            for s, e, lo, hi in rows.tolist():
                assert hi - lo + 1 == _occ(c.ref, q[s:e]) >= k
                assert s == 0 or _occ(c.ref, q[s - 1:e]) < k
                assert e == len(q) or _occ(c.ref, q[s:e + 1]) < k


def test_the_suite_is_not_vacuous():
    """Over the cases taken together, on every flag combination and some k >= 2: a position has 0 < ms_k < ms, a failed run
    start resolves a later position at full length, a row set differs from the parent's, and a strand-read is flagged or
    broken only because of a base rare at k.  Also the shapes the GPU tests name."""
    for flags in FLAGS:
        split = bool(flags & SPLIT)
        shortened = kept = differ = rare = 0
        for name in CASES:
            c = MO.case(name)
            for k in (2, 11):
                seen = {}
                for run in _units(c, split, k):
                    MO.ms_k_by_rows(c.ref, run, k, seen)
                shortened += seen.get("shortened", 0)
                kept += seen.get("kept", 0)
                got = MO.expected_smems(c.ref, c.reads, flags, k)
                want = MO.expected_smems(c.ref, c.reads, flags, 1)
                differ += not (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]))
                x, y = MO.expected_ms(c.ref, c.reads, flags, k), MS.expected(c.ref, c.reads, flags)
                if split:                                                       # a break where the parent has a match
                    rare += int(((x[0] == 0) & (y[0] > 0)).sum())
                else:
                    rare += int(((x[2] == MS.READ_ABSENT_BASE) & (y[2] == MS.READ_OK)).sum())
        assert shortened > 0 and kept > 0 and differ > 0 and rare > 0, (flags, shortened, kept, differ, rare)
    # iid: the repeat read fails at its start and keeps ms from position 20 on; run starts at 255 and 256; a run of 720
    c = MO.case("iid")
    rep, at255, at256, three = c.reads[6:10]
    ms2, ms = MO.ms_k_naive(c.ref, rep, 2), SM.matching_stats(c.ref, rep) - np.arange(len(rep))
    assert ms[0] == 80 and ms2[0] < 80 and np.array_equal(ms2[20:], ms[20:]) and ms2[20] == 60
    for read, at in ((at255, 255), (at256, 256), (three, 0)):
        fwd = SM.matching_stats(c.ref, read)
        assert fwd[at] == len(read) and (at == 0 or fwd[at - 1] != fwd[at])
        assert MO.ms_k_naive(c.ref, read, 2)[at] < fwd[at] - at
    assert len(three) == 720 and (SM.matching_stats(c.ref, three) == 720).all()
    assert sorted(len(r) for r in c.reads[:6]) == [255, 256, 257, 511, 512, 513]
    # tandem: intervals of more than 32 and of more than 64 rows, and k on both sides of them
    for name in CASES:
        if U.is_tandem(name):
            c = MO.case(name)
            lo, hi = U.interval(c.ref, U.suffix_rows(c.ref), c.reads[0])
            assert hi - lo + 1 > 65
            for k in (32, 33, 65):
                x = MO.expected_ms(c.ref, c.reads, 0, k)
                assert x[3] > 0 and (x[0] == MS.expected(c.ref, c.reads, 0)[0]).any()
    # once: T is rare at 2 and is in the reference
    c = MO.case("once")
    assert MO.usable(c.ref, 1).tolist() == [0, 1, 2, 3] and MO.usable(c.ref, 2).tolist() == [0, 1, 2] and len(c.ref) == 12
    # passes: with SPLIT_BREAKS more units than the workspace is sized for (one per 32 positions and one per strand-read)
    c = MO.case("passes")
    units = sum(len(MO._runs(q, c.ref, True, 2)) for q in MS.strand_reads(c.reads, 1))
    assert units > 2 * (len(c.reads) + sum(len(r) for r in c.reads) // 32 + 64)
