"""CPU-only tests of genie_match_stats_contigs and genie_find_smems_contigs: the symbols, the size functions, the C ABI's
argument checks (before the device check, so a host-only handle reaches them), the four facts of the header and the two
restatements of tests/contig_stats_util.py against each other on every case the GPU tests run, a guard against a vacuous
suite, and the ACGT | TTGA example as a known answer."""
import ctypes as C
import os

import numpy as np
import pytest

import contig_stats_util as CS
import contig_util as CU
import lookup_util as U
import match_stats_util as MS
import smem_util as SM

BOTH, SPLIT, FLAGS = CS.BOTH, CS.SPLIT, CS.FLAGS
INVALID, NO_DEVICE, TOO_LONG, CAPACITY = -1, -4, -6, -10
CASES = list(CS.cases())


@pytest.fixture(scope="module")
def pkg():
    import genie_smem_amd as g
    g._native.build()
    return g


def test_contig_stats_symbols_exported(pkg):
    lib = pkg._native.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "genie_smem.h")).read()
    for name, nargs, res in (("genie_match_stats_contigs", 16, C.c_int), ("genie_match_stats_contigs_workspace_bytes", 5, C.c_int64),
                             ("genie_find_smems_contigs", 19, C.c_int), ("genie_find_smems_contigs_workspace_bytes", 5, C.c_int64)):
        assert name in pkg._native.SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is res and len(fn.argtypes) == nargs
        assert name + "(" in header
    assert lib.genie_abi_version() == 2 and pkg._native.ABI_VERSION == 2      # additions: the version stays
    assert "#define GENIE_ABI_VERSION 2" in header


def test_size_functions(pkg):
    lib = pkg._native.lib()
    for ws, parent in ((lib.genie_match_stats_contigs_workspace_bytes, lib.genie_match_stats_workspace_bytes),
                       (lib.genie_find_smems_contigs_workspace_bytes, lib.genie_find_smems_long_ex_workspace_bytes)):
        for fl in FLAGS:
            assert ws(-1, 100, 10, fl, 1) == INVALID
            assert ws(1, -1, 10, fl, 1) == INVALID
            assert ws(1, 100, -1, fl, 1) == INVALID
            assert ws(1, 100, 2**31, fl, 1) == INVALID
            assert ws(1, 100, 10, fl, 0) == INVALID
            assert ws(1, 100, 10, fl, -5) == INVALID
            assert ws(1, 100, 10, fl, 2**31 - 1) == INVALID
        for fl in (4, 8, -1, BOTH | 4):
            assert ws(1, 100, 10, fl, 1) == INVALID
        ns, ts, cs = [0, 1, 3, 1000, 10**6], [0, 1, 255, 256, 257, 10**4, 10**8], [1, 2, 1023, 1024, 10**4, 10**7]
        for fl in FLAGS:
            grid = np.asarray([[[ws(n, t, 2**31 - 1, fl, c) for c in cs] for t in ts] for n in ns], np.int64)
            assert (grid > 0).all() and (grid % 256 == 0).all()
            assert (np.diff(grid, axis=0) >= 0).all() and (np.diff(grid, axis=1) >= 0).all() and (np.diff(grid, axis=2) >= 0).all()
            for i, n in enumerate(ns):
                for j, t in enumerate(ts):
                    assert (grid[i, j] >= parent(n, t, 2**31 - 1, fl)).all()
                    assert ws(n, t, 0, fl, 5) == ws(n, t, 2**31 - 1, fl, 5)      # max_len is a bound for the checks alone


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

        def table_checks(call):
            assert call(ix=None) == INVALID
            assert call(tab=None) == INVALID
            assert call(tab=odd8) == INVALID                        # the table is 8-byte aligned
            assert call(nc=0) == INVALID and call(nc=-1) == INVALID
            assert call(nc=2**31 - 1) == TOO_LONG
            assert call() == NO_DEVICE                              # every argument was fine
            assert call(nc=2**31 - 2) == NO_DEVICE

        for fl in FLAGS:
            ms_ok = lib.genie_match_stats_contigs_workspace_bytes(2, 100, 100, fl, 3)
            assert 0 < ms_ok <= (1 << 17) - 256

            def ms(ix=h, tab=p, nc=3, flags=fl, bases=p, offs=p, n=2, total=100, max_len=100, out=p, lohi=p, st=p, tt=p, wsp=p,
                   wsb=ms_ok):
                return lib.genie_match_stats_contigs(ix, tab, nc, flags, bases, offs, n, total, max_len, out, lohi, st, tt, wsp, wsb, None)

            table_checks(ms)
            for bad in (dict(offs=None), dict(bases=None), dict(out=None), dict(n=-1), dict(total=-1), dict(max_len=-1),
                        dict(max_len=2**31), dict(wsb=-1), dict(flags=fl | 4), dict(flags=-1), dict(out=odd4), dict(lohi=odd8),
                        dict(tt=odd8)):
                assert ms(**bad) == INVALID, bad
            assert ms(wsp=None) == CAPACITY and ms(wsp=C.c_void_p(al + 16)) == CAPACITY and ms(wsb=ms_ok - 1) == CAPACITY
            assert ms(tab=None, wsp=None) == INVALID                # a bad argument is reported before a capacity
            assert ms(nc=2**31 - 1, wsp=None) == TOO_LONG           # ... the table's too; its own checks come behind the others
            assert ms(nc=2**31 - 1, tt=odd8) == INVALID and ms(nc=2**31 - 1, wsb=-1) == INVALID
            assert ms(n=0, offs=None, wsp=None, wsb=0) == NO_DEVICE
            assert ms(lohi=None) == NO_DEVICE and ms(st=None, tt=None) == NO_DEVICE
            assert ms(n=0, wsp=None, wsb=0, total=0, bases=None, out=None) == NO_DEVICE

            sm_ok = lib.genie_find_smems_contigs_workspace_bytes(2, 100, 100, fl, 3)
            assert ms_ok <= sm_ok <= (1 << 17) - 256

            def sm(ix=h, tab=p, nc=3, mode=0, flags=fl, bases=p, offs=p, n=2, total=100, max_len=100, m=1, out=p, rows=p, cap=10,
                   st=p, tt=p, wsp=p, wsb=sm_ok):
                return lib.genie_find_smems_contigs(ix, tab, nc, mode, flags, bases, offs, n, total, max_len, m, out, rows, cap, st, tt,
                                                    wsp, wsb, None)

            table_checks(sm)
            for bad in (dict(out=None), dict(offs=None), dict(bases=None), dict(rows=None), dict(n=-1), dict(total=-1),
                        dict(max_len=-1), dict(max_len=2**31), dict(cap=-1), dict(wsb=-1), dict(mode=-1), dict(mode=3),
                        dict(flags=fl | 4), dict(flags=-1), dict(rows=odd16), dict(tt=odd8)):
                assert sm(**bad) == INVALID, bad
            if fl & SPLIT:
                assert sm(mode=1) == INVALID and sm(mode=2) == INVALID      # SPLIT_BREAKS has the BWA traversal alone
            assert sm(wsp=None) == CAPACITY and sm(wsp=C.c_void_p(al + 16)) == CAPACITY and sm(wsb=sm_ok - 1) == CAPACITY
            assert sm(tab=None, wsp=None) == INVALID
            assert sm(nc=2**31 - 1, wsp=None) == TOO_LONG
            assert sm(nc=2**31 - 1, tt=odd8) == INVALID and sm(nc=2**31 - 1, wsb=-1) == INVALID and sm(nc=2**31 - 1, mode=3) == INVALID
            if not fl & SPLIT:
                assert sm(mode=1) == NO_DEVICE and sm(mode=2) == NO_DEVICE      # the tables a mode needs are looked at last
            assert sm(n=0, offs=None, rows=None, wsp=None, wsb=0) == NO_DEVICE and sm(n=0, out=None, wsp=None, wsb=0) == INVALID
            assert sm(st=None, tt=None) == NO_DEVICE and sm(cap=0) == NO_DEVICE
            assert sm(n=0, wsp=None, wsb=0, total=0, bases=None, rows=None) == NO_DEVICE
    finally:
        lib.genie_index_destroy(h)


def test_python_layer_refuses_a_host_only_handle(pkg):
    rs = pkg.ReferenceSet.from_sequences(["ACGTACGTTGCA" * 30, "", "GGATC" * 50])
    ix = pkg.GenieIndex.build(rs.codes, 8)                         # host-only: no device was touched
    for fn in (ix.match_stats_contigs, ix.find_smems_contigs, pkg.SMEM.match_stats_contigs, pkg.SMEM.find_smems_contigs):
        assert callable(fn)
    with pytest.raises(Exception):
        ix.match_stats_contigs(rs, np.zeros(10, np.uint8), np.asarray([0, 10], np.int64))
    with pytest.raises(Exception):
        ix.find_smems_contigs(rs, "bwa", np.zeros(10, np.uint8), np.asarray([0, 10], np.int64))


# ------------------------------------------------------------------ the brute force
def _codes(s):
    return np.asarray(["ACGT".index(c) for c in s], np.uint8)


def test_the_example_of_the_header():
    ref, off, read = _codes("ACGTTTGA"), [0, 4, 8], _codes("CGTT")
    rows = U.suffix_rows(ref)
    assert MS.expected_one(ref, read, False)[0].tolist() == [4, 3, 2, 1]                  # CGTT occurs once, across the boundary
    assert SM.smems(ref, read, 1)[0][:, :2].tolist() == [[0, 4]]
    assert CU.locate_expected(ref, off, SM.smems(ref, read, 1)[0])[1].shape[0] == 0       # ... and its one occurrence is dropped
    for ms_c in (CS.ms_c_per_contig, CS.ms_c_by_rows):
        ms, lohi, status, clipped = CS.expected_one(ref, off, read, False, ms_c)
        assert ms.tolist() == [3, 2, 2, 1] and status == 0 and clipped == 2
        assert lohi.tolist() == [list(U.interval(ref, rows, read[p:p + l])) for p, l in enumerate([3, 2, 2, 1])]
    got, status, clipped = CS.smems_one(ref, off, read, False)
    assert got[:, :2].tolist() == [[0, 3], [2, 4]] and status == 0 and clipped == 2
    ho, hits, dropped = CU.locate_expected(ref, off, got)
    assert (np.diff(ho) >= 1).all() and [0, 2] in hits.tolist() and [1, 1] in hits.tolist()


def _units(c, split):
    """Every break-free run of every strand-read of the case that is not flagged GENIE_READ_BAD_BASE."""
    for q in MS.strand_reads(c.reads, 2):
        if not split and (q > 3).any():
            continue
        for a, b in CS._runs(q, c.ref, split):
            yield q[a:b]


@pytest.mark.parametrize("name", CASES)
def test_the_facts_and_the_two_restatements(name):
    c = CS.case(name)
    for split in (False, True):
        for run in _units(c, split):
            a, b = CS.ms_c_per_contig(c.ref, c.off, run), CS.ms_c_by_rows(c.ref, c.off, run)
            assert np.array_equal(a, b), (name, split)                      # facts 3 and 4
            ms = SM.matching_stats(c.ref, run) - np.arange(len(run))
            assert (a <= ms).all() and np.array_equal(a >= 1, ms >= 1)      # fact 1
            assert (a[1:] >= a[:-1] - 1).all()                              # fact 2
    for flags in FLAGS:
        x = CS.expected_ms(c.ref, c.off, c.reads, flags)
        y = CS.expected_ms(c.ref, c.off, c.reads, flags, ms_c=CS.ms_c_by_rows)
        assert all(np.array_equal(p, q) for p, q in zip(x[:3], y[:3])) and x[3] == y[3]
        assert np.array_equal(x[2], MS.expected(c.ref, c.reads, flags)[2])  # the statuses are the parent's
        if c.n_contigs == 1:
            assert all(np.array_equal(p, q) for p, q in zip(x[:3], MS.expected(c.ref, c.reads, flags))) and x[3] == 0
        # every row of the contig-exact SMEMs has an occurrence inside one contig
        offs, rows, st, clipped = CS.expected_smems(c.ref, c.off, c.reads, flags)
        ho, _, _ = CU.locate_expected(c.ref, c.off, rows)
        assert (np.diff(ho) >= 1).all(), (name, flags)
        if c.n_contigs == 1:
            w = CS.concat_smems(c.ref, c.reads, flags)
            assert np.array_equal(offs, w[0]) and np.array_equal(rows, w[1]) and np.array_equal(st, w[2])


def test_the_suite_is_not_vacuous():
    """Over the cases taken together, on every flag combination: a position is clipped, a flagged run resolves a position
    through another occurrence at full length, and a row set differs from that of the concatenation.  Also the shapes the
    GPU tests name: whole-wave intervals with no row, and with only the last row, inside one contig; run starts on either
    side of a window boundary; a flagged run over three windows; more than 1023 contigs."""
    for flags in FLAGS:
        split = bool(flags & SPLIT)
        clipped = kept = differ = 0
        for name in CASES:
            c = CS.case(name)
            seen = {}
            for run in _units(c, split):
                CS.ms_c_by_rows(c.ref, c.off, run, seen)
            clipped += seen.get("clipped", 0)
            kept += seen.get("kept", 0)
            got, want = CS.expected_smems(c.ref, c.off, c.reads, flags), CS.concat_smems(c.ref, c.reads, flags)
            differ += not (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]))
        assert clipped > 0 and kept > 0 and differ > 0, (flags, clipped, kept, differ)
    # the junction batch: rows of the concatenation without a hit
    c = CS.case("junction")
    plain = CS.concat_smems(c.ref, c.reads, 0)[1]
    assert (np.diff(CU.locate_expected(c.ref, c.off, plain)[0]) == 0).any()
    # junction_short: the bisection ends strictly between the largest room and ms
    c = CS.case("junction_short")
    ms_c, ms = CS.expected_ms(c.ref, c.off, c.reads, 0)[0], MS.expected(c.ref, c.reads, 0)[0]
    assert ((ms_c == ms - 1) & (ms > 30)).any()
    # tandem: intervals of more than 64 rows, none with room; and one where only the last row has it
    none = last = 0
    for name in CASES:
        if not U.is_tandem(name):
            continue
        c = CS.case(name)
        rows = U.suffix_rows(c.ref)
        for r in c.reads[:2]:
            lo, hi = U.interval(c.ref, rows, r)
            t = rows[lo:hi + 1]
            ok = c.off[CU.contig_of(c.off, t) + 1] - t >= len(r)
            none += hi - lo + 1 > 64 and not ok.any()
            last += hi - lo + 1 > 64 and ok[-1] and not ok[:-1].any()
    assert none > 0 and last > 0, (none, last)
    # windows: a flagged run starts at position 255, one at 256, one covers positions 0 .. 600
    c = CS.case("windows")
    last_r, first_r, three = c.reads[-3:]
    for read, at in ((last_r, 255), (first_r, 256), (three, 0)):
        fwd = SM.matching_stats(c.ref, read)
        assert fwd[at] == len(read) and (at == 0 or fwd[at - 1] != fwd[at])
        assert CS.ms_c_per_contig(c.ref, c.off, read)[at] < fwd[at] - at
    assert (SM.matching_stats(c.ref, three)[:600] == len(three)).all()
    assert sorted(len(r) for r in c.reads[:6]) == [255, 256, 257, 511, 512, 513]
    assert max(CS.case(n).n_contigs for n in CASES) > 1023
    # passes: with SPLIT_BREAKS more units than the workspace is sized for (one per 32 positions and one per strand-read)
    c = CS.case("passes")
    units = sum(len(CS._runs(q, c.ref, True)) for q in MS.strand_reads(c.reads, 1))
    assert units > 2 * (len(c.reads) + sum(len(r) for r in c.reads) // 32 + 64)
