"""CPU-only tests of the contig calls (genie_contigs_validate, genie_find_mems_contigs, genie_locate_contigs,
genie_contig_coords): the symbols, the size functions, the C ABI's argument checks (before the device check, so a host-only
handle reaches them), the two restatements of tests/contig_util.py against each other on every case the GPU tests run, a
guard against a vacuous suite, and ReferenceSet.from_sequences."""
import ctypes as C
import os

import numpy as np
import pytest

import contig_util as CU
import lookup_util as U
import mems_util as MM

BOTH, SPLIT, FLAGS = CU.BOTH, CU.SPLIT, CU.FLAGS
INVALID, NO_DEVICE, TOO_LONG, CAPACITY = -1, -4, -6, -10
CASES = list(CU.cases())


@pytest.fixture(scope="module")
def pkg():
    import genie_smem_amd as g
    g._native.build()
    return g


def test_contig_symbols_exported(pkg):
    lib = pkg._native.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "genie_smem.h")).read()
    for name, nargs, res in (("genie_contigs_validate", 4, C.c_int), ("genie_find_mems_contigs", 19, C.c_int),
                             ("genie_find_mems_contigs_workspace_bytes", 5, C.c_int64), ("genie_locate_contigs", 12, C.c_int),
                             ("genie_locate_contigs_tmp_bytes", 1, C.c_int64), ("genie_contig_coords", 8, C.c_int)):
        assert name in pkg._native.SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is res and len(fn.argtypes) == nargs
        assert name + "(" in header
    assert lib.genie_abi_version() == 2 and pkg._native.ABI_VERSION == 2      # additions: the version stays
    assert "#define GENIE_ABI_VERSION 2" in header


def test_size_functions(pkg):
    lib = pkg._native.lib()
    ws, parent, tmp = lib.genie_find_mems_contigs_workspace_bytes, lib.genie_find_mems_workspace_bytes, lib.genie_locate_contigs_tmp_bytes
    for fl in FLAGS:
        assert ws(-1, 100, 10, fl, 1) == INVALID
        assert ws(1, -1, 10, fl, 1) == INVALID
        assert ws(1, 100, -1, fl, 1) == INVALID
        assert ws(1, 100, 2**31, fl, 1) == INVALID
        assert ws(1, 100, 10, fl, 0) == INVALID
        assert ws(1, 100, 10, fl, -5) == INVALID
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
                # what the table adds is a function of n_contigs alone
                assert np.array_equal(grid[i, j] - parent(n, t, 2**31 - 1, fl), grid[0, 0] - parent(ns[0], ts[0], 2**31 - 1, fl))
    assert tmp(-1) == INVALID
    sizes = [tmp(s) for s in (0, 1, 255, 256, 257, 10**4, 10**7)]
    assert all(x >= 0 and x % 256 == 0 for x in sizes) and sizes == sorted(sizes) and sizes[-1] >= 4 * 10**7


def test_argument_checks_before_device(pkg):
    lib = pkg._native.lib()
    ref = np.random.default_rng(1).integers(0, 4, 2000).astype(np.uint8)
    h = C.c_void_p(0)
    assert lib.genie_index_create(ref.ctypes.data_as(C.POINTER(C.c_uint8)), ref.size, 8, 0, C.byref(h)) == 0
    try:
        buf = np.zeros(1 << 16, np.uint8)
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

        table_checks(lambda ix=h, tab=p, nc=3: lib.genie_contigs_validate(ix, tab, nc, None))

        for fl in FLAGS:
            bytes_ok = lib.genie_find_mems_contigs_workspace_bytes(2, 100, 100, fl, 3)
            assert 0 < bytes_ok <= (1 << 16) - 256

            def mems(ix=h, tab=p, nc=3, flags=fl, bases=p, offs=p, n=2, total=100, max_len=100, m=5, occ=0, out=p, rows=p, cap=10,
                     st=p, tt=p, wsp=p, wsb=bytes_ok):
                return lib.genie_find_mems_contigs(ix, tab, nc, flags, bases, offs, n, total, max_len, m, occ, out, rows, cap, st, tt,
                                                   wsp, wsb, None)

            table_checks(mems)
            for bad in (dict(out=None), dict(offs=None), dict(bases=None), dict(n=-1), dict(total=-1), dict(max_len=-1),
                        dict(max_len=2**31), dict(cap=-1), dict(wsb=-1), dict(m=0), dict(occ=-1), dict(flags=fl | 4), dict(flags=-1),
                        dict(rows=odd16), dict(out=odd8), dict(tt=odd8), dict(st=odd4)):
                assert mems(**bad) == INVALID, bad
            assert mems(wsp=None) == CAPACITY and mems(wsp=C.c_void_p(al + 16)) == CAPACITY and mems(wsb=bytes_ok - 1) == CAPACITY
            assert mems(tab=None, wsp=None) == INVALID              # a bad argument is reported before a capacity
            assert mems(nc=2**31 - 1, wsp=None) == TOO_LONG         # ... the table's too; its own checks come behind the others
            assert mems(nc=2**31 - 1, st=odd4) == INVALID and mems(nc=2**31 - 1, wsb=-1) == INVALID
            assert mems(n=0, offs=None, wsp=None, wsb=0) == INVALID     # the offsets hold N + 1 entries: one at least
            assert mems(rows=None) == NO_DEVICE and mems(st=None, tt=None, rows=None, cap=0) == NO_DEVICE
            assert mems(n=0, wsp=None, wsb=0, total=0, bases=None) == NO_DEVICE

        tmp_ok = lib.genie_locate_contigs_tmp_bytes(7)

        def loc(ix=h, tab=p, nc=3, rows=p, S=7, ho=p, hits=p, cap=10, tt=p, tmp=p, tb=tmp_ok):
            return lib.genie_locate_contigs(ix, tab, nc, rows, S, ho, hits, cap, tt, tmp, tb, None)

        table_checks(loc)
        for bad in (dict(S=-1), dict(cap=-1), dict(tb=-1), dict(ho=None), dict(rows=None), dict(rows=odd16), dict(hits=odd8),
                    dict(ho=odd8), dict(tt=odd8)):
            assert loc(**bad) == INVALID, bad
        assert loc(tmp=None) == CAPACITY and loc(tmp=C.c_void_p(al + 16)) == CAPACITY and loc(tb=tmp_ok - 1) == CAPACITY
        assert loc(hits=None, cap=0) == NO_DEVICE and loc(tt=None) == NO_DEVICE and loc(S=0, rows=None, tmp=None, tb=0) == NO_DEVICE

        def crd(ix=h, tab=p, nc=3, pos=p, stride=1, count=9, out=p):
            return lib.genie_contig_coords(ix, tab, nc, pos, stride, count, out, None)

        table_checks(crd)
        for bad in (dict(count=-1), dict(stride=0), dict(stride=-4), dict(pos=None), dict(out=None), dict(pos=odd4), dict(out=odd4)):
            assert crd(**bad) == INVALID, bad
        assert crd(stride=4) == NO_DEVICE and crd(count=0, pos=None, out=None) == NO_DEVICE and crd(out=odd8) == NO_DEVICE
    finally:
        lib.genie_index_destroy(h)


def test_python_layer_refuses_a_host_only_handle(pkg):
    rs = pkg.ReferenceSet.from_sequences(["ACGTACGTTGCA" * 30, "", "GGATC" * 50])
    ix = pkg.GenieIndex.build(rs.codes, 8)                         # host-only: no device was touched
    for fn in (ix.find_mems_contigs, ix.locate_contigs, ix.contig_coords, pkg.SMEM.find_mems_contigs, pkg.SMEM.locate_contigs):
        assert callable(fn)
    with pytest.raises(Exception):
        ix.find_mems_contigs(rs, np.zeros(10, np.uint8), np.asarray([0, 10], np.int64), 5)
    with pytest.raises(Exception):
        ix.contig_coords(rs, [1, 2, 3])


# ------------------------------------------------------------------ ReferenceSet on the host
def test_reference_set_from_sequences(pkg):
    rs = pkg.ReferenceSet.from_sequences(["ACGT", "", "ggTa", ""], names=["chr1", "gap", "chr2", "end"])
    assert rs.names == ["chr1", "gap", "chr2", "end"] and len(rs) == 4 and rs.n == 8
    assert rs.offsets.dtype == np.int64 and rs.offsets.tolist() == [0, 4, 4, 8, 8]
    assert rs.codes.dtype == np.uint8 and rs.codes.tolist() == [0, 1, 2, 3, 2, 2, 3, 0]
    assert pkg.ReferenceSet.from_sequences(["A", "C"]).names == ["0", "1"]
    assert pkg.ReferenceSet.from_sequences(["", "ACG"]).offsets.tolist() == [0, 0, 3]
    with pytest.raises(ValueError, match="chrN"):
        pkg.ReferenceSet.from_sequences(["ACGT", "ACNT"], names=["chr1", "chrN"])
    with pytest.raises(ValueError):
        pkg.ReferenceSet.from_sequences([])
    with pytest.raises(ValueError):
        pkg.ReferenceSet.from_sequences(["A"], names=["x", "y"])


# ------------------------------------------------------------------ the brute force
def _codes(s):
    return np.asarray(["ACGTN".index(c) if c != "N" else 7 for c in s], np.uint8)


def test_brute_force_on_hand_written_cases():
    # suffix rows of ACGTAC: '' AC ACGTAC C CGTAC GTAC TAC
    ref, off = _codes("ACGTAC"), [0, 3, 3, 6]                       # ACG | | TAC
    for one in (CU.per_contig_one, CU.clipped_one):
        rows = lambda read, m, split=False, occ=0: (lambda r: (r[0].tolist(), r[1], r[2]))(one(ref, off, _codes(read), m, split, occ))      # noqa: E731
        # the read equal to the concatenation: its one MEM is cut in two, the second left-maximal by the contig start alone
        assert rows("ACGTAC", 3) == ([[0, 3, 1, 2], [3, 6, 4, 6]], 0, 0)
        assert MM.expected_one(ref, _codes("ACGTAC"), 3, False)[0].tolist() == [[0, 6, 1, 2]]
        # m = 2: AC occurs at t = 0 (room 3) and t = 4 (room 2)
        assert rows("ACGTAC", 2) == ([[0, 2, 5, 1], [0, 3, 1, 2], [3, 6, 4, 6], [4, 6, 1, 2]], 0, 0)
        # a bridging occurrence with too little room on either side is no row at all
        assert rows("GT", 2) == ([], 0, 0) and MM.expected_one(ref, _codes("GT"), 2, False)[0].tolist() == [[0, 2, 3, 5]]
        assert rows("CGTA", 2) == ([[0, 2, 2, 4], [2, 4, 4, 6]], 0, 0)
        # max_occ counts occurrences in the concatenation: AC twice
        assert rows("ACGTAC", 2, occ=1) == ([[3, 6, 4, 6]], 0, 2)
        # a break on the boundary
        assert rows("ACNTAC", 3, split=True) == ([[3, 6, 4, 6]], 0, 0)
        assert rows("ACNTAC", 3) == ([], MM.READ_BAD_BASE, 0)
    assert CU.contig_of(off, np.arange(6)).tolist() == [0, 0, 0, 2, 2, 2]
    assert CU.coords_expected(off, 6, [0, 1, 3, 4, 6, 7]).tolist() == [[-1, -1], [0, 1], [0, 3], [2, 1], [2, 3], [-1, -1]]
    # locate: CGTA (rows of CGTAC: 4) bridges; AC (rows 1, 2) fits twice; the empty pattern's interval holds the $ row
    ho, hits, dropped = CU.locate_expected(ref, off, [[0, 4, 4, 4], [0, 2, 1, 2], [0, 0, 0, 6], [0, 3, -1, -1], [0, 3, 5, 4]])
    assert ho.tolist() == [0, 0, 2, 8, 8, 8] and dropped == 1
    assert hits.tolist() == [[2, 2], [0, 1]] + [[2, 2], [0, 1], [2, 3], [0, 2], [0, 3], [2, 1]]


@pytest.mark.parametrize("name", CASES)
def test_the_two_restatements_agree(name):
    c = CU.case(name)
    for flags in FLAGS:
        for occ in (0, 3):
            a = CU.expected(c.ref, c.off, c.reads, flags, c.m, occ, CU.per_contig_one)
            b = CU.expected(c.ref, c.off, c.reads, flags, c.m, occ, CU.clipped_one)
            assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3], (name, flags, occ)
            rows = a[1]
            assert (rows[:, 1] - rows[:, 0] >= c.m).all()
            t = rows[:, 2].astype(np.int64) - 1
            assert (rows[:, 1] - rows[:, 0] <= c.off[CU.contig_of(c.off, t) + 1] - t).all()      # inside one contig
    if c.n_contigs == 1:
        want = MM.expected(c.ref, c.reads, BOTH | SPLIT, c.m)
        assert all(np.array_equal(x, y) for x, y in zip(a[:3], want[:3]))


@pytest.mark.parametrize("name", [n for n in CASES if n != "table1"])
def test_the_cases_are_not_vacuous(name):
    """Against mems_util.expected of the concatenation the rows differ in both directions: a bridging row disappears, and a
    row appears that is left-maximal only because its contig starts there."""
    c = CU.case(name)
    with_t = set(map(tuple, CU.expected(c.ref, c.off, c.reads, 0, c.m)[1][:, :3].tolist()))
    plain = MM.expected(c.ref, c.reads, 0, c.m)[1]
    t = plain[:, 2].astype(np.int64) - 1
    bridging = plain[:, 1] - plain[:, 0] > c.off[CU.contig_of(c.off, t) + 1] - t
    assert bridging.any() and not any(tuple(r) in with_t for r in plain[bridging, :3].tolist())
    offs, rows, _, _ = CU.expected(c.ref, c.off, c.reads, 0, c.m)
    starts = set(np.unique(c.off).tolist())
    new = 0
    for q, read in enumerate(c.reads):
        for p, e, pos, r in rows[offs[q]:offs[q + 1]].tolist():
            if p > 0 and pos - 1 in starts and pos > 1 and read[p - 1] == c.ref[pos - 2]:
                new += 1
    assert new > 0
    if name.startswith("wave"):                                     # seeds of more than 32 rows; rows with room < m among them
        sa = U.suffix_rows(c.ref)
        at = 35 - c.m // 2                                        # an occurrence of this seed crosses the cut at 35
        lo, hi = U.interval(c.ref, sa, c.reads[0][at:at + c.m])
        assert hi - lo + 1 > 32
        room = c.off[CU.contig_of(c.off, sa[lo:hi + 1]) + 1] - sa[lo:hi + 1]
        short = np.flatnonzero(room < c.m)
        assert short.size and 0 < short[0] and short[-1] < hi - lo and (room >= c.m).sum() > 32
