"""CPU-only tests of the segment calls (genie_reference_segments, genie_segment_coords): the symbols, the scratch size
function, every argument check of the C ABI in its stated order (genie_reference_segments needs no handle: all of its
checks run here, on pointers that are never dereferenced; genie_segment_coords answers GENIE_E_NO_DEVICE on a host-only
handle only after its argument checks), ReferenceSet.from_sequences(..., ambiguous="cut") against tests/segment_util.py, and
a guard against a vacuous end-to-end case."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import contig_util as CU
import segment_util as SU

OK, INVALID, NO_DEVICE, TOO_LONG, CAPACITY = SU.OK, SU.INVALID, SU.NO_DEVICE, SU.TOO_LONG, SU.CAPACITY
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAND = ["ACNNGT", "", "NNN", "nACGTn", "ACGT"]


@pytest.fixture(scope="module")
def pkg():
    import genie_smem_amd as g
    g._native.build()
    return g


def test_segment_symbols_exported(pkg):
    lib = pkg._native.lib()
    header = open(os.path.join(ROOT, "include", "genie_smem.h")).read()
    for name, nargs, res in (("genie_reference_segments_tmp_bytes", 2, C.c_int64), ("genie_reference_segments", 14, C.c_int),
                             ("genie_segment_coords", 11, C.c_int)):
        assert name in pkg._native.SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is res and len(fn.argtypes) == nargs
        assert name + "(" in header
    assert lib.genie_abi_version() == 2 and pkg._native.ABI_VERSION == 2      # additions: the version stays
    assert "#define GENIE_ABI_VERSION 2" in header
    assert "#define GENIE_SEG_POSITIONS 0" in header and "#define GENIE_SEG_HITS 1" in header
    assert (pkg._native.SEG_POSITIONS, pkg._native.SEG_HITS) == (SU.POSITIONS, SU.HITS) == (0, 1)


def test_tmp_size_function(pkg):
    tmp = pkg._native.lib().genie_reference_segments_tmp_bytes
    header = open(os.path.join(ROOT, "include", "genie_smem.h")).read()
    assert tmp(-1, 1) == INVALID and tmp(1, -1) == INVALID and tmp(-5, -5) == INVALID
    ns, rs = [0, 1, 4095, 4096, 4097, 10**5, 10**8, 2**31 + 2**20, 2**36], [0, 1, 2, 700, 10**6, 2**31 - 1]
    grid = np.asarray([[tmp(n, r) for r in rs] for n in ns], np.int64)
    assert (grid > 0).all() and (grid % 256 == 0).all()
    assert (np.diff(grid, axis=0) >= 0).all() and (np.diff(grid, axis=1) >= 0).all()
    # the growth the header states: 32 bytes per 4096 of given reference (up to the rounding of three pieces to 256)
    assert "32 bytes per 4096 of given" in " ".join(header.split())
    for n in (10**8, 2**31 + 2**20):
        rate = (tmp(n + 4096 * 10**4, 1) - tmp(n, 1)) / 10**4
        assert abs(rate - 32) < 0.1, rate


def test_reference_segments_argument_checks(pkg):
    lib = pkg._native.lib()
    buf = np.zeros(1 << 16, np.uint8)
    al = (buf.ctypes.data + 255) & ~255
    p = C.c_void_p(al)
    odd8, odd4 = C.c_void_p(al + 4), C.c_void_p(al + 2)
    out4 = (C.c_int64 * 4)()
    tmp_ok = lib.genie_reference_segments_tmp_bytes(1000, 3)
    assert 0 < tmp_ok <= (1 << 16) - 256

    def seg(codes=p, n=1000, tab=p, nrec=3, bases=p, capb=1000, so=p, sr=p, sg=p, caps=500, out=out4, tmp=p, tb=tmp_ok):
        return lib.genie_reference_segments(codes, n, tab, nrec, bases, capb, so, sr, sg, caps, out, tmp, tb, None)

    nulls = dict(bases=None, so=None, sr=None, sg=None)
    # every bad argument is reported as such, also next to a bad scratch: the argument checks come first
    for bad in (dict(codes=None), dict(out=None), dict(n=-1), dict(tb=-1), dict(capb=-1), dict(caps=-1), dict(nrec=0), dict(nrec=-3),
                dict(tab=None), dict(tab=None, nrec=2), dict(bases=None), dict(so=None), dict(sr=None), dict(sg=None),
                dict(bases=None, so=None), dict(so=None, sr=None, sg=None), dict(tab=odd8), dict(so=odd8), dict(sg=odd8), dict(sr=odd4)):
        assert seg(**bad) == INVALID, bad
        assert seg(tmp=None, **bad) == INVALID, bad
    # then the scratch
    assert seg(tmp=None) == CAPACITY and seg(tmp=C.c_void_p(al + 16)) == CAPACITY and seg(tb=tmp_ok - 1) == CAPACITY
    assert seg(tmp=None, **nulls) == CAPACITY and seg(tb=0, **nulls) == CAPACITY
    # what is allowed reaches the scratch check too: a NULL table with one record, unaligned codes and bases, a null d_codes
    # with nothing given, and capacities that the sizing call does not look at
    assert seg(tab=None, nrec=1, tmp=None) == CAPACITY
    assert seg(codes=C.c_void_p(al + 1), bases=C.c_void_p(al + 3), tmp=None) == CAPACITY
    assert seg(codes=None, n=0, tmp=None) == CAPACITY
    assert seg(capb=-1, caps=-1, tmp=None, **nulls) == CAPACITY
    assert seg(nrec=2**31, tmp=None) == TOO_LONG and seg(nrec=2**31 - 1, tmp=None) == CAPACITY


def test_segment_coords_argument_checks(pkg):
    lib = pkg._native.lib()
    ref = np.random.default_rng(1).integers(0, 4, 2000).astype(np.uint8)
    h = C.c_void_p(0)
    assert lib.genie_index_create(ref.ctypes.data_as(C.POINTER(C.c_uint8)), ref.size, 8, 0, C.byref(h)) == 0
    try:
        buf = np.zeros(1 << 12, np.uint8)
        al = (buf.ctypes.data + 255) & ~255
        p = C.c_void_p(al)
        odd16, odd8, odd4 = C.c_void_p(al + 8), C.c_void_p(al + 4), C.c_void_p(al + 2)

        def crd(ix=h, so=p, sr=p, sg=p, ns=3, form=SU.POSITIONS, inp=p, stride=1, count=9, out=p):
            return lib.genie_segment_coords(ix, so, sr, sg, ns, form, inp, stride, count, out, None)

        for form, least in ((SU.POSITIONS, 1), (SU.HITS, 2)):
            for bad in (dict(ix=None), dict(so=None), dict(sr=None), dict(sg=None), dict(so=odd8), dict(sg=odd8), dict(sr=odd4),
                        dict(ns=0), dict(ns=-1), dict(count=-1), dict(stride=least - 1), dict(stride=-4), dict(inp=None), dict(out=None),
                        dict(inp=odd4), dict(out=odd16), dict(out=odd8)):
                assert crd(form=form, **{"stride": least, **bad}) == INVALID, (form, bad)
            assert crd(form=form, stride=least, ns=2**31 - 1) == TOO_LONG
            # every argument was fine: only now the handle is looked at
            assert crd(form=form, stride=least) == NO_DEVICE and crd(form=form, stride=least, ns=2**31 - 2) == NO_DEVICE
            assert crd(form=form, stride=4) == NO_DEVICE and crd(form=form, stride=least, count=0, inp=None, out=None) == NO_DEVICE
        for form in (-1, 2, 7):
            assert crd(form=form, stride=2) == INVALID
    finally:
        lib.genie_index_destroy(h)


# ------------------------------------------------------------------ the restatements against each other
def _small_cases():
    for n in (0, 1, 17, 300):
        for name, codes in SU.patterns(n).items():
            yield f"{name}{n}", codes, None
    for name, (codes, off) in SU.record_cases().items():
        yield name, codes, off


def test_the_restatements_agree(pkg):
    """cut(), one plain loop over the positions, against the package's host implementation in numpy, the one
    from_sequences(..., ambiguous="cut") uses."""
    from genie_smem_amd.contigs import cut_segments
    cases = list(_small_cases()) + [("random",) + SU.random_case(*SU.RANDOM[0])]
    for name, codes, off in cases:
        want = SU.cut(codes, off)
        mine = cut_segments(codes, [0, len(codes)] if off is None else off)
        for a, b in zip(want[:4], mine):
            assert a.dtype == b.dtype and np.array_equal(a, b), name
        so = want[1]
        assert want[4] == (np.diff(so).max() if len(so) > 1 else 0), name
        assert so[0] == 0 and (np.diff(so) > 0).all() and so[-1] == len(want[0])      # a valid contig table, no empty segment
    assert len(SU.cut(*SU.record_cases()["empties"])[2]) > 100


def test_cut_on_a_hand_written_case():
    codes = np.asarray([0, 1, 4, 4, 2, 3, 9, 9, 9, 7, 0, 1, 2, 3, 7, 0, 1, 2, 3], np.uint8)
    bases, so, sr, sg, longest = SU.cut(codes, [0, 6, 6, 9, 15, 19])
    assert bases.tolist() == [0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 2, 3] and so.tolist() == [0, 2, 4, 8, 12]
    assert sr.tolist() == [0, 0, 3, 4] and sg.tolist() == [0, 4, 1, 0] and longest == 4
    # two records that touch without a break between them: two segments
    assert SU.cut([0, 1, 2, 3])[1].tolist() == [0, 4]
    assert SU.cut([0, 1, 2, 3], [0, 2, 4])[1].tolist() == [0, 2, 4] and SU.cut([0, 1, 2, 3], [0, 2, 2, 4])[2].tolist() == [0, 2]


# ------------------------------------------------------------------ the Python layer on the host
def test_from_sequences_cut(pkg):
    rs = pkg.ReferenceSet.from_sequences(HAND, names=["a", "b", "c", "d", "e"], ambiguous="cut")
    assert isinstance(rs, pkg.SegmentedReferenceSet) and isinstance(rs, pkg.ReferenceSet)
    assert rs.names == ["a", "b", "c", "d", "e"] and len(rs) == 5 and rs.n_segments == 4
    assert rs.record_offsets.tolist() == [0, 6, 6, 9, 15, 19] and rs.n_given == 19 and rs.n == 12
    assert rs.codes.dtype == np.uint8 and rs.codes.tolist() == [0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 2, 3]      # AC GT ACGT ACGT
    assert rs.offsets.dtype == np.int64 and rs.offsets.tolist() == [0, 2, 4, 8, 12]
    assert rs.seg_record.dtype == np.int32 and rs.seg_record.tolist() == [0, 0, 3, 4]
    assert rs.seg_origin.dtype == np.int64 and rs.seg_origin.tolist() == [0, 4, 1, 0]
    assert rs.name_of(rs.seg_record[2]) == "d"
    # the three conditions of a contig table
    assert rs.offsets[0] == 0 and (np.diff(rs.offsets) >= 0).all() and rs.offsets[-1] == rs.n == len(rs.codes)
    for fn in (rs.coords, rs.hit_coords, rs.build_index, pkg.GenieIndex.segment_coords, pkg.reference_segments):
        assert callable(fn)
    with pytest.raises(RuntimeError, match="build_index"):
        rs.coords([1, 2])


def test_iupac_letters_are_breaks(pkg):
    rs = pkg.ReferenceSet.from_sequences(["ACRGTYAKCMGSTWA", "acgt"], ambiguous="cut")
    assert rs.codes.tolist() == [0, 1, 2, 3, 0, 1, 2, 3, 0, 0, 1, 2, 3]
    assert rs.offsets.tolist() == [0, 2, 4, 5, 6, 7, 8, 9, 13] and rs.seg_record.tolist() == [0] * 7 + [1]
    assert rs.seg_origin.tolist() == [0, 3, 6, 8, 10, 12, 14, 0]
    want = SU.cut(np.asarray([{"A": 0, "C": 1, "G": 2, "T": 3}.get(ch, 4) for ch in "ACRGTYAKCMGSTWAACGT"], np.uint8), [0, 15, 19])
    assert np.array_equal(rs.offsets, want[1]) and np.array_equal(rs.seg_record, want[2]) and np.array_equal(rs.seg_origin, want[3])


def test_refusals(pkg):
    for bad in (["NNN", "", "nn"], ["N"], [""]):
        with pytest.raises(ValueError):
            pkg.ReferenceSet.from_sequences(bad, ambiguous="cut")
    # the default still refuses, word for word, and names the record
    for kw in ({}, {"ambiguous": "error"}):
        with pytest.raises(ValueError, match="reference record 'chrN' holds 'N': only A, C, G and T are supported"):
            pkg.ReferenceSet.from_sequences(["ACGT", "ACNT"], names=["chr1", "chrN"], **kw)
    for value in ("keep", "", None, "CUT", 1):
        with pytest.raises(ValueError, match="ambiguous"):
            pkg.ReferenceSet.from_sequences(["ACGT"], ambiguous=value)
        with pytest.raises(ValueError, match="ambiguous"):
            pkg.ReferenceSet.from_fasta(b">a\nACGT\n", ambiguous=value)
    plain = pkg.ReferenceSet.from_sequences(["ACGT", "gg"])
    assert type(plain) is pkg.ReferenceSet and plain.offsets.tolist() == [0, 4, 6]


def test_coords_round_trip_to_the_given_letters(pkg):
    """coords_expected names, for every kept position, the letter that stands there in the given strings."""
    strings = SU.e2e_case()[0]
    for seqs in (HAND, ["ACRGTYAKCMGSTWA", "acgt"], strings):
        rs = pkg.ReferenceSet.from_sequences(seqs, ambiguous="cut")
        pos = np.arange(0, rs.n + 2)
        got = SU.coords_expected(rs.offsets, rs.seg_record, rs.seg_origin, pos)
        assert got[0].tolist() == [-1, -1] and got[-1].tolist() == [-1, -1]
        for p, (rec, o) in zip(pos[1:-1].tolist(), got[1:-1].tolist()):
            assert seqs[rec][o - 1].upper() == "ACGT"[rs.codes[p - 1]]
        hits = [(s, o) for s in range(rs.n_segments) for o in (1, int(rs.offsets[s + 1] - rs.offsets[s]))]
        by_hit = SU.hit_coords_expected(rs.offsets, rs.seg_record, rs.seg_origin, hits)
        by_pos = SU.coords_expected(rs.offsets, rs.seg_record, rs.seg_origin, [int(rs.offsets[s]) + o for s, o in hits])
        assert np.array_equal(by_hit, by_pos) and (by_hit >= 0).all()
        assert SU.hit_coords_expected(rs.offsets, rs.seg_record, rs.seg_origin, [(-1, 1), (rs.n_segments, 1), (0, 0),
                                      (0, int(rs.offsets[1]) + 1)]).tolist() == [[-1, -1]] * 4


def test_the_end_to_end_case_is_not_vacuous(pkg):
    """The reads the GPU test uses give at least one MEM row that ends at, and one that starts behind, every N run."""
    strings, names, text, reads = SU.e2e_case()
    rs = pkg.ReferenceSet.from_sequences(strings, names, ambiguous="cut")
    assert 5000 < rs.n_given < 6500 and rs.n <= 4096 and len(rs) == 3 and len(reads) == 200
    given = "".join(strings).upper()
    runs = [(m.start(), m.end()) for m in re.finditer("N+", given)]
    assert sorted(b - a for a, b in runs) == sorted(SU.E2E_RUNS) and b"\r\n" in text and strings[1].islower()
    offs, rows, status, _ = CU.expected(rs.codes, rs.offsets, reads, CU.BOTH | CU.SPLIT, SU.E2E_M)
    assert (status == 0).all() and rows.shape[0] >= 72             # the 72 reads laid across the runs hold 30 bases in a row: a row each
    at = SU.coords_expected(rs.offsets, rs.seg_record, rs.seg_origin, rows[:, 2])
    first = rs.record_offsets[at[:, 0]] + at[:, 1] - 1              # 0-based in the given concatenation
    last = first + (rows[:, 1] - rows[:, 0])
    for a, b in runs:
        assert (last == a).any() and (first == b).any(), (a, b)
    assert sum(1 for r in reads if (r > 3).any()) >= 72
