"""CPU-only tests of genie_find_smems_long_ex (both strands and breaks for reads of any length): the symbols, the
workspace function, the C ABI's argument checks (before the device check, so a host-only handle reaches them), and a
numpy restatement of the unit table the kernels build -- per strand-read its segments, their order, start, source range
and direction, found the way the device finds them (starts and ends ranked over the virtual positions) -- checked against
split_util.segments on packing.reverse_complement-ed reads."""
import ctypes as C
import os

import numpy as np
import pytest

import split_util as SU

BOTH, SPLIT = 1, 2


@pytest.fixture(scope="module")
def pkg():
    import genie_smem_amd as g
    g._native.build()
    return g


def test_long_ex_symbols_exported(pkg):
    lib = pkg._native.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "genie_smem.h")).read()
    for name in ("genie_find_smems_long_ex", "genie_find_smems_long_ex_workspace_bytes"):
        assert name in pkg._native.SYMBOLS
        getattr(lib, name)
        assert name + "(" in header
    assert "#define GENIE_READS_BOTH_STRANDS 1" in header and "#define GENIE_READS_SPLIT_BREAKS 2" in header
    assert (pkg._native.READS_BOTH_STRANDS, pkg._native.READS_SPLIT_BREAKS) == (BOTH, SPLIT)
    assert lib.genie_abi_version() == 2


def test_long_ex_workspace_bytes(pkg):
    import test_workspace_sizes_host as W
    lib = pkg._native.lib()
    ws = lib.genie_find_smems_long_ex_workspace_bytes
    for fl in (0, BOTH, SPLIT, BOTH | SPLIT):
        assert ws(-1, 100, 10, fl) < 0
        assert ws(1, -1, 10, fl) < 0
        assert ws(1, 100, -1, fl) < 0
        assert ws(1, 100, 2**31, fl) < 0
    for fl in (4, 8, -1, 1 << 30, BOTH | 4):
        assert ws(1, 100, 10, fl) < 0
    # flags == 0: the long call's own number, on the pinned grid
    for n, want in W.LONG.items():
        for m in W.MAX_LENS:
            assert [ws(n, t, m, 0) for t in W.TOTALS] == want, (n, m)
            assert [ws(n, t, m, 0) for t in W.TOTALS] == [lib.genie_find_smems_long_workspace_bytes(n, t, m) for t in W.TOTALS]
    ns = [0, 1, 2, 1000, 10**6]
    ts = [0, 1, 31, 32, 10**4, 10**6, 10**8]
    for fl in (0, BOTH, SPLIT, BOTH | SPLIT):
        grid = [[ws(n, t, 2**31 - 1, fl) for t in ts] for n in ns]
        for i in range(len(ns)):
            for j in range(len(ts)):
                assert grid[i][j] > 0
                if i:
                    assert grid[i][j] >= grid[i - 1][j], (fl, i, j)
                if j:
                    assert grid[i][j] >= grid[i][j - 1], (fl, i, j)
    for n in ns:
        for t in ts:
            w = {fl: ws(n, t, 2**31 - 1, fl) for fl in (0, BOTH, SPLIT, BOTH | SPLIT)}
            assert w[0] <= w[BOTH] <= w[BOTH | SPLIT] and w[0] <= w[SPLIT] <= w[BOTH | SPLIT], (n, t)
            assert w[BOTH] >= lib.genie_find_smems_long_workspace_bytes(2 * n, 2 * t, 2**31 - 1), (n, t)
    # the stated cost: about 17.3 S bytes per base without breaks, about 20.1 S with them
    assert ws(10, 10**8, 10**8, BOTH) < 2 * 17.5 * 10**8
    assert ws(10, 10**8, 10**8, SPLIT) < 20.5 * 10**8
    assert ws(10, 10**8, 10**8, BOTH | SPLIT) < 2 * 20.5 * 10**8


def test_long_ex_argument_checks_before_device(pkg):
    lib = pkg._native.lib()
    ref = np.random.default_rng(1).integers(0, 4, 2000).astype(np.uint8)
    h = C.c_void_p(0)
    assert lib.genie_index_create(ref.ctypes.data_as(C.POINTER(C.c_uint8)), ref.size, 8, 0, C.byref(h)) == 0
    try:
        ws = np.zeros(1 << 16, np.uint8)
        buf = ws.ctypes.data
        al = (buf + 255) & ~255
        p = C.c_void_p(al)
        for fl in (0, BOTH, SPLIT, BOTH | SPLIT):
            bytes_ok = lib.genie_find_smems_long_ex_workspace_bytes(2, 100, 100, fl)
            assert 0 < bytes_ok <= (1 << 16) - 256

            def call(ix=h, mode=0, flags=fl, bases=p, offs=p, n=2, total=100, max_len=100, out_off=p, rows=p, cap=10, wsp=p,
                     wsb=bytes_ok):
                return lib.genie_find_smems_long_ex(ix, mode, flags, bases, offs, n, total, max_len, 1, out_off, rows, cap, None,
                                                    wsp, wsb, None)

            assert call(ix=None) == -1
            assert call(n=-1) == -1
            assert call(total=-1) == -1
            assert call(max_len=-1) == -1
            assert call(max_len=2**31) == -1
            assert call(cap=-1) == -1
            assert call(out_off=None) == -1
            assert call(offs=None) == -1
            assert call(rows=None) == -1
            assert call(wsp=None) == -1
            assert call(bases=None) == -1
            assert call(mode=3) == -1
            assert call(flags=fl | 4) == -1                         # an unknown flag bit
            assert call(flags=fl | (1 << 20)) == -1
            assert call(flags=-1) == -1
            assert call(rows=C.c_void_p(al + 4)) == -1              # rows must be 16-byte aligned
            assert call(wsp=C.c_void_p(al + 16)) == -1              # workspace 256-byte aligned
            assert call(wsb=bytes_ok - 1) == -10                    # GENIE_E_CAPACITY
            assert call(wsb=-1) == -10                              # this call does not look at the sign: just too small
            assert call(wsp=None, wsb=0) == -1 and call(wsp=C.c_void_p(al + 16), wsb=0) == -1      # ... and a missing or
            assert call(n=0, wsp=C.c_void_p(al + 16)) == -1         # misaligned workspace is a bad argument, reads or none
            assert call(mode=3, wsb=0) == -1 and call(flags=fl | 4, wsb=0) == -1
            if fl & SPLIT:                                          # the split semantics have no LUT / RMI traversal
                assert call(mode=1) == -1 and call(mode=2) == -1
            else:
                assert call(mode=1) == -4
            assert call() == -4                                     # GENIE_E_NO_DEVICE: every argument was fine
            assert call(n=0, offs=None, rows=None, wsp=None, total=0, bases=None) == -4
            assert call(n=0, offs=None, rows=None, wsp=None, total=0, bases=None, wsb=-1) == -4
    finally:
        lib.genie_index_destroy(h)


def test_split_breaks_needs_bwa_before_any_device(pkg):
    ref = np.random.default_rng(2).integers(0, 4, 3000).astype(np.uint8)
    ix = pkg.GenieIndex.build(ref, 8)                               # host-only: no device was touched
    with pytest.raises(ValueError):
        ix.find_smems_long("lut", np.zeros(10, np.uint8), np.asarray([0, 10], np.int64), split_breaks=True)
    with pytest.raises(ValueError):
        ix.find_smems_long("rmi", np.zeros(10, np.uint8), np.asarray([0, 10], np.int64), both_strands=True, split_breaks=True)


# ------------------------------------------------------------------ the unit table, restated in numpy
def unit_table(bases, offs, strands, split, present=0xF, chunk=16384):
    """What the device builds.  Strand-read q = strands * i + s; its virtual positions start at vat[q].  Returns a list of
    units (strand-read, start inside it, length, first source byte in strand order, reversed) in unit order, and the index of
    every strand-read's first unit ([S N + 1]).  With `split` the units are found as the kernels find them: per virtual
    position good / start / end, starts counted per chunk and scanned, begin and end scattered by rank."""
    bases = np.asarray(bases, np.uint8)
    offs = np.asarray(offs, np.int64)
    n = offs.size - 1
    sn = strands * n
    lens = np.repeat(offs[1:] - offs[:-1], strands)
    vat = np.zeros(sn + 1, np.int64)
    vat[1:] = np.cumsum(lens)
    vat += strands * offs[0]

    def src_of(q, p):                                              # (source byte of position p of strand-read q, reversed)
        i, s = divmod(q, strands)
        return (int(offs[i + 1]) - 1 - p, True) if s else (int(offs[i]) + p, False)

    if not split:
        units = [(q, 0, int(lens[q])) + src_of(q, 0) for q in range(sn)]
        return units, np.arange(sn + 1)
    vtot = int(vat[-1] - vat[0])
    v = np.arange(vat[0], vat[-1])
    q = np.searchsorted(vat, v, side="right") - 1                   # the last strand-read that starts at or before v
    q = np.minimum(q, sn - 1) if sn else q
    p = v - vat[q]
    i, s = q // strands, q % strands
    src = np.where(s == 1, offs[i + 1] - 1 - p, offs[i] + p)
    c = bases[src].astype(np.int64)
    code = np.where(c < 4, c ^ np.where(s == 1, 3, 0), 0)
    good = (c < 4) & (((present >> code) & 1) == 1)
    first = p == 0
    last = p == lens[q] - 1
    prev_good = np.concatenate([[False], good[:-1]]) & ~first
    next_good = np.concatenate([good[1:], [False]]) & ~last
    start = good & ~prev_good
    end = good & ~next_good
    # block counts, their exclusive scan, ranks inside a block
    nblk = (int(vat[-1]) + chunk - 1) // chunk
    blk = v // chunk
    bsum = np.zeros(nblk + 1, np.int64)
    np.add.at(bsum, blk[start] + 1, 1)
    bsum = np.cumsum(bsum)
    incl = np.cumsum(start)
    assert vtot == 0 or (bsum[blk] <= incl).all()
    k = incl - 1                                                    # the segment a good position belongs to
    total = int(start.sum())
    assert total == int(end.sum())
    ua = np.full(total, -1, np.int64)
    ub = np.full(total, -1, np.int64)
    ua[k[start]] = v[start]
    ub[k[end]] = v[end] + 1
    assert (ua >= 0).all() and (ub > ua).all()
    units = []
    for a, b in zip(ua.tolist(), ub.tolist()):
        qq = int(np.searchsorted(vat, a, side="right") - 1)
        pp = a - int(vat[qq])
        units.append((qq, pp, b - a) + src_of(qq, pp))
    excl = incl - start
    firstunit = np.full(sn + 1, total, np.int64)
    for qq in range(sn - 1, -1, -1):                                # an empty strand-read takes what follows it
        firstunit[qq] = excl[int(vat[qq] - vat[0])] if lens[qq] > 0 else firstunit[qq + 1]
    return units, firstunit


def _strand_reads(reads, strands):
    from genie_smem_amd import packing
    out = []
    for r in reads:
        out.append(np.asarray(r, np.uint8))
        if strands == 2:
            out.append(packing.reverse_complement(np.asarray(r, np.uint8)) if len(r) else np.zeros(0, np.uint8))
    return out


def _csr(reads, lead=0):
    offs = np.zeros(len(reads) + 1, np.int64)
    offs[1:] = np.cumsum([len(r) for r in reads])
    bases = np.concatenate([np.zeros(lead, np.uint8)] + [np.asarray(r, np.uint8) for r in reads]) if reads else np.zeros(lead, np.uint8)
    return bases, offs + lead


def _reads_with_breaks(seed):
    rng = np.random.default_rng(seed)
    lens = [0, 1, 2, 31, 32, 33, 255, 256, 257, 2047, 2048, 2049, 0, 0, 5000] + [int(x) for x in rng.integers(0, 700, 20)] + [0]
    reads = []
    for j, L in enumerate(lens):
        r = rng.integers(0, 4, L).astype(np.uint8)
        hit = rng.random(L) < (0.0, 0.01, 0.1, 0.5, 1.0)[j % 5]
        r[hit] = rng.integers(4, 256, int(hit.sum())).astype(np.uint8)
        if L > 3 and j % 3 == 0:
            r[0] = 4
            r[-1] = 255
        reads.append(r)
    return reads


@pytest.mark.parametrize("strands", [1, 2])
@pytest.mark.parametrize("present", [0xF, 0x7, 0xE])
@pytest.mark.parametrize("lead", [0, 77])
def test_unit_table_matches_segments_of_strand_reads(pkg, strands, present, lead):
    reads = _reads_with_breaks(5 + strands)
    bases, offs = _csr(reads, lead)
    units, firstunit = unit_table(bases, offs, strands, True, present)
    sreads = _strand_reads(reads, strands)
    want, want_first = [], []
    for q, sr in enumerate(sreads):
        want_first.append(len(want))
        for s, l in SU.segments(sr, present):
            want.append((q, s, l))
    want_first.append(len(want))
    assert [u[:3] for u in units] == want
    assert firstunit.tolist() == want_first
    for q, s, l, src, rev in units:                                 # the source range gives the strand-read's bases back
        got = bases[src - l + 1:src + 1][::-1] ^ 3 if rev else bases[src:src + l]
        assert (got == sreads[q][s:s + l]).all()
        assert rev == (strands == 2 and q % 2 == 1)


@pytest.mark.parametrize("strands", [1, 2])
def test_unit_table_without_breaks_is_the_strand_reads(pkg, strands):
    reads = _reads_with_breaks(9)
    bases, offs = _csr(reads, 13)
    units, firstunit = unit_table(bases, offs, strands, False)
    sreads = _strand_reads(reads, strands)
    assert len(units) == len(sreads) and firstunit.tolist() == list(range(len(sreads) + 1))
    for (q, s, l, src, rev), sr in zip(units, sreads):
        assert (s, l) == (0, len(sr))
        got = bases[src - l + 1:src + 1][::-1] ^ 3 if rev else bases[src:src + l]
        assert (got == sr).all()


def test_two_strands_can_have_different_segment_counts(pkg):
    # a reference without T (present = A, C, G): on the forward strand T breaks, on the reverse strand A does (3 - 0 = T)
    read = np.asarray([0, 1, 2, 0, 3, 1, 1, 0], np.uint8)
    bases, offs = _csr([read])
    units, firstunit = unit_table(bases, offs, 2, True, 0x7)
    assert [u[:3] for u in units if u[0] == 0] == [(0, 0, 4), (0, 5, 3)]
    assert [u[:3] for u in units if u[0] == 1] == [(1, 1, 3), (1, 5, 2)]      # rc = [3, 2, 2, 0, 3, 1, 2, 3]: T breaks
    assert firstunit.tolist() == [0, 2, 4]
