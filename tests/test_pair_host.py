"""CPU-only tests of genie_pair_alignments (the alignments of paired-end reads, with SAM's per-record fields): the brute force
of tests/pair_util.py on hand-written cases pinned with literal rows, the mapq formula at its ends, the symbols and the header's
wording, the C ABI's argument checks in their documented order (before the device check, so a host-only handle reaches them),
the workspace function's figures and formula, sam_lines / sam_header, and text_reads.interleave_reads on CPU tensors."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pair_util as PU

INVALID, NO_DEVICE, CAPACITY, TOO_LONG = PU.INVALID, PU.NO_DEVICE, PU.CAPACITY, PU.TOO_LONG
D = PU.DEFAULTS


@pytest.fixture(scope="module")
def pkg():
    import genie_smem_amd as g
    g._native.build()
    return g


# ------------------------------------------------------------------ hand-written cases: (kind, parent, strand, contig, offset, r_span, score, mapq)
def H(strand, contig, offset, r_span, score, mapq):
    return (0, 0, strand, contig, offset, r_span, score, mapq)


def S(parent, strand, contig, offset, r_span, score):
    return (2, parent, strand, contig, offset, r_span, score, 0)


def X(strand, contig, offset, r_span, score, mapq):
    return (1, 0, strand, contig, offset, r_span, score, mapq)


def _run(reads, p):
    e = PU.expected(PU.make_batch(reads), p)
    return e["pairs"].tolist(), e["sam"].tolist(), e["totals"].tolist(), e["mapq"].tolist()


FR_PAIR = [[H(0, 0, 101, 100, 90, 60)], [H(1, 0, 301, 100, 80, 50)]]        # [100, 200) forward, [300, 400) reverse
RF_PAIR = [[H(0, 0, 301, 100, 90, 60)], [H(1, 0, 101, 100, 80, 50)]]
SAME_PAIR = [[H(1, 0, 101, 100, 90, 60)], [H(1, 0, 301, 100, 80, 50)]]


@pytest.mark.parametrize("mask", range(1, 8))
def test_orientation_masks(mask):
    # 90 + 80 with no penalty at the mean; U = 170 - 17; pair_mapq = 60 * 17 // 170 = 6, below both records' own
    for reads, typ, flags, signs in ((FR_PAIR, 0, (99, 147), (300, -300)), (RF_PAIR, 1, (99, 147), (-300, 300)),
                                     (SAME_PAIR, 2, (115, 179), (300, -300))):
        proper = (mask >> typ) & 1
        pairs, sam, totals, mapq = _run(reads, D._replace(orient=mask))
        assert pairs == [[0, 1, 6 + proper, 170 * proper, 0, 300, proper, typ]]
        assert sam == [[flags[0] - 2 * (1 - proper), 60, 1, signs[0]], [flags[1] - 2 * (1 - proper), 50, 0, signs[1]]]
        assert totals == [1, proper, 0, 0] and mapq == [6 * proper]


def test_span_at_the_ends_of_the_insert_range():
    yes = ([[0, 1, 7, 170, 0, 300, 1, 0]], [[99, 60, 1, 300], [147, 50, 0, -300]], [1, 1, 0, 0], [6])
    no = ([[0, 1, 6, 0, 0, 300, 0, 0]], [[97, 60, 1, 300], [145, 50, 0, -300]], [1, 0, 0, 0], [0])
    assert _run(FR_PAIR, D._replace(isize_min=300)) == yes and _run(FR_PAIR, D._replace(isize_min=301)) == no
    assert _run(FR_PAIR, D._replace(isize_max=300)) == yes and _run(FR_PAIR, D._replace(isize_max=299)) == no


def test_containment_and_two_contigs():
    # [200, 300) reverse strictly inside [100, 400) forward: neither FR nor RF, under every mask
    inside = [[H(0, 0, 101, 300, 90, 60)], [H(1, 0, 201, 100, 80, 50)]]
    assert _run(inside, D._replace(orient=7)) == ([[0, 1, 6, 0, 0, 300, 0, 3]], [[97, 60, 1, 300], [145, 50, 0, -300]], [1, 0, 0, 0], [0])
    apart = [[H(0, 0, 101, 100, 90, 60)], [H(1, 1, 301, 100, 80, 50)]]
    assert _run(apart, D._replace(orient=7)) == ([[0, 1, 6, 0, 0, 0, 0, -1]], [[97, 60, 1, 0], [145, 50, 0, 0]], [1, 0, 0, 0], [0])


def test_the_pair_against_the_unpaired_alternative():
    # span 844: |844 - 300| * 8 // 256 = 17 = pen_max = pen_unpaired: W1 == U is proper, with pair_mapq 0
    far = [[H(0, 0, 101, 100, 90, 60)], [H(1, 0, 845, 100, 80, 50)]]
    assert _run(far, D._replace(pen_max=17)) == ([[0, 1, 7, 153, 0, 844, 1, 0]], [[99, 60, 1, 844], [147, 50, 0, -844]], [1, 1, 0, 0], [0])
    # span 876: the penalty is 18, W1 = 152 < U = 153: not proper, both heads kept, the score still reported
    farther = [[H(0, 0, 101, 100, 90, 60)], [H(1, 0, 877, 100, 80, 50)]]
    assert _run(farther, D._replace(pen_max=18)) == ([[0, 1, 6, 152, 0, 876, 1, 0]], [[97, 60, 1, 876], [145, 50, 0, -876]], [1, 0, 0, 0], [0])
    # W1 = 5 + 5 - 16 <= 0 with an unpaired alternative far below: proper, pair_mapq 0
    weak = [[H(0, 0, 101, 100, 5, 60)], [H(1, 0, 877, 100, 5, 50)]]
    assert _run(weak, D._replace(pen_unpaired=1 << 20)) == ([[0, 1, 7, -6, 0, 876, 1, 0]], [[99, 60, 1, 876], [147, 50, 0, -876]], [1, 1, 0, 0], [0])


def test_candidates_and_a_displaced_head():
    # the secondary (record 2) belongs to the supplementary record 1, not to the head: no candidate, although it alone is concordant
    reads = [[H(0, 1, 5001, 100, 90, 0), X(0, 0, 2001, 60, 40, 30), S(1, 0, 0, 101, 100, 90)], [H(1, 0, 301, 100, 80, 50)]]
    assert _run(reads, D) == ([[0, 3, 6, 0, 0, 0, 0, -1]], [[97, 0, 3, 0], [2145, 30, 3, -1760], [353, 0, 3, 300], [145, 50, 0, 0]],
                              [1, 0, 0, 0], [0])
    # the head's own secondary next to the mate displaces it: the head gets 0x100 and mapq 0, the secondary the pair's mapq
    reads = [[H(0, 0, 5001, 100, 90, 0), S(0, 0, 0, 101, 100, 90)], [H(1, 0, 301, 100, 80, 50)]]
    assert _run(reads, D) == ([[1, 2, 15, 170, 0, 300, 1, 0]], [[355, 0, 2, -4800], [99, 6, 2, 300], [147, 50, 1, -300]], [1, 1, 1, 0], [6])
    # without class rows no secondary is a candidate: the heads, 4800 apart, reverse before forward
    e = PU.expected(PU.make_batch(reads), D, cap=0)
    assert e["pairs"].tolist() == [[0, 2, 6, 0, 0, 4800, 0, 1]] and e["sam"][:, 0].tolist() == [97, 353, 145]


def test_tlen_sign_at_equal_begin():
    reads = [[H(0, 0, 101, 100, 90, 60)], [H(1, 0, 101, 150, 80, 50)]]      # FR holds with f.b == r.b; 150 * 8 // 256 = 4
    assert _run(reads, D) == ([[0, 1, 7, 166, 0, 150, 1, 0]], [[99, 60, 1, 150], [147, 50, 0, -150]], [1, 1, 0, 0], [4])
    reads = [[H(0, 0, 101, 100, 90, 60)], [H(0, 0, 101, 150, 80, 50)]]
    assert _run(reads, D._replace(orient=4)) == ([[0, 1, 7, 166, 0, 150, 1, 2]], [[67, 60, 1, 150], [131, 50, 0, -150]], [1, 1, 0, 0], [4])


def test_unmapped_mates():
    reads = [[], [H(1, 0, 301, 100, 80, 50), X(0, 1, 40, 30, 20, 7)], [H(0, 0, 101, 100, 90, 60)], []]
    assert _run(reads, D) == ([[-1, 0, 4, 0, 0, 0, 0, -1], [2, -1, 2, 0, 0, 0, 0, -1]],
                              [[153, 50, -1, 0], [2185, 7, -1, 0], [73, 60, -1, 0]], [0, 0, 0, 2], [0, 0])
    assert _run([[], []], D) == ([[-1, -1, 0, 0, 0, 0, 0, -1]], [], [0, 0, 0, 0], [0])


def test_best_of_several_and_ties():
    # two secondaries of mate 0 tie at the same place: the smaller record index wins, W2 == W1, pair_mapq 0
    reads = [[H(0, 0, 5001, 100, 90, 0), S(0, 0, 0, 101, 100, 90), S(0, 0, 0, 101, 100, 90)], [H(1, 0, 301, 100, 80, 50)]]
    pairs, sam, totals, mapq = _run(reads, D)
    assert pairs == [[1, 3, 15, 170, 170, 300, 2, 0]] and mapq == [0] and [row[1] for row in sam] == [0, 0, 0, 50]
    # a better second combination sets W2, not U: 60 * (170 - 160) // 170 = 3
    reads = [[H(0, 0, 5001, 100, 90, 0), S(0, 0, 0, 101, 100, 90), S(0, 0, 0, 101, 100, 80)], [H(1, 0, 301, 100, 80, 50)]]
    pairs, sam, totals, mapq = _run(reads, D)
    assert pairs == [[1, 3, 15, 170, 160, 300, 2, 0]] and mapq == [3]


def test_mapq_formula_at_its_ends():
    assert PU.pair_mapq(0, 0, -5) == 0 and PU.pair_mapq(-3, 0, -30) == 0
    assert PU.pair_mapq(100, 0, -1) == 60 and PU.pair_mapq(100, -7, -1) == 60      # nothing above zero to compare with
    assert PU.pair_mapq(100, 100, 0) == 0 and PU.pair_mapq(100, 0, 100) == 0 and PU.pair_mapq(100, 250, 0) == 0
    assert PU.pair_mapq(100, 50, 20) == 30 and PU.pair_mapq(100, 20, 50) == 30 and PU.pair_mapq(7, 0, 6) == 8
    assert PU.record_mapq(0, True, 60, 40) == 40 and PU.record_mapq(0, True, 30, 40) == 30 and PU.record_mapq(50, True, 60, 40) == 60
    assert PU.record_mapq(50, True, 10, 40) == 50 and PU.record_mapq(20, True, 60, 0) == 20 and PU.record_mapq(20, False, 60, 40) == 20
    assert PU.record_mapq(60, True, 60, 60) == 60 and PU.record_mapq(0, True, 60, 60) == 60


# ------------------------------------------------------------------ the C layer
def test_pair_alignments_symbols_exported(pkg):
    lib = pkg._native.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "genie_smem.h")).read()
    for name, nargs, res in (("genie_pair_alignments", 21, C.c_int), ("genie_pair_alignments_workspace_bytes", 2, C.c_int64)):
        assert name in pkg._native.SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is res and len(fn.argtypes) == nargs
        assert name + "(" in header
    assert lib.genie_abi_version() == 2 and pkg._native.ABI_VERSION == 2      # an addition: the version stays
    for words in ("(rec0, rec1, flags, pair_score, sub_score, isize, n_concordant, type)", "(flag, mapq, mate_record, tlen)",
                  "W = w_x + w_y - min(pen_max, floor(|span - isize_mean| pen_slope / 256))", "Equality is proper",
                  "floor(60 (W1 - min(max(W2, U, 0), W1)) / W1)", "max(q, min(pair_mapq, q + mapq_boost))", "48 bytes per\n * pair",
                  "8 per 1024\n * pairs", "No atomic decides a value", "a POLICY, expressed through eight scalars"):
        assert words in header, words
    consts = dict(re.findall(r"#define (GENIE_PAIR_[A-Z_]+) (\d+)", header))
    assert int(consts["GENIE_PAIR_LANE_MAX"]) == pkg._native.PAIR_LANE_MAX == PU.LANE_MAX
    assert int(consts["GENIE_PAIR_TILE"]) == pkg._native.PAIR_TILE == PU.TILE


def test_pair_alignments_workspace_bytes(pkg):
    ws = pkg._native.lib().genie_pair_alignments_workspace_bytes
    assert ws(-2, 1) == INVALID and ws(2, -1) == INVALID
    for k, vals in enumerate(([0, 2, 126, 2048, 2050, 10**6, 10**8], [0, 1, 63, 65, 10**4, 10**8])):
        seen = []
        for v in vals:
            args = [6, 9]
            args[k] = v
            seen.append(ws(*args))
            assert seen[-1] > 0 and seen[-1] % 256 == 0
        assert all(a <= b for a, b in zip(seen, seen[1:])), (k, seen)
    big = 10**8
    per_pair = (ws(4 * big, 7) - ws(2 * big, 7)) / big
    want = PU.PAIR_BYTES + PU.PAIR_SCAN_BYTES_PER_1024 / 1024
    assert want <= per_pair < want + 1e-4, per_pair
    assert ws(8, 0) == ws(8, 10**9)                                  # nothing per record
    up = lambda v: (v + 255) & ~255      # noqa: E731
    for n in (0, 2, 6, 2000, 2050, 100002):                          # every piece is rounded up to 256 on its own
        p = n // 2
        scan = ((p + 1023) // 1024 + 2) * 8 + 16
        assert ws(n, 77) == 256 + 2 * up(4 * p) + 2 * up(16 * p) + up(8 * (p + 1)) + up(scan), n


def test_pair_alignments_argument_checks_before_device(pkg):
    lib = pkg._native.lib()
    ref = np.random.default_rng(1).integers(0, 4, 2000).astype(np.uint8)
    h = C.c_void_p(0)
    assert lib.genie_index_create(ref.ctypes.data_as(C.POINTER(C.c_uint8)), ref.size, 8, 0, C.byref(h)) == 0
    try:
        buf = np.zeros(1 << 16, np.uint8)
        al = (buf.ctypes.data + 255) & ~255
        p = C.c_void_p(al)
        at = lambda k: C.c_void_p(al + k)      # noqa: E731
        bytes_ok = lib.genie_pair_alignments_workspace_bytes(4, 10)
        assert 0 < bytes_ok <= (1 << 16) - 256

        def call(ix=h, N=4, so=p, rec=p, nrec=10, kl=p, cap=9, orient=1, lo=0, hi=1000, mean=300, slope=8, pmax=16, unp=17, boost=40,
                 pairs=p, sam=p, tt=p, wsp=p, wsb=bytes_ok):
            return lib.genie_pair_alignments(ix, N, so, rec, nrec, kl, cap, orient, lo, hi, mean, slope, pmax, unp, boost, pairs, sam, tt,
                                             wsp, wsb, None)

        assert call(ix=None) == INVALID and call(so=None) == INVALID and call(pairs=None) == INVALID
        assert call(N=3) == INVALID and call(N=-2) == INVALID and call(N=1) == INVALID
        for name in ("nrec", "cap", "wsb"):
            assert call(**{name: -1}) == INVALID, name
        assert call(rec=None) == INVALID and call(sam=None) == INVALID and call(kl=None) == INVALID
        for bad in (dict(orient=0), dict(orient=8), dict(orient=-1), dict(lo=-1), dict(hi=-1), dict(mean=-1), dict(hi=(1 << 30) + 1),
                    dict(mean=(1 << 30) + 1), dict(lo=1001), dict(lo=(1 << 30) + 1, hi=1 << 30), dict(slope=-1), dict(slope=65537),
                    dict(pmax=-1), dict(pmax=(1 << 20) + 1), dict(unp=-1), dict(unp=(1 << 20) + 1), dict(boost=-1), dict(boost=61)):
            assert call(**bad) == INVALID, bad
        for name in ("rec", "kl", "pairs", "sam"):                      # 16-byte aligned
            assert call(**{name: at(8)}) == INVALID, name
        for name in ("so", "tt"):                                       # 8-byte aligned
            assert call(**{name: at(4)}) == INVALID, name
        assert call(N=2**31) == TOO_LONG and call(nrec=2**31) == TOO_LONG
        assert call(N=2**31, wsp=None) == TOO_LONG and call(N=2**31, orient=0) == INVALID and call(N=2**31 + 1) == INVALID
        assert call(wsp=None) == CAPACITY and call(wsp=at(16)) == CAPACITY
        assert call(wsb=bytes_ok - 1) == CAPACITY and call(wsb=0) == CAPACITY and call(N=10**4) == CAPACITY
        assert call(orient=8, wsp=None) == INVALID
        assert call() == NO_DEVICE
        assert call(orient=7, lo=0, hi=0, mean=0, slope=0, pmax=0, unp=0, boost=0) == NO_DEVICE
        assert call(lo=1 << 30, hi=1 << 30, mean=1 << 30, slope=65536, pmax=1 << 20, unp=1 << 20, boost=60) == NO_DEVICE
        assert call(tt=None) == NO_DEVICE and call(nrec=0, rec=None, sam=None) == NO_DEVICE and call(cap=0, kl=None) == NO_DEVICE
        assert call(N=0, wsp=None, wsb=0) == NO_DEVICE
    finally:
        lib.genie_index_destroy(h)


def test_python_layer(pkg):
    ref = np.random.default_rng(2).integers(0, 4, 3000).astype(np.uint8)
    ix = pkg.GenieIndex.build(ref, 8)                               # host-only: no device was touched
    assert callable(ix.pair_alignments) and callable(pkg.SMEM.pair_alignments) and callable(pkg.SMEM.map_pairs)
    assert pkg._native.PAIR_ORIENT == {"fr": 1, "rf": 2, "same": 4, "any": 7}
    with pytest.raises(Exception):
        ix.pair_alignments(np.asarray([0, 0, 0], np.int64), np.zeros((0, 12), np.int32), np.zeros((0, 4), np.int32))


# ------------------------------------------------------------------ text
def test_sam_lines_and_header(pkg):
    ops = lambda *v: [(n << 4) | o for n, o in v]      # noqa: E731
    # pair 0: read 0 on chrA forward with a secondary, read 1 on chrA reverse; pair 1: read 2 on chrB, read 3 without records
    records = np.asarray([[0, 4, 0, 0, 0, 101, 50, 0, 50, 48, 40, 0], [0, 6, 2, 0, 1, 11, 50, 0, 50, 40, 0, 0],
                          [1, 9, 0, 1, 0, 301, 52, 3, 53, 50, 0, 60], [2, 12, 0, 1, 1, 41, 50, 0, 50, 50, 0, 60]], np.int32)
    sam = np.asarray([[99, 6, 2, 252], [355, 0, 2, 0], [147, 60, 0, -252], [89, 60, -1, 0]], np.int32)
    info = np.asarray([[4, 0, 1, 1, 49, 1, 0, 0], [6, 0, 1, 2, 48, 2, 0, 0], [9, 0, 4, 2, 50, 0, 0, 2], [12, 0, 1, 0, 50, 0, 0, 0]], np.int32)
    cigar = np.asarray(ops((50, 7)) + ops((50, 7)) + ops((3, 4), (20, 7), (2, 2), (30, 7)) + ops((50, 7)), np.uint32)
    offs = np.asarray([0, 1, 2, 6, 7], np.int64)
    names = ["p0", "p0", "p1", "p1"]
    lines = pkg.sam_lines(records, sam, info, offs, cigar, names, ["chrA", "chrB"])
    assert lines == ["p0\t99\tchrA\t101\t6\t50=\t=\t301\t252\t*\t*\tNM:i:1\tAS:i:48",
                     "p0\t355\tchrB\t11\t0\t50=\tchrA\t301\t0\t*\t*\tNM:i:2\tAS:i:40",
                     "p0\t147\tchrA\t301\t60\t3S20=2D30=\t=\t101\t-252\t*\t*\tNM:i:2\tAS:i:50",
                     "p1\t89\tchrB\t41\t60\t50=\t*\t0\t0\t*\t*\tNM:i:0\tAS:i:50",
                     "p1\t165\tchrB\t41\t0\t*\t=\t41\t0\t*\t*"]      # unmapped: 0x1 | 0x4 | 0x20 | 0x80, at its mate's place
    seqs, quals = ["ACGTA", "AACCG", "TTTTG", "GGGGA"], ["IIIIH", "ABCDE", "FFFFG", "#####"]
    full = pkg.sam_lines(records, sam, info, offs, cigar, names, ["chrA", "chrB"], seqs, quals)
    assert [ln.split("\t")[9:11] for ln in full] == [["ACGTA", "IIIIH"], ["ACGTA", "IIIIH"], ["CGGTT", "EDCBA"], ["CAAAA", "GFFFF"],
                                                     ["GGGGA", "#####"]]
    none = pkg.sam_lines(records[:0], sam[:0], info[:0], offs[:1], cigar[:0], ["q", "q"], ["chrA"])
    assert none == ["q\t77\t*\t0\t0\t*\t*\t0\t0\t*\t*", "q\t141\t*\t0\t0\t*\t*\t0\t0\t*\t*"]
    with pytest.raises(ValueError):
        pkg.sam_lines(records, sam[:2], info, offs, cigar, names, ["chrA", "chrB"])
    assert pkg.sam_header(["chrA", "chrB"], [500, 600]) == ["@HD\tVN:1.6\tSO:unsorted\tGO:query", "@SQ\tSN:chrA\tLN:500",
                                                            "@SQ\tSN:chrB\tLN:600", "@PG\tID:genie-smem_amd\tPN:genie-smem_amd"]


def test_interleave_reads_on_cpu_tensors(pkg):
    import torch
    rng = np.random.default_rng(3)
    for n in (0, 1, 5, 40):
        batches = []
        for _ in range(2):
            lens = rng.integers(0, 9, n)
            off = np.zeros(n + 1, np.int64)
            off[1:] = np.cumsum(lens)
            batches.append((rng.integers(0, 5, int(off[-1])).astype(np.uint8), off))
        bases, offsets = pkg.text_reads.interleave_reads(*[(torch.from_numpy(b), torch.from_numpy(o)) for b, o in batches])
        assert bases.dtype == torch.uint8 and offsets.dtype == torch.int64 and offsets.numel() == 2 * n + 1 and offsets[0] == 0
        want = [batches[k % 2][0][batches[k % 2][1][k // 2]:batches[k % 2][1][k // 2 + 1]] for k in range(2 * n)]
        for k in range(2 * n):
            assert bases[offsets[k]:offsets[k + 1]].numpy().tolist() == want[k].tolist(), (n, k)
        assert bases.numel() == sum(len(w) for w in want)
    with pytest.raises(ValueError):
        pkg.text_reads.interleave_reads((torch.zeros(0, dtype=torch.uint8), torch.zeros(2, dtype=torch.int64)),
                                        (torch.zeros(0, dtype=torch.uint8), torch.zeros(3, dtype=torch.int64)))
