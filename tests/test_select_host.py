"""CPU-only tests of genie_select_alignments (primary, supplementary and secondary alignments of every read, with a mapping
quality): the symbols and the header's wording, the workspace function's figures, the C ABI's argument checks in their
documented order (before the device check, so a host-only handle reaches them), the two forms of the brute force of
tests/select_util.py against each other and against the checks that hold whatever the tie-breaks, hand-written cases of the
definition, and paf_lines."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import select_util as SU

INVALID, NO_DEVICE, CAPACITY, TOO_LONG = SU.INVALID, SU.NO_DEVICE, SU.CAPACITY, SU.TOO_LONG
P = SU.Params
D = SU.DEFAULTS


@pytest.fixture(scope="module")
def pkg():
    import genie_smem_amd as g
    g._native.build()
    return g


def test_select_alignments_symbols_exported(pkg):
    lib = pkg._native.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "genie_smem.h")).read()
    for name, nargs, res in (("genie_select_alignments", 26, C.c_int), ("genie_select_alignments_workspace_bytes", 2, C.c_int64)):
        assert name in pkg._native.SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is res and len(fn.argtypes) == nargs
        assert name + "(" in header
    assert lib.genie_abi_version() == 2 and pkg._native.ABI_VERSION == 2      # an addition: the version stays
    for words in ("(kind, parent, order, mapq)", "(read, chain, kind, strand, contig, offset, r_span, q_begin, q_end, score, sub, mapq)",
                  "(candidates, primaries, secondaries, best chain or -1)", "{candidates, primaries, secondaries, selected}",
                  "100 ov > mask_level min(len_i, len_j)", "Equality is no overlap", "100 score >= pri_ratio score(parent)",
                  "Equality is eligible", "[L - q_end, L - q_begin)", "minimap2's shape without the\n * logarithm",
                  "a POLICY, expressed through five scalars", "4 bytes\n * per chain", "64 bytes per read", "8 per 1024 reads",
                  "No atomic decides a value"):
        assert words in header, words
    consts = dict(re.findall(r"#define (GENIE_SELECT_[A-Z_]+) (\d+)", header))
    assert int(consts["GENIE_SELECT_LANE_MAX"]) == pkg._native.SELECT_LANE_MAX == SU.LANE_MAX
    assert int(consts["GENIE_SELECT_TILE"]) == pkg._native.SELECT_TILE == SU.TILE


def test_select_alignments_workspace_bytes(pkg):
    ws = pkg._native.lib().genie_select_alignments_workspace_bytes
    assert ws(-1, 1) == INVALID and ws(1, -1) == INVALID
    for k, vals in enumerate(([0, 1, 63, 1024, 1025, 10**6, 10**8], [0, 1, 63, 65, 10**4, 10**8])):
        seen = []
        for v in vals:
            args = [5, 9]
            args[k] = v
            seen.append(ws(*args))
            assert seen[-1] > 0 and seen[-1] % 256 == 0
        assert all(a <= b for a, b in zip(seen, seen[1:])), (k, seen)
    big = 10**8
    per_chain = (ws(7, 2 * big) - ws(7, big)) / big
    assert SU.CHAIN_BYTES <= per_chain < SU.CHAIN_BYTES + 1e-4, per_chain
    per_read = (ws(2 * big, 7) - ws(big, 7)) / big
    want = SU.READ_BYTES + SU.READ_SCAN_BYTES_PER_1024 / 1024
    assert want <= per_read < want + 1e-4, per_read
    up = lambda v: (v + 255) & ~255      # noqa: E731
    for n, cap in ((0, 0), (1, 0), (3, 100), (1000, 5000), (1025, 1)):      # every piece is rounded up to 256 on its own
        scan = ((n + 1023) // 1024 + 2) * 8 + 16
        assert ws(n, cap) == 256 + up(4 * cap) + 2 * up(4 * n) + 3 * up(16 * n) + up(8 * (n + 1)) + up(scan), (n, cap)


def test_select_alignments_argument_checks_before_device(pkg):
    lib = pkg._native.lib()
    ref = np.random.default_rng(1).integers(0, 4, 2000).astype(np.uint8)
    h = C.c_void_p(0)
    assert lib.genie_index_create(ref.ctypes.data_as(C.POINTER(C.c_uint8)), ref.size, 8, 0, C.byref(h)) == 0
    try:
        buf = np.zeros(1 << 16, np.uint8)
        al = (buf.ctypes.data + 255) & ~255
        p = C.c_void_p(al)
        at = lambda k: C.c_void_p(al + k)      # noqa: E731
        wsf = lib.genie_select_alignments_workspace_bytes
        for tab, nc in ((None, 0), (p, 1), (p, 3)):
            bytes_ok = wsf(2, 10)
            assert 0 < bytes_ok <= (1 << 16) - 256

            def call(ix=h, tab=tab, nc=nc, flags=1, roff=p, N=2, co=p, U=4, ch=p, aln=p, cap=10, mask=50, ratio=80, msec=5, mins=1,
                     full=40, kl=p, so=p, sel=p, rec=p, cap_sel=7, rc=p, tt=p, wsp=p, wsb=bytes_ok):
                return lib.genie_select_alignments(ix, tab, nc, flags, roff, N, co, U, ch, aln, cap, mask, ratio, msec, mins, full, kl, so, sel,
                                                   rec, cap_sel, rc, tt, wsp, wsb, None)

            assert call(ix=None) == INVALID
            for name in ("roff", "co", "so", "ch", "aln", "kl"):
                assert call(**{name: None}) == INVALID, name
            assert call(rec=None) == INVALID                                # d_records may be NULL only together with d_sel
            for name in ("N", "U", "cap", "cap_sel", "wsb"):
                assert call(**{name: -1}) == INVALID, name
            assert call(flags=4) == INVALID and call(flags=7) == INVALID
            assert call(U=2) == INVALID and call(flags=0) == INVALID and call(flags=2) == INVALID      # U != S N
            for bad in (dict(mask=-1), dict(mask=101), dict(ratio=-1), dict(ratio=101), dict(msec=-1), dict(msec=(1 << 20) + 1), dict(mins=0),
                        dict(mins=(1 << 30) + 1), dict(full=0), dict(full=(1 << 20) + 1)):
                assert call(**bad) == INVALID, bad
            for name in ("roff", "co", "so", "sel", "tt"):                  # 8-byte aligned
                assert call(**{name: at(4)}) == INVALID, name
            for name in ("ch", "aln", "kl", "rec", "rc"):                   # 16-byte aligned
                assert call(**{name: at(8)}) == INVALID, name
            assert call(tab=p, nc=0) == INVALID and call(tab=p, nc=-1) == INVALID
            assert call(tab=None, nc=1) == INVALID and call(tab=at(4), nc=2) == INVALID
            assert call(tab=p, nc=2**31 - 1) == TOO_LONG
            assert call(cap=2**31) == TOO_LONG and call(N=2**31, U=2**32) == TOO_LONG
            assert call(cap=2**31, wsp=None) == TOO_LONG and call(cap=2**31, mask=101) == INVALID      # behind a bad argument, before the capacity
            assert call(wsp=None) == CAPACITY and call(wsp=at(16)) == CAPACITY
            assert call(wsb=bytes_ok - 1) == CAPACITY and call(wsb=0) == CAPACITY and call(cap=10**4) == CAPACITY
            assert call(mask=101, wsp=None) == INVALID
            assert call() == NO_DEVICE
            assert call(mask=0, ratio=0, msec=0, mins=1 << 30, full=1 << 20) == NO_DEVICE
            assert call(mask=100, ratio=100, msec=1 << 20) == NO_DEVICE
            assert call(sel=None, rec=None, cap_sel=0, rc=None, tt=None) == NO_DEVICE and call(sel=None) == NO_DEVICE
            assert call(flags=3) == NO_DEVICE and call(flags=0, N=4) == NO_DEVICE and call(flags=2, N=4) == NO_DEVICE
            assert call(cap=0, ch=None, aln=None, kl=None) == NO_DEVICE
            assert call(N=0, U=0, roff=None, wsp=None, wsb=0) == NO_DEVICE
    finally:
        lib.genie_index_destroy(h)


def test_python_layer(pkg):
    ref = np.random.default_rng(2).integers(0, 4, 3000).astype(np.uint8)
    ix = pkg.GenieIndex.build(ref, 8)                               # host-only: no device was touched
    assert callable(ix.select_alignments) and callable(pkg.SMEM.select_alignments) and callable(pkg.SMEM.map_records)
    with pytest.raises(Exception):
        ix.select_alignments(np.asarray([0, 10], np.int64), np.asarray([0, 1], np.int64), np.zeros((1, 8), np.int32),
                             np.asarray([[20, 0, 10, 1, 11, 3, 1, 10]], np.int32))


# ------------------------------------------------------------------ the brute force against itself
def test_the_two_forms_agree_on_random_reads():
    rng = np.random.default_rng(41)
    kinds, n_reads = set(), 0
    sets = (D, P(0, 100, 1, 22, 7), P(100, 0, 1 << 20, 1, 1), P(30, 90, 3, 1, 40))
    for S, counts, prms in ((1, rng.integers(0, 41, 1500), sets[:2]), (2, rng.integers(0, 41, 1500), sets[2:]),
                            (2, rng.integers(0, 6, 1500), sets)):
        b = SU.random_batch(rng, [int(c) for c in counts], S, skipped=0.05)
        for prm in prms:
            one, two = SU.expected(b, prm), SU.expected(b, prm, classify=SU.greedy)
            SU.agrees(two, one)
            SU.check_result(b, prm, one)
            kinds |= set(one["klass"][:, 0].tolist())
        n_reads += len(counts)
    assert kinds == {0, 1, 2, 3} and n_reads >= 4000


# ------------------------------------------------------------------ hand-written cases
def _one_read(L, rows, prm, S=1, second=()):
    b = SU.make_batch([L], [list(rows)] + ([list(second)] if S == 2 else []), S)
    one, two = SU.expected(b, prm), SU.expected(b, prm, classify=SU.greedy)
    SU.agrees(two, one)
    SU.check_result(b, prm, one)
    return one


def _row(score, qb, qe, matched=None, flags=0, rb=100, contig=0):
    return (score, qb, qe, rb, rb + qe - qb, flags, qe - qb if matched is None else matched, contig)


def test_hand_written_cases():
    # mask equality is no overlap: [0, 100) and [50, 150) share 50 of min(100, 100): 100 * 50 > 50 * 100 is false
    res = _one_read(200, [_row(90, 0, 100), _row(80, 50, 150)], D)
    assert res["klass"][:, 0].tolist() == [0, 1] and res["sel"].tolist() == [0, 1]
    res = _one_read(200, [_row(90, 0, 100), _row(80, 49, 149)], D)
    assert res["klass"].tolist() == [[0, 0, 0, 60 * 10 // 90], [2, 0, 1, 0]]
    # the shorter one decides: 30 of 40 bases inside a long one
    assert _one_read(200, [_row(90, 0, 100), _row(80, 70, 110)], D)["klass"][1, 0] == 2
    # pri_ratio equality is eligible: 100 * 72 >= 80 * 90; one less is not
    assert _one_read(200, [_row(90, 0, 100), _row(72, 0, 100)], D)["klass"][1].tolist() == [2, 0, 1, 0]
    res = _one_read(200, [_row(90, 0, 100), _row(71, 0, 100)], D)
    assert res["klass"][1].tolist() == [2, 0, -1, 0] and res["sel"].tolist() == [0] and res["counts"].tolist() == [[2, 1, 1, 0]]
    # a candidate that overlaps two primaries goes to the first in key order, which is the second chain here
    res = _one_read(300, [_row(80, 0, 100), _row(90, 150, 250), _row(50, 40, 210)], P(20, 0, 5, 1, 40))
    assert res["klass"][:, :3].tolist() == [[1, 0, 1], [0, 1, 0], [2, 1, 2]] and res["sel"].tolist() == [1, 0, 2]
    assert res["records"][:, 10].tolist() == [50, 0, 0] and res["counts"].tolist() == [[3, 2, 1, 1]]
    # ties go to the smaller chain index
    assert _one_read(100, [_row(50, 0, 100), _row(50, 0, 100)], D)["klass"][:, 0].tolist() == [0, 2]
    # the mapq formula: sub == score, sub == 0, and matched on both sides of mapq_full
    assert _one_read(100, [_row(50, 0, 100), _row(50, 0, 100)], D)["klass"][0, 3] == 0
    assert _one_read(100, [_row(50, 0, 100)], D)["klass"][0, 3] == 60
    assert _one_read(100, [_row(50, 0, 100, matched=39)], D)["klass"][0, 3] == 60 * 39 // 40 == 58
    assert _one_read(100, [_row(50, 0, 100, matched=40)], D)["klass"][0, 3] == 60
    assert _one_read(100, [_row(50, 0, 100, matched=41)], D)["klass"][0, 3] == 60
    assert _one_read(100, [_row(50, 0, 100, matched=30), _row(20, 10, 90)], D)["klass"][0, 3] == 60 * 30 * 30 // (50 * 40) == 27
    # strand 1 is converted to forward coordinates: [0, 40) of the reverse strand of a read of 100 is [60, 100)
    res = _one_read(100, [_row(50, 60, 100)], D, 2, [_row(45, 0, 40)])
    assert res["klass"][:, 0].tolist() == [0, 2] and res["records"][1, [3, 7, 8]].tolist() == [1, 60, 100]
    assert _one_read(100, [_row(50, 0, 40)], D, 2, [_row(45, 0, 40)])["klass"][:, 0].tolist() == [0, 1]
    # skipped chains and chains below min_score are no candidates; max_secondary cuts the selection, not the classification
    res = _one_read(100, [_row(50, 0, 100), _row(49, 0, 100, flags=4), _row(9, 0, 100), _row(48, 0, 100), _row(47, 0, 100)], P(50, 0, 1, 10, 40))
    assert res["klass"].tolist() == [[0, 0, 0, 60 * 2 // 50], [3, -1, -1, 0], [3, -1, -1, 0], [2, 0, 1, 0], [2, 0, -1, 0]]
    assert res["counts"].tolist() == [[3, 1, 2, 0]] and res["totals"].tolist() == [3, 1, 2, 2]
    # a read without chains, and offsets inside a contig
    b = SU.make_batch([50, 60], [[], [_row(30, 5, 55, rb=1234, contig=1)]], 1)
    res = SU.expected(b, D, table=[0, 1000, 5000])
    assert res["offsets"].tolist() == [0, 0, 1] and res["counts"].tolist() == [[0, 0, 0, -1], [1, 1, 0, 0]]
    assert res["records"].tolist() == [[1, 0, 0, 0, 1, 234, 50, 5, 55, 30, 0, 60]]


def test_paf_lines(pkg):
    ops = lambda *v: [(n << 4) | o for n, o in v]      # noqa: E731
    cigar = np.asarray(ops((3, 4), (20, 7), (1, 8), (5, 7), (2, 2), (40, 7), (4, 4)) + ops((30, 7), (1, 1), (10, 7)), np.uint32)
    offs = np.asarray([0, 7, 10], np.int64)
    records = np.asarray([[1, 7, 0, 1, 2, 101, 68, 4, 70, 55, 20, 37], [1, 9, 2, 0, 0, 11, 40, 10, 51, 30, 0, 0]], np.int32)
    info = np.asarray([[7, 0, 7, 3, 65, 1, 0, 2], [9, 0, 3, 1, 40, 0, 1, 0]], np.int32)
    lines = pkg.paf_lines(records, info, offs, cigar, ["r0", "r1"], [50, 73], ["chrA", "chrB", "chrC"], [500, 600, 700])
    assert lines == ["r1\t73\t4\t70\t-\tchrC\t700\t100\t168\t65\t68\t37\ttp:A:P\tNM:i:3\tcg:Z:20=1X5=2D40=",
                     "r1\t73\t10\t51\t+\tchrA\t500\t10\t50\t40\t41\t0\ttp:A:S\tNM:i:1\tcg:Z:30=1I10="]
    assert pkg.paf_lines(records[:0], info[:0], offs[:1], cigar[:0], [], [], [], []) == []
    with pytest.raises(ValueError):
        pkg.paf_lines(records, info[:1], offs, cigar, ["r0", "r1"], [50, 73], ["chrA", "chrB", "chrC"], [500, 600, 700])
