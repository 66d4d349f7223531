"""CPU-only tests of genie_chain_cigars (the CIGAR of selected chains: the traceback of genie_align_chains): the symbols, the
workspace function and the header's figures, the C ABI's argument checks in their documented order (before the device check, so
a host-only handle reaches them), cigar_strings, and the brute force of tests/cigar_util.py: its two forms against each other
and against the checks that hold whatever the tie-breaks, on random chains, and hand-written cases of the canonical path."""
import ctypes as C
import os

import numpy as np
import pytest

import align_util as AU
import cigar_util as CU

INVALID, NO_DEVICE, CAPACITY, TOO_LONG = AU.INVALID, AU.NO_DEVICE, AU.CAPACITY, AU.TOO_LONG
P = AU.Params
D = AU.DEFAULTS


@pytest.fixture(scope="module")
def pkg():
    import genie_smem_amd as g
    g._native.build()
    return g


def test_chain_cigars_symbols_exported(pkg):
    lib = pkg._native.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "genie_smem.h")).read()
    for name, nargs, res in (("genie_chain_cigars", 38, C.c_int), ("genie_chain_cigars_workspace_bytes", 4, C.c_int64)):
        assert name in pkg._native.SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is res and len(fn.argtypes) == nargs
        assert name + "(" in header
    assert lib.genie_abi_version() == 2 and pkg._native.ABI_VERSION == 2      # an addition: the version stays
    for words in ("(chain, flags, n_ops, nm, n_eq, n_x, ins_bases, del_bases)", "I = 1, D = 2, S = 4, '=' = 7, X = 8",
                  "4 bytes\n * per chain", "20 bytes per selected chain", "8 per 1024 of them", "0 bytes per unit",
                  "stay in F iff F(i, j) == F(i-1, j) - e", "stay in E iff E(i, j) == E(i, j-1) - e",
                  "A = 0 or B = 0 is one 'D' or one\n * 'I' of A + B bases", "A * ceil(D / 64) * 32 bytes"):
        assert words in header, words


def test_chain_cigars_workspace_bytes(pkg):
    ws = pkg._native.lib().genie_chain_cigars_workspace_bytes
    for bad in ((-1, 1, 1, 1), (1, -1, 1, 1), (1, 1, -1, 1), (1, 1, 1, -1)):
        assert ws(*bad) == INVALID
    axes = [[0, 1, 1000, 10**6], [0, 1, 63, 65, 10**4, 10**8], [0, 1, 64, 1025, 10**6, 10**8], [0, 1, 255, 256, 257, 10**9]]
    base = [3, 10, 7, 1000]
    for k, vals in enumerate(axes):
        seen = []
        for v in vals:
            args = list(base)
            args[k] = v
            seen.append(ws(*args))
            assert seen[-1] > 0 and seen[-1] % 256 == 0
        assert all(a <= b for a, b in zip(seen, seen[1:])), (k, seen)
    big = 10**8
    per_chain = (ws(1, 2 * big, 5, 0) - ws(1, big, 5, 0)) / big
    assert CU.CHAIN_BYTES <= per_chain < CU.CHAIN_BYTES + 1e-4, per_chain
    per_sel = (ws(1, 5, 2 * big, 0) - ws(1, 5, big, 0)) / big
    want = CU.SEL_BYTES + CU.SEL_SCAN_BYTES_PER_1024 / 1024
    assert want <= per_sel < want + 1e-4, per_sel
    assert ws(2 * big, 7, 7, 0) - ws(big, 7, 7, 0) == CU.UNIT_BYTES * big
    assert ws(5, 7, 7, 10**9 + 256) - ws(5, 7, 7, 10**9) == 256 and ws(5, 7, 7, 1) - ws(5, 7, 7, 0) == 256


def test_chain_cigars_argument_checks_before_device(pkg):
    lib = pkg._native.lib()
    ref = np.random.default_rng(1).integers(0, 4, 2000).astype(np.uint8)
    h = C.c_void_p(0)
    assert lib.genie_index_create(ref.ctypes.data_as(C.POINTER(C.c_uint8)), ref.size, 8, 0, C.byref(h)) == 0
    try:
        buf = np.zeros(1 << 16, np.uint8)
        al = (buf.ctypes.data + 255) & ~255
        p = C.c_void_p(al)
        at = lambda k: C.c_void_p(al + k)      # noqa: E731
        wsf = lib.genie_chain_cigars_workspace_bytes
        for tab, nc in ((None, 0), (p, 1), (p, 3)):
            bytes_ok = wsf(4, 10, 5, 4096)
            assert 0 < bytes_ok <= (1 << 16) - 256

            def call(ix=h, tab=tab, nc=nc, flags=1, bases=p, roff=p, N=2, total=300, max_len=200, offs=p, rows=p, U=4, R=100, ac=p, ap=p,
                     co=p, ch=p, cap=10, a=1, b=4, o=6, e=1, w=32, indel=64, bonus=5, aln=p, sel=p, n_sel=5, cof=p, cg=p, cap_ops=100,
                     info=p, need=p, tt=p, dirb=4096, wsp=p, wsb=bytes_ok):
                return lib.genie_chain_cigars(ix, tab, nc, flags, bases, roff, N, total, max_len, offs, rows, U, R, ac, ap, co, ch, cap,
                                              a, b, o, e, w, indel, bonus, aln, sel, n_sel, cof, cg, cap_ops, info, need, tt, dirb, wsp, wsb,
                                              None)

            # every check of genie_align_chains, in its order
            assert call(ix=None) == INVALID
            for name in ("bases", "roff", "offs", "rows", "ac", "ap", "co", "ch", "aln"):
                assert call(**{name: None}) == INVALID, name
            for name in ("N", "total", "max_len", "U", "R", "cap", "wsb"):
                assert call(**{name: -1}) == INVALID, name
            assert call(flags=4) == INVALID and call(flags=7) == INVALID
            assert call(U=2) == INVALID and call(flags=0) == INVALID and call(flags=2) == INVALID      # U != S N
            for bad in (dict(a=0), dict(a=65), dict(b=-1), dict(b=65), dict(o=-1), dict(o=65), dict(e=0), dict(e=65), dict(w=-1),
                        dict(w=512), dict(indel=-1), dict(indel=1023 - 64 + 1), dict(w=511, indel=2), dict(bonus=-1), dict(bonus=32769)):
                assert call(**bad) == INVALID, bad
            for name in ("roff", "offs", "co", "tt"):                   # 8-byte aligned
                assert call(**{name: at(4)}) == INVALID, name
            for name in ("rows", "ch", "aln"):                          # 16-byte aligned
                assert call(**{name: at(8)}) == INVALID, name
            assert call(ac=at(2)) == INVALID and call(ap=at(1)) == INVALID
            assert call(tab=p, nc=0) == INVALID and call(tab=p, nc=-1) == INVALID
            assert call(tab=None, nc=1) == INVALID and call(tab=None, nc=-1) == INVALID
            assert call(tab=at(4), nc=2) == INVALID
            assert call(tab=p, nc=2**31 - 1) == TOO_LONG
            # this call's own
            assert call(cap=0, ch=None, aln=None, wsb=1 << 15) == INVALID                     # d_aln whatever cap_chains is
            for name in ("cof", "info"):
                assert call(**{name: None}) == INVALID, name
            for name in ("n_sel", "cap_ops", "dirb"):
                assert call(**{name: -1}) == INVALID, name
            for name in ("sel", "cof", "need"):                         # 8-byte aligned
                assert call(**{name: at(4)}) == INVALID, name
            assert call(info=at(8)) == INVALID and call(cg=at(2)) == INVALID
            assert call(max_len=2**30, total=2**31) == TOO_LONG
            assert call(max_len=2**30, total=2**31, wsp=None) == TOO_LONG      # ... before the capacity
            assert call(n_sel=-1, max_len=2**30, total=2**31) == INVALID       # ... and behind a bad argument
            assert call(wsp=None) == CAPACITY and call(wsp=at(16)) == CAPACITY
            assert call(wsb=bytes_ok - 1) == CAPACITY and call(wsb=0) == CAPACITY
            assert call(n_sel=10**4) == CAPACITY and call(dirb=1 << 20) == CAPACITY
            assert call(sel=None, n_sel=10**6, wsb=wsf(4, 10, 10, 4096)) == NO_DEVICE          # NULL: n_sel is ignored
            assert call(sel=None, wsb=wsf(4, 10, 10, 4096) - 1) == CAPACITY
            assert call(n_sel=-1, wsp=None) == INVALID
            assert call() == NO_DEVICE
            assert call(tt=None, need=None, cg=None, cap_ops=0, dirb=0) == NO_DEVICE
            assert call(cg=at(4)) == NO_DEVICE
            assert call(flags=3) == NO_DEVICE and call(flags=0, N=4) == NO_DEVICE
            assert call(R=0, rows=None, ac=None, ap=None) == NO_DEVICE
            assert call(cap=0, ch=None) == NO_DEVICE
            assert call(N=0, U=0, total=0, max_len=0, bases=None, roff=None, sel=None, wsp=None, wsb=0, cap=0) == NO_DEVICE
            assert call(N=0, U=0, total=0, max_len=0, bases=None, roff=None, wsp=None, wsb=0) == CAPACITY      # a selection needs room
    finally:
        lib.genie_index_destroy(h)


def test_python_layer_refuses_a_host_only_handle_and_cigar_strings(pkg):
    ref = np.random.default_rng(2).integers(0, 4, 3000).astype(np.uint8)
    ix = pkg.GenieIndex.build(ref, 8)                               # host-only: no device was touched
    assert callable(ix.chain_cigars) and callable(pkg.SMEM.chain_cigars) and callable(pkg.SMEM.map_reads)
    none = np.zeros(0, np.int32)
    chains = (np.asarray([0, 1], np.int64), np.asarray([[0, 10, 1, 11, 10, 1, 0, 0]], np.int32), np.zeros(1, np.int32),
              np.full(1, -1, np.int32), none, 0)
    with pytest.raises(Exception):
        ix.chain_cigars((ref[:10], np.asarray([0, 10], np.int64)), np.asarray([0, 1], np.int64), np.asarray([[0, 10, 1, 0]], np.int32),
                        chains, np.asarray([[20, 0, 10, 1, 11, 3, 1, 10]], np.int32))
    ops = lambda *v: [(n << 4) | o for n, o in v]      # noqa: E731
    cigar = np.asarray(ops((3, 4), (20, 7), (1, 8), (5, 7), (2, 2), (40, 7)) + ops((100, 7)) + ops((1, 1), (1, 2), ((1 << 28) - 1, 7)), np.uint32)
    offs = np.asarray([0, 6, 6, 7, 10], np.int64)
    assert pkg.cigar_strings(offs, cigar) == ["3S20=1X5=2D40=", "", "100=", "1I1D268435455="]
    assert pkg.cigar_strings(offs, cigar) == CU.cigar_strings(offs, cigar)
    assert pkg.cigar_strings(np.zeros(1, np.int64), np.zeros(0, np.uint32)) == []
    import torch
    assert pkg.cigar_strings(torch.as_tensor(offs), torch.as_tensor(cigar.view(np.int32)).view(torch.uint32))[0] == "3S20=1X5=2D40="


# ------------------------------------------------------------------ the brute force against itself
def _params(rng):
    return P(int(rng.integers(1, 5)), int(rng.integers(0, 6)), int(rng.choice([0, 1, 3, 6])), int(rng.integers(1, 4)),
             int(rng.choice([0, 1, 2, 5, 40])), 64, int(rng.choice([0, 1, 5, 20])))


def test_the_two_forms_agree_on_random_small_problems():
    rng = np.random.default_rng(31)
    letters = set()
    for _ in range(600):
        p = _params(rng)
        A, B = int(rng.integers(0, 14)), int(rng.integers(0, 14))
        x = rng.integers(0, 4, A)
        y = AU.mutate(rng, np.resize(x, B), 0.2) if A and rng.random() < 0.7 else rng.integers(0, 4, B)
        if A and rng.random() < 0.15:
            x[int(rng.integers(0, A))] = 4
        dlo, dhi = min(0, B - A) - p.band, max(0, B - A) + p.band
        one, two = CU.hef_loops(x, y, dlo, dhi, p), CU.hef_band(x, y, dlo, dhi, p)
        for a, b in zip(one, two):
            assert np.array_equal(a, b)
        assert int(one[0][A, B]) == AU.gap_fill(x, y, p, AU.dp_loops)
        t1, t2 = CU.trace(x, y, dlo, dhi, p, CU.hef_loops), CU.trace(x, y, dlo, dhi, p, CU.hef_band)
        assert t1 == t2 and sum(c in "=XI" for c in t1) == A and sum(c in "=XD" for c in t1) == B
        letters |= set(t1)
    assert letters == set("=XID")


def _random_chain(rng, T, rate):
    n = int(rng.integers(1, 5))
    spec = []
    for _ in range(n):
        A, B = int(rng.integers(0, 9)), int(rng.integers(0, 9))
        if rng.random() < 0.3:
            A, B = (0, B) if rng.random() < 0.5 else (A, 0)
        spec.append((int(rng.integers(3, 15)), A, B))
    left, right = int(rng.integers(0, 25)), int(rng.integers(0, 25))
    span = sum(l + B for l, A, B in spec)
    t0 = int(rng.integers(0, len(T) - span - 30))
    Q, rows = AU.synth_chain(rng, T, t0, spec, left, right, rate)
    free = [q for q in range(len(Q)) if not any(s <= q < e for s, e, _ in rows)]
    if free and rng.random() < 0.4:
        Q[free[int(rng.integers(0, len(free)))]] = 4                # a break, outside the members
    return Q, rows


def test_random_chains_both_forms_and_the_tie_break_free_checks():
    rng = np.random.default_rng(32)
    T = rng.integers(0, 4, 400).astype(np.uint8)
    ops_seen, done = set(), 0
    for k in range(160):
        p = D._replace(band=int(rng.choice([0, 2, 8, 32])), gap_open=int(rng.choice([0, 2, 6])), end_bonus=int(rng.choice([0, 5])))
        Q, rows = _random_chain(rng, T, [0.0, 0.05, 0.1, 0.2][k % 4])
        mem = [(s, e - s, pos - 1) for s, e, pos in rows][::-1]
        clo, chi = (0, len(T)) if k % 3 else (max(0, rows[0][2] - 1 - 6), min(len(T), rows[-1][2] - 1 + (rows[-1][1] - rows[-1][0]) + 6))
        row1, row2 = (AU.align_chain(np.asarray(Q, np.int64), np.asarray(T, np.int64), clo, chi, mem, p, dp)[0] for dp in (AU.dp_loops, AU.dp_band))
        assert row1 == row2
        c1, c2 = (CU.chain_cigar(Q, T, clo, chi, mem, p, row1, hef) for hef in (CU.hef_loops, CU.hef_band))
        assert c1 == c2
        flags, ops, need = c1
        if flags:
            assert flags == CU.SKIPPED and row1[5] == 4
            continue
        CU.check_chain(Q, T, row1, ops, p)
        assert CU.info_row(7, 0, ops)[3] == sum(ln for op, ln in ops if op in (CU.OP_X, CU.OP_I, CU.OP_D))
        ops_seen |= {op for op, _ in ops}
        done += 1
    assert done > 120 and ops_seen == {CU.OP_I, CU.OP_D, CU.OP_S, CU.OP_EQ, CU.OP_X}


# ------------------------------------------------------------------ hand-written cases
def _both(x, y, dlo, dhi, p):
    t = [CU.trace(np.asarray(x), np.asarray(y), dlo, dhi, p, hef) for hef in (CU.hef_loops, CU.hef_band)]
    assert t[0] == t[1]
    return t[0]


def _cigar(Q, T, members, p, clo=0, chi=None):
    """members in read order as (s, e, pos) -> the chain's CIGAR string, checked against its d_aln row."""
    mem = [(s, e - s, pos - 1) for s, e, pos in members][::-1]
    chi = len(T) if chi is None else chi
    row = AU.align_chain(np.asarray(Q, np.int64), np.asarray(T, np.int64), clo, chi, mem, p)[0]
    got = [CU.chain_cigar(Q, T, clo, chi, mem, p, row, hef) for hef in (CU.hef_loops, CU.hef_band)]
    assert got[0] == got[1] and got[0][0] == 0
    CU.check_chain(Q, T, row, got[0][1], p)
    cigar = np.asarray([(ln << 4) | op for op, ln in got[0][1]], np.uint32)
    return CU.cigar_strings([0, len(cigar)], cigar)[0], row


def test_hand_written_cases():
    free = P(1, 4, 0, 1, 1, 64, 5)
    # A = B = 1, x != y, o = 0, w = 1.  H(0, 1) = H(1, 0) = -1 (a gap of one base costs o + e = 1), so E(1, 1) = H(1, 0) - 1 = -2 and
    # F(1, 1) = H(0, 1) - 1 = -2; the diagonal gives 0 - b = -4.  H(1, 1) = -2 is not the diagonal; it equals F(1, 1), so state F: 'I',
    # move to (0, 1); F(1, 1) == F(0, 1) - e does not hold (F(0, 1) is -infinity), so state H at (0, 1), where only E holds: 'D', to
    # (0, 0).  Emitted backwards I then D: forwards the reference base is deleted first, then the query base inserted: 1D1I.
    assert _both([0], [1], -1, 1, free) == "DI"
    assert _both([0], [1], 0, 0, free) == "X" and _both([0], [0], -1, 1, free) == "=" and _both([4], [4], -1, 1, free._replace(mismatch=1)) == "X"
    # with o = 1 the two gaps cost 4, the mismatch 4: the diagonal is taken first
    assert _both([0], [1], -1, 1, free._replace(gap_open=1)) == "X"
    # one-sided gaps are one op, as the closed forms of genie_align_chains have them; A = B = 0 is nothing
    assert _both([], [1, 2, 3], -3, 3, D) == "DDD" and _both([1, 2], [], -2, 2, D) == "II" and _both([], [], 0, 0, D) == ""
    # ... and the program itself gives the same on the border: x against nothing that matches, through the band's edge
    assert _both([0, 0], [1, 1, 1, 0, 0], 0, 3, P(1, 4, 1, 1, 0, 64, 0)) == "DDD=="
    # the order diagonal, F, E: x = AA against y = A with o = 0.  H(1, 0) = -1 and H(1, 1) = 1 (the match).  At (2, 1) the diagonal
    # gives H(1, 0) + a = 0 and F(2, 1) = max(H(1, 1) - 1, F(1, 1) - 1) = 0 as well: the diagonal is taken first, '=' to (1, 0), then
    # 'I'.  Forwards the insertion comes first; F first would have given "=I".
    assert _both([0, 0], [0], -1, 1, free) == "I="
    assert _both([0, 0], [0], -1, 0, free) == "I=" and _both([0, 1], [0], -1, 1, free) == "=I"
    # a run of three inserted bases with o = 0: every step of F ties open against extend (H(i-1, j) == F(i-1, j)) and stays in F
    assert _both([0, 1, 1, 1, 2], [0, 2], -3, 3, free._replace(band=3)) == "=III="
    rng = np.random.default_rng(33)
    T = rng.integers(0, 4, 600).astype(np.uint8)
    sub = lambda v: (v + 1) & 3      # noqa: E731
    # an exact read; a read with clips: the local extension stops where the mismatches begin
    assert _cigar(T[100:150], T, [(0, 50, 101)], D)[0] == "50="
    Qc = np.concatenate([3 - T[90:100], T[100:150], 3 - T[150:158]])
    assert _cigar(Qc, T, [(10, 60, 101)], D)[0] == "10S50=8S"
    # a substitution between two members: a gap of A = B = 1 is the diagonal, and the ops merge across the piece borders
    Qm = np.concatenate([T[100:120], [sub(T[120])], T[121:140]])
    assert _cigar(Qm, T, [(0, 20, 101), (21, 40, 122)], D)[0] == "20=1X19="
    assert _cigar(Qm, T, [(0, 20, 101), (21, 40, 122)], free)[0] == "20=1D1I19="
    # a break of the query is X, in a gap and in an extension
    Qb = Qm.copy()
    Qb[20] = 4
    assert _cigar(Qb, T, [(0, 20, 101), (21, 40, 122)], D)[0] == "20=1X19="
    Qe = np.concatenate([T[100:130], [4], T[131:140]])
    assert _cigar(Qe, T, [(0, 30, 101)], D)[0] == "30=1X9="
    # one-sided gaps: a deletion of 3 reference bases, an insertion of 2 query bases
    Qd = np.concatenate([T[200:230], T[233:260]])
    assert _cigar(Qd, T, [(0, 30, 201), (30, 57, 234)], D)[0] == "30=3D27="
    Qi = np.concatenate([T[200:230], [sub(T[230]), sub(T[230])], T[230:260]])
    got, row = _cigar(Qi, T, [(0, 30, 201), (32, 62, 231)], D)
    assert got == "30=2I30=" and row[0] == 60 - 8 + 10
    # an overlapping member is trimmed, a member that starts where the next one starts is skipped
    Qs = np.concatenate([T[100:130], T[130:150], T[150:170]])
    assert _cigar(Qs, T, [(0, 35, 101), (30, 70, 131)], D)[0] == "70="
    assert _cigar(Qs, T, [(0, 30, 101), (40, 45, 151), (50, 70, 151)], D)[0] == "70="
    # a tie goes to the end: the last base mismatches and G + end_bonus == M; one less and the extension is local
    Qt = np.concatenate([T[400:429], [sub(T[429])]])
    assert _cigar(Qt, T, [(0, 20, 401)], D._replace(end_bonus=4))[0] == "29=1X"
    assert _cigar(Qt, T, [(0, 20, 401)], D._replace(end_bonus=3))[0] == "29=1S"
    # the contig ends 10 bases behind the member: the extension is local and the rest is clipped
    assert _cigar(T[300:370], T, [(0, 20, 301)], D._replace(band=5), 0, 330)[0] == "30=40S"
    # the left extension at the contig's start, on the reversed strings: three bases of the read hang over
    assert _cigar(np.concatenate([[0, 0, 0], T[300:340]]), T, [(13, 43, 311)], D, 300, 600)[0] in ("3S40=", "1S1X1=40=", "3X40=")
    # a chain that genie_align_chains skipped, and end points that are not this chain's
    far = [(0, 20, 101), (30, 50, 131 + 65)]
    mem = [(s, e - s, pos - 1) for s, e, pos in far][::-1]
    Qf = np.resize(T[100:120], 50)
    assert CU.chain_cigar(Qf, T, 0, len(T), mem, D, [0, 0, 0, 0, 0, 4, 0, 0]) == (CU.SKIPPED, [], 0)
    one = [(0, 50, 100)]
    for row in ([60, 0, 51, 101, 151, 3, 1, 50], [60, -1, 50, 101, 151, 3, 1, 50], [60, 0, 50, 100, 151, 3, 1, 50], [60, 0, 50, 101, 152, 3, 1, 50]):
        assert CU.chain_cigar(T[100:150], T, 0, len(T), one, D, row)[0] == CU.BAD
    assert CU.chain_cigar(T[100:150], T, 0, len(T), one, D, [60, 0, 50, 101, 151, 3, 1, 50]) == (0, [(CU.OP_EQ, 50)], 0)
    assert CU.piece_bytes(70, 70, 81) == 70 * 64 and CU.piece_bytes(70, 70, 63) == 70 * 32 and CU.piece_bytes(5, 0, 9) == 0
    assert CU.piece_bytes(300, 600, 1024) == 300 * 512
