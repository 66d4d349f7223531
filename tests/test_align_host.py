"""CPU-only tests of genie_align_chains (every chain aligned on the device: banded gap fill and end extension): the symbols, the
workspace function and the header's figures, the C ABI's argument checks in their documented order (before the device check, so
a host-only handle reaches them), and the brute force of tests/align_util.py: its two forms against each other on random small
problems, the gap fill's behaviour in the band width, and hand-written cases."""
import ctypes as C
import os

import numpy as np
import pytest

import align_util as AU

INVALID, NO_DEVICE, CAPACITY, TOO_LONG = AU.INVALID, AU.NO_DEVICE, AU.CAPACITY, AU.TOO_LONG
P = AU.Params
D = AU.DEFAULTS


@pytest.fixture(scope="module")
def pkg():
    import genie_smem_amd as g
    g._native.build()
    return g


def test_align_chains_symbols_exported(pkg):
    lib = pkg._native.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "genie_smem.h")).read()
    for name, nargs, res in (("genie_align_chains", 30, C.c_int), ("genie_align_chains_workspace_bytes", 2, C.c_int64)):
        assert name in pkg._native.SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is res and len(fn.argtypes) == nargs
        assert name + "(" in header
    assert lib.genie_abi_version() == 2 and pkg._native.ABI_VERSION == 2      # an addition: the version stays
    for words in ("#define GENIE_ALIGN_MAX_DIAGS 1024", "(score, q_begin, q_end, r_begin, r_end, flags, n_used, matched)",
                  "4 bytes\n * per chain", "0 bytes per unit", "E(i, j) = max(H(i, j-1) - o - e, E(i, j-1) - e)",
                  "ov = max(0, s_j + l_j - qs, t_j + l_j - ts)", "G + end_bonus >= M"):
        assert words in header, words


def test_align_chains_workspace_bytes(pkg):
    ws = pkg._native.lib().genie_align_chains_workspace_bytes
    assert ws(-1, 10) == INVALID and ws(1, -1) == INVALID
    us = [0, 1, 2, 1000, 10**6]
    cs = [0, 1, 63, 64, 65, 10**4, 10**6, 10**8]
    grid = [[ws(u, c) for c in cs] for u in us]
    for i in range(len(us)):
        for j in range(len(cs)):
            assert grid[i][j] > 0 and grid[i][j] % 256 == 0
            assert not i or grid[i][j] >= grid[i - 1][j]
            assert not j or grid[i][j] >= grid[i][j - 1]
    big = 10**8
    per_chain = (ws(1, 2 * big) - ws(1, big)) / big
    assert AU.CHAIN_BYTES <= per_chain < AU.CHAIN_BYTES + 1e-4, per_chain
    assert ws(2 * big, 7) - ws(big, 7) == AU.UNIT_BYTES * big
    assert ws(5, 0) == AU.FIXED_BYTES


def test_align_chains_argument_checks_before_device(pkg):
    lib = pkg._native.lib()
    ref = np.random.default_rng(1).integers(0, 4, 2000).astype(np.uint8)
    h = C.c_void_p(0)
    assert lib.genie_index_create(ref.ctypes.data_as(C.POINTER(C.c_uint8)), ref.size, 8, 0, C.byref(h)) == 0
    try:
        buf = np.zeros(1 << 16, np.uint8)
        al = (buf.ctypes.data + 255) & ~255
        p = C.c_void_p(al)
        at = lambda k: C.c_void_p(al + k)      # noqa: E731
        for tab, nc in ((None, 0), (p, 1), (p, 3)):
            bytes_ok = lib.genie_align_chains_workspace_bytes(4, 10)
            assert 0 < bytes_ok <= (1 << 16) - 256

            def call(ix=h, tab=tab, nc=nc, flags=1, bases=p, roff=p, N=2, total=300, max_len=200, offs=p, rows=p, U=4, R=100, ac=p, ap=p,
                     co=p, ch=p, cap=10, a=1, b=4, o=6, e=1, w=32, indel=64, bonus=5, aln=p, tt=p, wsp=p, wsb=bytes_ok):
                return lib.genie_align_chains(ix, tab, nc, flags, bases, roff, N, total, max_len, offs, rows, U, R, ac, ap, co, ch, cap,
                                              a, b, o, e, w, indel, bonus, aln, tt, wsp, wsb, None)

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
            # (2 max_len + max_indel + 2 w + 2) max(a, b, o + e) + 2 end_bonus < 2^30
            assert call(max_len=2**30, total=2**31) == TOO_LONG
            edge = (2**30 - 1 - 10) // 7                                 # o + e = 7 is the largest of the defaults
            assert call(max_len=(edge - 130) // 2, total=2**31) == NO_DEVICE
            assert call(max_len=(edge - 130) // 2 + 1, total=2**31) == TOO_LONG
            assert call(max_len=2**30, total=2**31, wsp=None) == TOO_LONG      # ... before the capacity
            assert call(a=0, max_len=2**30, total=2**31) == INVALID            # ... and behind a bad argument
            assert call(wsp=None) == CAPACITY
            assert call(wsp=at(16)) == CAPACITY
            assert call(wsb=bytes_ok - 1) == CAPACITY and call(wsb=0) == CAPACITY
            assert call(a=0, wsp=None) == INVALID
            assert call() == NO_DEVICE
            assert call(tt=None) == NO_DEVICE
            assert call(flags=3) == NO_DEVICE and call(flags=0, N=4) == NO_DEVICE and call(flags=2, N=4) == NO_DEVICE
            assert call(a=64, b=64, o=64, e=64, w=511, indel=1, bonus=32768) == NO_DEVICE
            assert call(a=1, b=0, o=0, e=1, w=0, indel=1023, bonus=0) == NO_DEVICE
            assert call(R=0, rows=None, ac=None, ap=None) == NO_DEVICE
            assert call(cap=0, ch=None, aln=None, wsb=lib.genie_align_chains_workspace_bytes(4, 0)) == NO_DEVICE
            assert call(N=0, U=0, total=0, max_len=0, bases=None, roff=None, wsp=None, wsb=0) == NO_DEVICE
    finally:
        lib.genie_index_destroy(h)


def test_python_layer_refuses_a_host_only_handle(pkg):
    ref = np.random.default_rng(2).integers(0, 4, 3000).astype(np.uint8)
    ix = pkg.GenieIndex.build(ref, 8)                               # host-only: no device was touched
    assert callable(ix.align_chains) and callable(pkg.SMEM.align_chains) and callable(pkg.SMEM.find_alignments)
    none = np.zeros(0, np.int32)
    chains = (np.asarray([0, 1], np.int64), np.asarray([[0, 10, 1, 11, 10, 1, 0, 0]], np.int32), np.zeros(1, np.int32),
              np.full(1, -1, np.int32), none, 0)
    with pytest.raises(Exception):
        ix.align_chains((ref[:10], np.asarray([0, 10], np.int64)), np.asarray([0, 1], np.int64), np.asarray([[0, 10, 1, 0]], np.int32), chains)


# ------------------------------------------------------------------ the brute force against itself
def _params(rng):
    return P(int(rng.integers(1, 5)), int(rng.integers(0, 6)), int(rng.choice([0, 1, 3, 6])), int(rng.integers(1, 4)),
             int(rng.choice([0, 1, 2, 5, 40])), 64, int(rng.choice([0, 1, 5, 20])))


def _pair(rng, hi=14):
    A, B = int(rng.integers(0, hi)), int(rng.integers(0, hi))
    x = rng.integers(0, 4, A)
    y = AU.mutate(rng, np.resize(x, B), 0.2) if A and rng.random() < 0.7 else rng.integers(0, 4, B)
    if A and rng.random() < 0.15:
        x[int(rng.integers(0, A))] = 4                              # a break of the query
    return x, y


def test_the_two_forms_agree_on_random_small_problems():
    rng = np.random.default_rng(21)
    fills = exts = ties = to_end = local = 0
    for _ in range(1000):
        p = _params(rng)
        x, y = _pair(rng)
        dlo, dhi = min(0, len(y) - len(x)) - p.band, max(0, len(y) - len(x)) + p.band
        assert np.array_equal(AU.dp_loops(x, y, dlo, dhi, p), AU.dp_band(x, y, dlo, dhi, p))
        assert AU.gap_fill(x, y, p, AU.dp_loops) == AU.gap_fill(x, y, p, AU.dp_band)
        fills += 1
    for _ in range(1000):
        p = _params(rng)
        x, y = _pair(rng)
        a, b = AU.extension(x, y, p, AU.dp_loops), AU.extension(x, y, p, AU.dp_band)
        assert a == b
        assert a[0] >= 0 and a[1] <= len(x) and a[2] <= min(len(y), len(x) + p.band)
        exts, ties, to_end, local = exts + 1, ties + a[4], to_end + a[3], local + (not a[3])
    assert fills + exts == 2000 and ties > 100 and to_end > 200 and local > 200, (ties, to_end, local)


def test_gap_fill_is_monotone_in_the_band_and_reaches_the_unbanded_score():
    rng = np.random.default_rng(22)
    grew = 0
    for _ in range(150):
        p = _params(rng)
        x, y = _pair(rng, 12)
        if not len(x) or not len(y):
            continue
        full = int(AU.dp_loops(x, y, -len(x), len(y), p)[len(x), len(y)])      # every diagonal of the rectangle
        seen = [AU.gap_fill(x, y, p._replace(band=w)) for w in range(len(x) + len(y) + 3)]
        assert all(u <= v for u, v in zip(seen, seen[1:]))
        assert all(v == full for v in seen[len(x) + len(y):])
        grew += seen[0] < full
    assert grew > 3


# ------------------------------------------------------------------ hand-written cases
def _row(Q, T, members, p, clo=0, chi=None):
    """members in read order as (s, e, pos)."""
    mem = [(s, e - s, pos - 1) for s, e, pos in members][::-1]
    rows = [AU.align_chain(np.asarray(Q), np.asarray(T), clo, len(T) if chi is None else chi, mem, p, dp)[0]
            for dp in (AU.dp_loops, AU.dp_band)]
    assert rows[0] == rows[1]
    return rows[0]


def test_hand_written_cases():
    rng = np.random.default_rng(23)
    T = rng.integers(0, 4, 600).astype(np.uint8)
    # an exact read: a L + 2 end_bonus, both ends reached
    assert _row(T[100:150], T, [(0, 50, 101)], D) == [50 + 10, 0, 50, 101, 151, 3, 1, 50]
    assert _row(T[100:200], T, [(20, 80, 121)], D) == [100 + 10, 0, 100, 101, 201, 3, 1, 60]
    assert _row(T[100:200], T, [(20, 80, 121)], P(3, 4, 6, 1, 32, 64, 7)) == [300 + 14, 0, 100, 101, 201, 3, 1, 60]
    # three substitutions and one 2-base deletion; the MEMs are the five exact runs between the edits, 198 bases in all: the
    # run in front of the deletion matches three bases past it (the reference repeats there) and is trimmed by them
    T2 = T.copy()
    Dp = 50 + 40 + 1 + 40 + 1 + 37                                   # the first deleted base
    T2[Dp - 1:Dp + 6] = [2, 0, 1, 0, 1, 0, 2]
    sub = lambda v: (v + 1) & 3      # noqa: E731
    Q = np.concatenate([T2[50:90], [sub(T2[90])], T2[91:131], [sub(T2[131])], T2[132:Dp], T2[Dp + 2:Dp + 42], [sub(T2[Dp + 42])],
                        T2[Dp + 43:Dp + 81]])
    q3 = 82 + 37                                                     # where the read goes on behind the deletion
    mems = [(0, 40, 51), (41, 81, 92), (82, q3 + 3, 133), (q3, q3 + 40, Dp + 3), (q3 + 41, q3 + 79, Dp + 44)]
    assert sum(e - s for s, e, _ in mems) == 198 and len(Q) == q3 + 79
    for s, e, pos in mems:
        assert np.array_equal(Q[s:e], T2[pos - 1:pos - 1 + e - s])
    assert _row(Q, T2, mems, D) == [198 - 3 - 12 - 8 + 10, 0, len(Q), 51, Dp + 82, 3, 5, 195]
    # o = 0: a one-base mismatch gap scores -2 e through two gaps when the band has room for them, -b on the diagonal alone
    free = P(1, 4, 0, 1, 1, 64, 5)
    for dp in (AU.dp_loops, AU.dp_band):
        assert AU.gap_fill([0], [1], free, dp) == -2 and AU.gap_fill([0], [1], free._replace(band=0), dp) == -4
        assert AU.gap_fill([0], [1], free._replace(gap_open=1), dp) == -4 and AU.gap_fill([0], [0], free, dp) == 1
    Qm = np.concatenate([T[100:120], [sub(T[120])], T[121:140]])
    assert _row(Qm, T, [(0, 20, 101), (21, 40, 122)], free)[0] == 39 - 2 + 10
    assert _row(Qm, T, [(0, 20, 101), (21, 40, 122)], free._replace(band=0))[0] == 39 - 4 + 10
    # a member that does not lie in front of the one behind it (the same reference position) is skipped: n_used drops
    three = [(0, 30, 101), (40, 45, 151), (50, 70, 151)]
    Qs = np.concatenate([T[100:130], T[130:150], T[150:170]])
    assert _row(Qs, T, three, D)[5:] == [3, 2, 50] and _row(Qs, T, [three[0], three[2]], D) == _row(Qs, T, three, D)[:6] + [2, 50]
    # an overlap in the read alone is trimmed
    assert _row(Qs, T, [(0, 35, 101), (30, 70, 131)], D) == [70 + 10, 0, 70, 101, 171, 3, 2, 70]
    # |B - A| = max_indel + 1: the chain is skipped
    far = [(0, 20, 101), (30, 50, 131 + 65)]
    assert _row(np.resize(T[100:120], 50), T, far, D) == [0, 0, 0, 0, 0, 4, 0, 0]
    assert _row(np.resize(T[100:120], 50), T, far, D._replace(max_indel=65))[5] != 4
    # the contig ends 10 bases behind the member, 50 bases of the read are left: row A has no cell, the extension is local
    cut = _row(T[300:370], T, [(0, 20, 301)], D._replace(band=5), 0, 330)
    assert cut == [20 + 10 + 5, 0, 30, 301, 331, 1, 1, 20]
    assert _row(T[300:370], T, [(0, 20, 301)], D._replace(band=5), 0, 370)[5] == 3
    # a tie goes to the end: the last base mismatches, G + end_bonus == M
    Qt = np.concatenate([T[400:429], [sub(T[429])]])
    assert AU.extension(Qt[20:], T[420:], D._replace(end_bonus=4)) == (9, 10, 10, 1, 1)
    assert AU.extension(Qt[20:], T[420:], D._replace(end_bonus=3))[:4] == (9, 9, 9, 0)
    assert _row(Qt, T, [(0, 20, 401)], D._replace(end_bonus=4)) == [20 + 9 + 4, 0, 30, 401, 431, 3, 1, 20]
    assert _row(Qt, T, [(0, 20, 401)], D._replace(end_bonus=3)) == [20 + 9 + 3, 0, 29, 401, 430, 1, 1, 20]
    # A = 0 gives end_bonus; a break of the query is a mismatch against everything
    assert AU.extension([], T[:5], D)[:4] == (5, 0, 0, 1) and AU.gap_fill([4], [0], D) == -4 and AU.gap_fill([4], [4], D) == -4
