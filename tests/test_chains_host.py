"""CPU-only tests of genie_chain_mems (the MEM rows of every strand-read chained on the device): the symbols, the workspace
function and the header's figures, the C ABI's argument checks (before the device check, so a host-only handle reaches them),
and the brute force of tests/chain_util.py: its two chain extractions against each other on random units, f rising along
every link, and hand-written cases."""
import ctypes as C
import os

import numpy as np
import pytest

import chain_util as CU

INVALID, NO_DEVICE, CAPACITY, TOO_LONG = CU.INVALID, CU.NO_DEVICE, CU.CAPACITY, CU.TOO_LONG
P = CU.Params


@pytest.fixture(scope="module")
def pkg():
    import genie_smem_amd as g
    g._native.build()
    return g


def test_chain_mems_symbols_exported(pkg):
    lib = pkg._native.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "genie_smem.h")).read()
    for name, nargs, res in (("genie_chain_mems", 22, C.c_int), ("genie_chain_mems_workspace_bytes", 3, C.c_int64)):
        assert name in pkg._native.SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is res and len(fn.argtypes) == nargs
        assert name + "(" in header
    assert lib.genie_abi_version() == 2 and pkg._native.ABI_VERSION == 2      # an addition: the version stays
    assert "#define GENIE_ABI_VERSION 2" in header
    for words in ("q_begin, q_end, r_begin, r_end, score,", "24 bytes per row", "28 with more than one", "8 bytes per unit",
                  "gain(j, i) = min(l_i, dq, dr) - ((g * gap_cost) >> 4) >= 1"):
        assert words in header, words


def test_chain_mems_workspace_bytes(pkg):
    ws = pkg._native.lib().genie_chain_mems_workspace_bytes
    assert ws(-1, 10, 0) == INVALID and ws(1, -1, 0) == INVALID and ws(1, 10, -1) == INVALID and ws(1, 10, 2**31 - 1) == INVALID
    us = [0, 1, 2, 3, 1000, 1024, 1025, 10**6]
    rs = [0, 1, 63, 64, 65, 255, 256, 257, 10**4, 10**6, 10**8]
    for nc in (0, 1, 2, 25, 10**4):
        grid = [[ws(u, r, nc) for r in rs] for u in us]
        for i in range(len(us)):
            for j in range(len(rs)):
                assert grid[i][j] > 0 and grid[i][j] % 256 == 0
                assert not i or grid[i][j] >= grid[i - 1][j]
                assert not j or grid[i][j] >= grid[i][j - 1]
    # the header's figures: 24 bytes per row, 28 with more than one contig; 8 per unit and 8 per 1024 units
    big = 10**8
    for nc, per_row in ((0, CU.ROW_BYTES), (1, CU.ROW_BYTES), (2, CU.ROW_BYTES_CONTIGS), (25, CU.ROW_BYTES_CONTIGS)):
        per = (ws(1, 2 * big, nc) - ws(1, big, nc)) / big
        assert per_row <= per < per_row + 1e-4, (nc, per)
    per_unit = (ws(2 * big, 0, 0) - ws(big, 0, 0)) / big
    assert CU.UNIT_BYTES + 8 / 1024 - 1e-4 <= per_unit < CU.UNIT_BYTES + 8 / 1024 + 1e-4, per_unit


def test_chain_mems_argument_checks_before_device(pkg):
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
            bytes_ok = lib.genie_chain_mems_workspace_bytes(2, 100, nc)
            assert 0 < bytes_ok <= (1 << 16) - 256

            def call(ix=h, tab=tab, nc=nc, offs=p, rows=p, U=2, R=100, dist=5000, bw=500, gap=2, pred=5000, score=40, co=p, ch=p, cap=10,
                     ac=p, ap=p, asc=p, tt=p, wsp=p, wsb=bytes_ok):
                return lib.genie_chain_mems(ix, tab, nc, offs, rows, U, R, dist, bw, gap, pred, score, co, ch, cap, ac, ap, asc, tt, wsp,
                                            wsb, None)

            assert call(ix=None) == INVALID
            assert call(offs=None) == INVALID
            assert call(co=None) == INVALID
            assert call(rows=None) == INVALID                       # total_rows > 0
            assert call(U=-1) == INVALID
            assert call(R=-1) == INVALID
            assert call(cap=-1) == INVALID
            assert call(wsb=-1) == INVALID
            for bad in (dict(dist=0), dict(dist=-1), dict(dist=2**22 + 1), dict(bw=-1), dict(bw=5001), dict(dist=7, bw=8), dict(gap=-1),
                        dict(gap=256), dict(pred=-1), dict(score=-1)):
                assert call(**bad) == INVALID, bad
            assert call(offs=at(4)) == INVALID                      # d_offsets, d_chain_offsets, d_totals 8-byte aligned
            assert call(co=at(4)) == INVALID
            assert call(tt=at(4)) == INVALID
            assert call(rows=at(8)) == INVALID                      # d_rows, d_chains 16-byte aligned
            assert call(ch=at(8)) == INVALID
            assert call(ac=at(2)) == INVALID and call(ap=at(2)) == INVALID and call(asc=at(1)) == INVALID      # anchor arrays 4-byte
            assert call(tab=p, nc=0) == INVALID                     # a table given with n_contigs < 1
            assert call(tab=p, nc=-1) == INVALID
            assert call(tab=None, nc=1) == INVALID                  # a null table with n_contigs != 0
            assert call(tab=None, nc=-1) == INVALID
            assert call(tab=at(4), nc=2) == INVALID
            assert call(tab=p, nc=2**31 - 1) == TOO_LONG
            assert call(wsp=None) == CAPACITY
            assert call(wsp=at(16)) == CAPACITY                     # workspace 256-byte aligned
            assert call(wsb=bytes_ok - 1) == CAPACITY
            assert call(wsb=0) == CAPACITY
            assert call(dist=0, wsp=None) == INVALID                # a bad argument is reported before a capacity
            assert call() == NO_DEVICE                              # every argument was fine
            assert call(ch=None) == NO_DEVICE and call(ch=None, cap=0) == NO_DEVICE      # the sizing call
            assert call(ac=None) == NO_DEVICE and call(ap=None) == NO_DEVICE and call(asc=None) == NO_DEVICE and call(tt=None) == NO_DEVICE
            assert call(ac=None, ap=None, asc=None, tt=None, ch=None) == NO_DEVICE
            assert call(dist=2**22, bw=2**22, gap=255, pred=2**31 - 1, score=2**31 - 1) == NO_DEVICE
            assert call(dist=1, bw=0, gap=0, pred=0, score=0) == NO_DEVICE
            assert call(offs=at(8), co=at(8), tt=at(8), rows=at(16), ch=at(16), ac=at(4), ap=at(4), asc=at(4)) == NO_DEVICE
            assert call(R=0, rows=None) == NO_DEVICE                # units without rows
            assert call(U=0, wsp=None, wsb=0) == NO_DEVICE          # no unit needs no workspace
    finally:
        lib.genie_index_destroy(h)


def test_python_layer_refuses_a_host_only_handle(pkg):
    ref = np.random.default_rng(2).integers(0, 4, 3000).astype(np.uint8)
    ix = pkg.GenieIndex.build(ref, 8)                               # host-only: no device was touched
    assert callable(ix.chain_mems) and callable(pkg.SMEM.chain_mems) and callable(pkg.SMEM.find_chains)
    with pytest.raises(Exception):
        ix.chain_mems(np.asarray([0, 1], np.int64), np.asarray([[0, 10, 1, 0]], np.int32))


# ------------------------------------------------------------------ the brute force against itself
def _random_units(count, seed):
    rng = np.random.default_rng(seed)
    for k in range(count):
        n = int(rng.integers(0, 60))
        rows = CU.synth_unit(rng, n, 4096, diagonals=int(rng.integers(1, 5)), jitter=int(rng.integers(0, 4)), step=int(rng.integers(2, 12)))
        cuts = np.sort(rng.integers(0, 4097, int(rng.integers(0, 4))))
        ctg = np.concatenate([[0], cuts, [4096]]) if k % 2 else None
        prm = P(int(rng.choice([1, 7, 60, 300, 2**22])), 0, int(rng.choice([0, 2, 16, 255])), int(rng.choice([0, 1, 3, 64])),
                int(rng.choice([0, 20, 40])))
        yield rows, ctg, prm._replace(bandwidth=int(rng.choice([0, min(5, prm.max_dist), prm.max_dist])))


def test_the_two_extractions_agree_and_f_rises_along_links():
    units = anchors = links = ties = many = 0
    for rows, ctg, prm in _random_units(2200, 5):
        f, p, t = CU.forward(rows, prm, ctg)
        a, b = CU.chains_by_top(f, p), CU.chains_by_backtrack(f, p)
        assert a == b
        has = p >= 0
        assert (f[has] > f[p[has]]).all() and (p[has] < np.flatnonzero(has)).all()
        assert (f >= rows[:, 1] - rows[:, 0]).all()
        top = CU.tops(f, p)
        assert all((top[v] == v) == (not (p == v).any()) for v in range(len(f)))      # the tops are the leaves
        x, y = CU.expected_unit(rows, prm, ctg, CU.chains_by_top), CU.expected_unit(rows, prm, ctg, CU.chains_by_backtrack)
        assert all(np.array_equal(u, v) for u, v in zip(x[:4], y[:4])) and x[4:] == y[4:]
        units, anchors, links, ties, many = units + 1, anchors + len(f), links + int(has.sum()), ties + t, many + (len(a) > 1)
    assert units >= 2000 and anchors > 40000 and links > 10000 and ties > 500 and many > 500, (units, anchors, links, ties, many)


# ------------------------------------------------------------------ hand-written cases
def _unit(*anchors):
    return np.asarray([[s, e, pos, -1] for s, e, pos in anchors], np.int64).reshape(-1, 4)


def _one(rows, prm, ctg=None):
    chains, achain, p, f, lost, _ = CU.expected_unit(rows, prm, ctg)
    return chains.tolist(), achain.tolist(), p.tolist(), f.tolist(), lost


def test_hand_written_cases():
    base = P(5000, 500, 2, 0, 0)
    # two anchors on one diagonal, 5 bases apart: gain = min(10, 15, 15)
    two = _unit((0, 10, 100), (15, 25, 115))
    assert _one(two, base) == ([[0, 25, 100, 125, 20, 2, 0, 1]], [0, 0], [-1, 0], [10, 20], 0)
    assert _one(two, base._replace(min_score=21)) == ([], [-1, -1], [-1, 0], [10, 20], 1)
    # a 5-base deletion (dr - dq = 5) at gap_cost 0, 16 (one base per base) and 255 (79 bases: no link)
    gap = _unit((0, 20, 100), (20, 40, 125))
    assert _one(gap, base._replace(gap_cost=0))[2:4] == ([-1, 0], [20, 40])
    assert _one(gap, base._replace(gap_cost=16))[2:4] == ([-1, 0], [20, 35])
    assert _one(gap, base._replace(gap_cost=255)) == ([[0, 20, 100, 120, 20, 1, 0, 0], [20, 40, 125, 145, 20, 1, 0, 1]], [0, 1], [-1, -1],
                                                      [20, 20], 0)
    assert _one(gap, base._replace(bandwidth=4, gap_cost=0))[2] == [-1, -1]
    assert _one(gap, base._replace(max_dist=24, bandwidth=24, gap_cost=0))[2] == [-1, -1]      # dr = 25
    # equal starts never link (dq = 0), whatever the positions
    assert _one(_unit((5, 15, 100), (5, 15, 130), (5, 25, 140)), base)[2] == [-1, -1, -1]
    # a tie takes the larger j: both predecessors give 10 + 10
    tie = _unit((0, 10, 1), (0, 10, 6), (20, 30, 21))
    assert _one(tie, base._replace(gap_cost=0)) == ([[0, 10, 1, 11, 10, 1, 0, 0], [0, 30, 6, 31, 20, 2, 0, 2]], [0, 1, 1], [-1, -1, 1],
                                                    [10, 10, 20], 0)
    assert _one(tie, base._replace(gap_cost=16))[2] == [-1, -1, 0]                             # the gap now costs 5
    # a link that does not beat l_i gives p = -1: 5 + min(10, 5, 5) equals l_1; 3 + 1 is below it
    assert _one(_unit((0, 5, 1), (5, 15, 6)), base)[2:4] == ([-1, -1], [5, 10])
    assert _one(_unit((0, 3, 1), (1, 21, 2)), base)[2:4] == ([-1, -1], [3, 20])
    assert _one(_unit((0, 5, 1), (5, 14, 6)), base)[2:4] == ([-1, 0], [5, 10])
    # max_pred = 1 cuts a better link
    cut = _unit((0, 30, 1), (10, 12, 2000), (40, 50, 41))
    assert _one(cut, base)[2:4] == ([-1, -1, 0], [30, 2, 40])
    assert _one(cut, base._replace(max_pred=2))[2:4] == ([-1, -1, 0], [30, 2, 40])
    assert _one(cut, base._replace(max_pred=1))[2:4] == ([-1, -1, -1], [30, 2, 10])
    # a contig boundary between two otherwise perfect anchors: t = 99 and t = 114
    assert _one(two, base, [0, 1000])[2] == [-1, 0]
    assert _one(two, base, [0, 50, 1000])[0] == [[0, 25, 100, 125, 20, 2, 1, 1]]
    assert _one(two, base, [0, 110, 110, 1000]) == ([[0, 10, 100, 110, 10, 1, 0, 0], [15, 25, 115, 125, 10, 1, 2, 1]], [0, 1], [-1, -1],
                                                    [10, 10], 0)
    # the score of a chain that branches off another: f(top) - f(p(first))
    fork = _unit((0, 10, 1), (20, 30, 21), (20, 25, 21), (40, 50, 41))
    chains, achain, p, f, lost = _one(fork, base._replace(gap_cost=0))
    assert p == [-1, 0, 0, 1] and f == [10, 20, 15, 30]
    assert chains == [[20, 25, 21, 26, 5, 1, 0, 2], [0, 50, 1, 51, 30, 3, 0, 3]] and achain == [1, 1, 0, 1]
    # the empty unit
    assert _one(np.zeros((0, 4), np.int64), base) == ([], [], [], [], 0)
