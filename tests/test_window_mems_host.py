"""CPU-only tests of genie_rescue_windows and genie_window_mems (mate rescue: where to seed a mate again, and the MEMs of a
strand-read against a window of the reference): the symbols, constants and the header's wording, the C ABI's argument checks
in their documented order (before the device check, so a host-only handle reaches them), both workspace formulas against the
header's figures, and the brute forces of tests/window_util.py on hand-written cases pinned with literal rows."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import match_stats_util as MS
import window_util as WU

INVALID, NO_DEVICE, CAPACITY, TOO_LONG = WU.INVALID, WU.NO_DEVICE, WU.CAPACITY, WU.TOO_LONG
T16 = np.asarray([0, 1, 2, 3, 0, 0, 1, 1, 2, 2, 3, 3, 0, 2, 1, 3], np.uint8)      # ACGT AACC GGTT AGCT


@pytest.fixture(scope="module")
def pkg():
    import genie_smem_amd as g
    g._native.build()
    return g


# ------------------------------------------------------------------ window MEMs, by hand
def _one(Q, window, m, S=1, in_offsets=None, in_rows=None, reads=None):
    off, rows, st, tt = WU.expected(T16, [Q] if reads is None else reads, S, window, m, in_offsets, in_rows)
    return off.tolist(), rows.tolist(), st.tolist(), tt.tolist()


def test_a_match_clipped_at_both_window_edges():
    Q = T16[2:12]                                                    # GTAACCGGTT equals T[2:12); the window holds AACCGG only
    assert _one(Q, [(4, 10)], 4) == ([0, 1], [[2, 8, 5, -1]], [1], [1, 1, 0])
    assert _one(Q, [(0, 16)], 4) == ([0, 1], [[0, 10, 3, -1]], [1], [1, 1, 0])      # the whole reference: the unclipped MEM
    assert _one(Q, [(4, 10)], 7) == ([0, 0], [], [1], [0, 0, 0])      # searched, nothing long enough


def test_a_read_equal_to_the_window():
    assert _one(T16[4:10], [(4, 10)], 6) == ([0, 1], [[0, 6, 5, -1]], [1], [1, 1, 0])
    assert _one(T16[4:10], [(4, 4)], 1) == ([0, 0], [], [0], [0, 0, 0])             # no window: not searched


def test_a_code_4_inside_a_match():
    Q = T16[2:12].copy()
    Q[5] = 4
    assert _one(Q, [(0, 16)], 3) == ([0, 2], [[0, 5, 3, -1], [6, 10, 9, -1]], [1], [2, 2, 0])


def test_strand_1():
    read = MS.rc(T16[4:10])                                          # unit 1, its reverse complement, is the window itself
    assert _one(None, [(0, 0), (4, 10)], 6, S=2, reads=[read]) == ([0, 0, 1], [[0, 6, 5, -1]], [0, 1], [1, 1, 0])
    assert _one(None, [(4, 10), (0, 0)], 6, S=2, reads=[read]) == ([0, 0, 0], [], [1, 0], [0, 0, 0])


def test_a_duplicate_triple_keeps_the_inputs_column_3():
    got = _one(T16[4:10], [(4, 10)], 6, in_offsets=[0, 1], in_rows=[(0, 6, 5, 77)])
    assert got == ([0, 1], [[0, 6, 5, 77]], [1], [1, 0, 0])
    got = _one(T16[4:10], [(4, 4)], 6, in_offsets=[0, 1], in_rows=[(0, 6, 5, 77)])
    assert got == ([0, 1], [[0, 6, 5, 77]], [0], [1, 0, 0])


def test_equal_starts_in_suffix_array_order_come_out_by_pos():
    rows_in = [(0, 3, 9, 5), (0, 3, 2, 6)]                           # (start, row) order as genie_find_mems writes it: pos 9 before pos 2
    got = _one(T16[4:10], [(4, 10)], 6, in_offsets=[0, 2], in_rows=rows_in)
    assert got == ([0, 3], [[0, 3, 2, 6], [0, 6, 5, -1], [0, 3, 9, 5]], [1], [3, 1, 0])
    got = _one(T16[4:10], [(7, 7)], 6, in_offsets=[0, 2], in_rows=rows_in)          # without a window: byte for byte, in their order
    assert got == ([0, 2], [[0, 3, 9, 5], [0, 3, 2, 6]], [0], [2, 0, 0])


def test_window_clamping_and_caps():
    assert WU.clamp_window((-5, 9), 16) == (0, 9) and WU.clamp_window((9, 4), 16) == (9, 9) and WU.clamp_window((3, 99), 16) == (3, 16)
    assert WU.clamp_window((40, 50), 16) == (16, 16) and WU.clamp_window((0, 10**6), 10**6) == (0, WU.WINDOW_MAX)
    T = np.zeros(2000, np.uint8)
    Q = np.zeros(150, np.uint8)
    for B, status, rows in ((1925, WU.SEARCHED, 2048), (1926, WU.ROW_CAP, 0)):      # L + B + 1 - 2 m rows: the cap at its border
        off, out, st, tt = WU.expected(T, [Q], 1, [(0, B)], 14)
        assert st.tolist() == [status] and out.shape[0] == rows and tt.tolist() == [rows, rows, int(status == WU.ROW_CAP)]
    long_read = np.zeros(WU.MAX_READ_LEN + 1, np.uint8)
    off, out, st, tt = WU.expected(T, [long_read], 1, [(0, 5)], 3, [0, 1], [(0, 5, 1, 9)])
    assert st.tolist() == [WU.TOO_LONG_READ] and out.tolist() == [[0, 5, 1, 9]] and tt.tolist() == [1, 0, 1]


# ------------------------------------------------------------------ the planner, by hand
TABLE = np.asarray([0, 1000, 3000], np.int64)                        # the anchor lies in contig 1: [1000, 3000)
NONE = [0, 0]


def _plan(reads, orient, isize_max=400, min_anchor=40, proper=(), table=TABLE, lengths=None):
    b = WU.plan_batch(reads, lengths)
    for k in proper:
        b["pairs"][k, 2] |= 1
    win, tt = WU.plan(3000, table, b["read_offsets"], b["sel_offsets"], b["records"], b["pairs"], orient, isize_max, min_anchor)
    return win.tolist(), tt.tolist()


@pytest.mark.parametrize("mask", range(1, 8))
@pytest.mark.parametrize("sa", [0, 1])
def test_every_orientation_mask_and_anchor_strand(mask, sa):
    # the anchor: b = 500, e = 600 inside contig 1; RIGHT [500, 900), LEFT [200, 600), both [200, 900)
    opposite = {(1, 0): [1500, 1900], (1, 1): [1200, 1600], (2, 0): [1200, 1600], (2, 1): [1500, 1900], (3, 0): [1200, 1900],
                (3, 1): [1200, 1900], (0, 0): NONE, (0, 1): NONE}[(mask & 3, sa)]
    same = [1200, 1900] if mask & 4 else NONE
    want = [NONE, NONE, NONE, NONE]
    want[2 + (1 - sa)], want[2 + sa] = opposite, same                # read 1 is the target: units 2 and 3
    n = (opposite != NONE) + (same != NONE)
    assert _plan([[(sa, 1, 501, 100, 60)], []], mask) == (want, [n, 1, 1])
    flipped = [want[2], want[3], NONE, NONE]                         # the anchor on mate 1: read 0 is the target
    assert _plan([[], [(sa, 1, 501, 100, 60)]], mask) == (flipped, [n, 1, 1])


def test_an_anchor_at_a_contig_start_and_at_a_contig_end():
    assert _plan([[(1, 1, 1, 100, 60)], []], 1) == ([NONE, NONE, [1000, 1100], NONE], [1, 1, 1])      # LEFT [-300, 100) cut at 0
    assert _plan([[(0, 1, 1901, 100, 60)], []], 1) == ([NONE, NONE, NONE, [2900, 3000]], [1, 1, 1])   # RIGHT [1900, 2300) cut at 2000
    assert _plan([[(0, 1, 2001, 100, 60)], []], 1) == ([NONE] * 4, [0, 0, 1])       # behind its contig's end: empty, still a target
    assert _plan([[(0, 0, 501, 100, 60)], []], 1, table=None) == ([NONE, NONE, NONE, [500, 900]], [1, 1, 1])
    assert _plan([[(0, 7, 501, 100, 60)], []], 1) == ([NONE, NONE, NONE, [1500, 1900]], [1, 1, 1])    # the contig is clamped to the table
    assert _plan([[(0, 1, 501, 100, 60)], []], 1, isize_max=WU.WINDOW_MAX // 2)[0][3] == [1500, 3000]


def test_no_target():
    assert _plan([[(0, 1, 501, 100, 39)], []], 7) == ([NONE] * 4, [0, 0, 0])        # below min_anchor_score
    assert _plan([[(0, 1, 501, 100, 40)], []], 7)[1] == [2, 1, 1]                   # equality anchors
    assert _plan([[(0, 1, 501, 100, 60)], [(1, 1, 701, 100, 60)]], 7, proper=(0,)) == ([NONE] * 4, [0, 0, 0])
    assert _plan([[], []], 7) == ([NONE] * 4, [0, 0, 0])
    assert _plan([[(0, 1, 501, 100, 60)], []], 7, lengths=[100, 0]) == ([NONE] * 4, [0, 0, 1])      # a target without bases


def test_both_mates_as_targets():
    # not proper (the heads lie 1.6 kb apart, isize_max is 400): each mate is sought next to the other
    win, tt = _plan([[(0, 1, 101, 100, 60)], [(1, 1, 1701, 100, 60)]], 1)
    assert win == [[2400, 2800], NONE, NONE, [1100, 1500]] and tt == [2, 1, 2]      # LEFT of mate 1, RIGHT of mate 0, + 1000


def test_the_property_on_random_records():
    import pair_util as PU
    rng = np.random.default_rng(5)
    for _ in range(300):
        orient, most = int(rng.integers(1, 8)), int(rng.integers(1, 1200))
        sa, b, span = int(rng.integers(0, 2)), int(rng.integers(0, 1900)), int(rng.integers(1, 200))
        win, _ = _plan([[(sa, 1, b + 1, span, 60)], []], orient, isize_max=most)
        a = PU.Rec(0, [0, 0, 0, sa, 1, b + 1, span, 0, 0, 60, 0, 0])
        for _ in range(40):
            y = PU.Rec(1, [1, 1, 0, int(rng.integers(0, 2)), 1, int(rng.integers(1, 2000)), int(rng.integers(1, 200)), 0, 0, 60, 0, 0])
            if y.e > 2000 or not PU.concordant(a, y, PU.DEFAULTS._replace(orient=orient, isize_min=0, isize_max=most)):
                continue
            wb, we = win[2 + y.s]
            assert wb <= 1000 + y.b and 1000 + y.e <= we, (orient, most, sa, b, span, y.s, y.b, y.e, win)


# ------------------------------------------------------------------ the C layer
def test_symbols_and_constants(pkg):
    lib = pkg._native.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "genie_smem.h")).read()
    for name, nargs, res in (("genie_rescue_windows", 17, C.c_int), ("genie_rescue_windows_workspace_bytes", 1, C.c_int64),
                             ("genie_window_mems", 21, C.c_int), ("genie_window_mems_workspace_bytes", 1, C.c_int64)):
        assert name in pkg._native.SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is res and len(fn.argtypes) == nargs
        assert name + "(" in header
    assert lib.genie_abi_version() == 2 and pkg._native.ABI_VERSION == 2      # additions: the version stays
    consts = dict(re.findall(r"#define (GENIE_[A-Z_]+) (\d+)", header))
    assert int(consts["GENIE_WINDOW_MAX"]) == pkg._native.WINDOW_MAX == WU.WINDOW_MAX == 65536
    assert int(consts["GENIE_WINDOW_MAX_ROWS"]) == pkg._native.WINDOW_MAX_ROWS == WU.WINDOW_MAX_ROWS == 2048
    assert int(consts["GENIE_MAX_READ_LEN"]) == WU.MAX_READ_LEN
    assert (pkg._native.WINDOW_SEARCHED, pkg._native.WINDOW_ROW_CAP, pkg._native.WINDOW_TOO_LONG) == (1, 2, 4)
    for words in ("RIGHT [b, b + isize_max)", "LEFT  [e - isize_max, e)", "[e - isize_max, b + isize_max)", "left-maximal INSIDE THE WINDOW",
                  "(p, p + l, t + 1, -1)", "sorted ascending by (start, pos, end)", "56 bytes per unit", "4 bytes per read",
                  "choices sized to LDS", "decides no value"):
        assert words in header, words
    assert callable(pkg.GenieIndex.rescue_windows) and callable(pkg.GenieIndex.window_mems)
    assert callable(pkg.SMEM.rescue_windows) and callable(pkg.SMEM.window_mems)
    import inspect
    prm = inspect.signature(pkg.SMEM.map_pairs).parameters
    assert prm["rescue"].default is False and prm["rescue_options"].default is None


def test_workspace_formulas(pkg):
    lib = pkg._native.lib()
    up = lambda v: (v + 255) & ~255      # noqa: E731
    rw, wm = lib.genie_rescue_windows_workspace_bytes, lib.genie_window_mems_workspace_bytes
    assert rw(-1) == INVALID and wm(-1) == INVALID
    seen_r, seen_w = [], []
    for n in (0, 2, 64, 1000, 2050, 100002, 10**8):
        assert rw(n) == 256 + up(4 * n), n                           # the verdict, and the target mark of every read
        scan = ((n + 1023) // 1024 + 2) * 8 + 16
        assert wm(n) == 256 + sum(up(k * n) for k in WU.UNIT_BYTES) + up(8 * (n + 1)) + up(scan), n
        seen_r.append(rw(n))
        seen_w.append(wm(n))
    assert seen_r == sorted(seen_r) and seen_w == sorted(seen_w) and sum(WU.UNIT_BYTES) == 56
    big = 10**8
    per_unit = (wm(2 * big) - wm(big)) / big
    assert 64 <= per_unit < 64 + 8 / 1024 + 1e-4                      # 56, the list's offset 8, the scan


def _host_handle(lib):
    ref = np.random.default_rng(1).integers(0, 4, 2000).astype(np.uint8)
    h = C.c_void_p(0)
    assert lib.genie_index_create(ref.ctypes.data_as(C.POINTER(C.c_uint8)), ref.size, 8, 0, C.byref(h)) == 0
    return h


def test_rescue_windows_argument_checks_before_device(pkg):
    lib = pkg._native.lib()
    h = _host_handle(lib)
    try:
        buf = np.zeros(1 << 16, np.uint8)
        al = (buf.ctypes.data + 255) & ~255
        p = C.c_void_p(al)
        at = lambda k: C.c_void_p(al + k)      # noqa: E731
        ok = lib.genie_rescue_windows_workspace_bytes(4)

        def call(ix=h, tab=None, nc=0, roff=p, N=4, so=p, rec=p, nrec=10, pairs=p, orient=1, most=1000, anchor=40, win=p, tt=p, wsp=p,
                 wsb=ok):
            return lib.genie_rescue_windows(ix, tab, nc, roff, N, so, rec, nrec, pairs, orient, most, anchor, win, tt, wsp, wsb, None)

        assert call(ix=None) == INVALID and call(so=None) == INVALID
        assert call(N=3) == INVALID and call(N=-2) == INVALID and call(nrec=-1) == INVALID and call(wsb=-1) == INVALID
        assert call(roff=None) == INVALID and call(pairs=None) == INVALID and call(win=None) == INVALID and call(rec=None) == INVALID
        for bad in (dict(orient=0), dict(orient=8), dict(most=0), dict(most=WU.WINDOW_MAX // 2 + 1), dict(anchor=-1),
                    dict(anchor=(1 << 30) + 1)):
            assert call(**bad) == INVALID, bad
        for name in ("rec", "pairs"):                                   # 16-byte aligned
            assert call(**{name: at(8)}) == INVALID, name
        for name in ("roff", "so", "win", "tt"):                        # 8-byte aligned
            assert call(**{name: at(4)}) == INVALID, name
        assert call(nc=1) == INVALID and call(tab=p, nc=0) == INVALID and call(tab=at(4), nc=2) == INVALID
        assert call(tab=p, nc=2**31 - 1) == TOO_LONG
        assert call(N=2**31) == TOO_LONG and call(nrec=2**31) == TOO_LONG and call(N=2**31, orient=0) == INVALID
        assert call(N=2**31, wsp=None) == TOO_LONG
        assert call(wsp=None) == CAPACITY and call(wsp=at(16)) == CAPACITY and call(wsb=ok - 1) == CAPACITY
        assert call(orient=8, wsp=None) == INVALID
        assert call() == NO_DEVICE and call(tab=p, nc=3) == NO_DEVICE and call(tt=None) == NO_DEVICE
        assert call(orient=7, most=WU.WINDOW_MAX // 2, anchor=1 << 30) == NO_DEVICE and call(most=1, anchor=0) == NO_DEVICE
        assert call(nrec=0, rec=None) == NO_DEVICE
        assert call(N=0, roff=None, pairs=None, win=None, wsp=None, wsb=0) == NO_DEVICE
    finally:
        lib.genie_index_destroy(h)


def test_window_mems_argument_checks_before_device(pkg):
    lib = pkg._native.lib()
    h = _host_handle(lib)
    try:
        buf = np.zeros(1 << 16, np.uint8)
        al = (buf.ctypes.data + 255) & ~255
        p = C.c_void_p(al)
        at = lambda k: C.c_void_p(al + k)      # noqa: E731
        ok = lib.genie_window_mems_workspace_bytes(8)

        def call(ix=h, flags=1, bases=p, roff=p, N=4, total=600, max_len=150, U=8, win=p, m=12, ioff=p, irows=p, nin=10, offs=p, rows=p,
                 cap=100, st=p, tt=p, wsp=p, wsb=ok):
            return lib.genie_window_mems(ix, flags, bases, roff, N, total, max_len, U, win, m, ioff, irows, nin, offs, rows, cap, st, tt,
                                         wsp, wsb, None)

        assert call(ix=None) == INVALID and call(offs=None) == INVALID and call(roff=None) == INVALID and call(bases=None) == INVALID
        assert call(N=-1, U=-2) == INVALID and call(total=-1) == INVALID and call(max_len=-1) == INVALID and call(max_len=2**31) == INVALID
        assert call(flags=4) == INVALID and call(flags=8) == INVALID
        assert call(U=-1) == INVALID and call(U=4) == INVALID and call(flags=0, U=8) == INVALID and call(cap=-1) == INVALID
        assert call(nin=-1) == INVALID and call(wsb=-1) == INVALID and call(m=0) == INVALID and call(m=-3) == INVALID
        assert call(win=None) == INVALID and call(irows=None) == INVALID
        for name in ("rows", "irows"):                                  # 16-byte aligned
            assert call(**{name: at(8)}) == INVALID, name
        for name in ("offs", "ioff", "roff", "win", "tt"):              # 8-byte aligned
            assert call(**{name: at(4)}) == INVALID, name
        assert call(st=at(2)) == INVALID
        assert call(N=2**31, U=2**32) == TOO_LONG and call(N=2**31, U=2**32, wsp=None) == TOO_LONG and call(N=2**31, U=2**32, m=0) == INVALID
        assert call(wsp=None) == CAPACITY and call(wsp=at(16)) == CAPACITY and call(wsb=ok - 1) == CAPACITY and call(wsb=0) == CAPACITY
        assert call(m=0, wsp=None) == INVALID
        assert call() == NO_DEVICE and call(flags=3) == NO_DEVICE and call(flags=0, U=4) == NO_DEVICE and call(flags=2, U=4) == NO_DEVICE
        assert call(rows=None) == NO_DEVICE and call(st=None, tt=None) == NO_DEVICE and call(ioff=None, irows=None, nin=0) == NO_DEVICE
        assert call(ioff=None, irows=None, nin=5) == NO_DEVICE and call(nin=0, irows=None) == NO_DEVICE and call(m=2**31 - 1) == NO_DEVICE
        assert call(N=0, U=0, total=0, bases=None, win=None, wsp=None, wsb=0) == NO_DEVICE
    finally:
        lib.genie_index_destroy(h)


def test_python_layer(pkg):
    ref = np.random.default_rng(2).integers(0, 4, 3000).astype(np.uint8)
    ix = pkg.GenieIndex.build(ref, 8)                               # host-only: no device was touched
    with pytest.raises(Exception):
        ix.window_mems(np.zeros(4, np.uint8), np.asarray([0, 4], np.int64), np.zeros((1, 2), np.int32), 3)
    with pytest.raises(Exception):
        ix.rescue_windows(np.asarray([0, 4, 8], np.int64), np.asarray([0, 0, 0], np.int64), np.zeros((0, 12), np.int32),
                          np.zeros((1, 8), np.int32))
