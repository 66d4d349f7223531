"""GPU: genie_window_mems and genie_rescue_windows against the brute forces of tests/window_util.py, every output exactly
equal.  Read lengths and window lengths on both sides of the 32-base word, of the 64 and 128 diagonals of a wave's batches and of
GENIE_MAX_READ_LEN; windows at position 0 and ending at n; min_len 1 on a 5-base window; both strands; a tandem repeat, where
many rows share a start; the row cap at its border, through window rows and through input rows alone; units without a window
copied byte for byte; the sizing call, a capacity inside a unit, U == 0; more searched units than one grid of waves; and the
planner on the record counts of tests/test_pair_gpu.py.  Each expectation is computed on the CPU before the GPU is asked."""
import numpy as np
import pytest

import match_stats_util as MS
import pair_util as PU
import window_util as WU

pytestmark = pytest.mark.gpu

N_REF = 1 << 14
M = 12
LENGTHS = (1, M, 31, 32, 33, 64, 65, 150, 8192, 8193)
WINDOWS = (0, 1, M - 1, M, 63, 64, 65, 128, 1000)
HOMO = (3000, 5000)                                                  # a homopolymer stretch of the reference
TANDEM = (6000, 6300)                                                # a tandem repeat of period 7


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import genie_smem_amd as g

    class Env:
        pass
    e = Env()
    e.g, e.lib = g, g._native.lib()
    T = np.random.default_rng(60).integers(0, 4, N_REF).astype(np.uint8)
    T[HOMO[0]:HOMO[1]] = 0
    T[TANDEM[0]:TANDEM[1]] = np.resize(np.asarray([0, 1, 1, 2, 3, 0, 2], np.uint8), TANDEM[1] - TANDEM[0])
    e.T = T
    e.ix = g.GenieIndex.build(T, 0).to("cuda")
    return e


def _input_rows(rng, T, reads, S, windows, m, share=0.5, extra=3):
    """Synthetic input rows per unit: a share of the unit's true window rows under another column 3 (so that the union has
    repeats to drop), and a few random rows; ordered by (start, column 3) as genie_find_mems orders by (start, row)."""
    n = len(T)
    offs, rows = [0], []
    for Q, w in zip(MS.strand_reads(reads, S), windows):
        mine = []
        wb, we = WU.clamp_window(w, n)
        if we > wb and len(Q) <= 600:
            mine = [(s, e, p, int(rng.integers(0, n))) for s, e, p, _ in WU.window_rows(T, Q, wb, we, m) if rng.random() < share]
        for _ in range(int(rng.integers(0, extra + 1))):
            s = int(rng.integers(0, len(Q) + 1))
            mine.append((s, int(rng.integers(s, len(Q) + 1)), int(rng.integers(1, n + 1)), int(rng.integers(0, n))))
        mine.sort(key=lambda r: (r[0], r[3]))
        rows += mine
        offs.append(len(rows))
    return np.asarray(offs, np.int64), np.asarray(rows, np.int32).reshape(-1, 4)


def _exact(env, flags, reads, windows, m, in_offsets=None, in_rows=None):
    want = WU.expected(env.T, reads, 2 if flags & WU.BOTH else 1, windows, m, in_offsets, in_rows)
    got = WU.sized_call(env.lib, env.ix, flags, reads, windows, m, in_offsets, in_rows)
    WU.agrees(got, want)
    return want


def test_read_lengths_and_window_lengths(env):
    rng = np.random.default_rng(61)
    lengths = [L for L in LENGTHS for _ in WINDOWS]
    wlens = [B for _ in LENGTHS for B in WINDOWS]
    reads, windows = WU.planted_units(rng, env.T, lengths, wlens, M, S=2)
    off, rows, st, tt = _exact(env, WU.BOTH, reads, windows, M)
    assert set(st.tolist()) == {0, WU.SEARCHED, WU.TOO_LONG_READ} and tt[2] == len(WINDOWS) - 1 and tt[0] == tt[1] > 60
    per_len = {L: int(np.diff(off).reshape(len(LENGTHS), -1)[k].sum()) for k, L in enumerate(LENGTHS)}
    assert per_len[8192] > 0 and per_len[8193] == 0 and per_len[150] > 0 and per_len[33] > 0, per_len
    ioff, irows = _input_rows(rng, env.T, reads, 2, windows, M)     # the same batch with input rows: union, repeats, units copied
    off2, rows2, st2, tt2 = _exact(env, WU.BOTH | WU.SPLIT, reads, windows, M, ioff, irows)
    assert tt2[1] < tt[1] and tt2[0] > tt[0] and np.array_equal(st, st2)


def test_window_edges_short_minimum_and_strands(env):
    T, n = env.T, N_REF
    reads = [T[0:40].copy(), MS.rc(T[n - 40:n]), T[5:10].copy(), T[n - 3:n].copy(), MS.rc(T[0:33]), T[100:164].copy()]
    windows = [(0, 30), (0, 0), (0, 0), (n - 50, n), (3, 8), (3, 8), (n - 5, n), (n - 5, n), (0, 64), (-7, 40), (n - 60, n + 9), (100, 164)]
    for m in (1, 3, 5):
        off, rows, st, tt = _exact(env, WU.BOTH, reads, windows, m)
        assert st.tolist() == [1, 0, 0, 1] + [1] * 8
    off, rows, st, tt = _exact(env, WU.BOTH, reads, windows, 1)
    first = rows[off[0]:off[1]]
    assert [0, 30, 1, -1] in first.tolist() and (first[:, 2] <= 30).all() and rows[off[3]:off[4]].tolist().count([0, 40, n - 39, -1]) == 1
    assert [0, 3, 6, -1] in rows[off[4]:off[5]].tolist() and [0, 3, n - 2, -1] in rows[off[6]:off[7]].tolist()
    # one strand only: the units are the reads
    _exact(env, 0, reads, windows[0::2], 2)
    # garbage windows are clamped as the header says: negative, reversed, past n
    wild = [(-5, 7), (9, 2), (n - 4, n + 100), (n + 5, n + 9), (-9, -1), (2**31 - 1, -2**31), (0, 0), (0, 3), (5, 5), (-2**31, 2**31 - 1),
            (1, 2), (16000, 17000)]
    _exact(env, WU.BOTH, reads, wild, 2)


def test_a_tandem_repeat_window(env):
    T = env.T
    reads = [T[TANDEM[0] + 10:TANDEM[0] + 70].copy(), T[TANDEM[0] + 3:TANDEM[0] + 153].copy()]
    off, rows, st, tt = _exact(env, 0, reads, [(TANDEM[0] - 20, TANDEM[1] + 20), TANDEM], M)
    starts = rows[off[0]:off[1], 0]
    assert (starts == 0).sum() > 30 and np.diff(off).min() > 40      # one row per period from the same start


def test_the_row_cap_at_its_border(env):
    Q = np.zeros(150, np.uint8)
    windows = [(HOMO[0], HOMO[0] + 1925), (HOMO[0], HOMO[0] + 1926), (HOMO[0] + 74, HOMO[1])]
    ioff, irows = np.asarray([0, 0, 2, 3], np.int64), np.asarray([(0, 150, 3001, 5), (0, 20, 9, 6), (7, 9, 11, 2)], np.int32)
    off, rows, st, tt = _exact(env, 0, [Q, Q, Q], windows, 14, ioff, irows)
    assert st.tolist() == [WU.SEARCHED, WU.ROW_CAP, WU.ROW_CAP] and np.diff(off).tolist() == [2048, 2, 1] and tt.tolist() == [2051, 2048, 2]
    # through input rows alone: 2048 rows and a window that adds nothing; 2049 rows
    rng = np.random.default_rng(62)
    many = np.stack([rng.integers(0, 100, 2049), rng.integers(100, 151, 2049), rng.permutation(8000)[:2049] + 1, np.arange(2049)], axis=1)
    many = many[np.argsort(many[:, 0], kind="stable")].astype(np.int32)
    lone = env.T[200:350].copy()
    for k, status in ((2048, WU.SEARCHED), (2049, WU.ROW_CAP)):
        off, rows, st, tt = _exact(env, 0, [lone], [(9000, 9005)], 14, np.asarray([0, k], np.int64), many[:k])
        assert st.tolist() == [status] and tt.tolist() == [k, 0, int(status == WU.ROW_CAP)]
        if status == WU.ROW_CAP:
            assert np.array_equal(rows, many[:k])                   # kept as they are, not sorted
    # the last row that fits: 2047 input rows and one window row
    two = [env.T[1000:1030].copy()]
    off, rows, st, tt = _exact(env, 0, two, [(990, 1040)], 14, np.asarray([0, 2047], np.int64), many[:2047])
    assert st.tolist() == [WU.SEARCHED] and tt.tolist() == [2048, 1, 0]


def test_the_sizing_call_a_capacity_inside_a_unit_and_no_units(env):
    rng = np.random.default_rng(63)
    reads, windows = WU.planted_units(rng, env.T, [150] * 12, [400] * 12, M, S=2)
    ioff, irows = _input_rows(rng, env.T, reads, 2, windows, M)
    want = WU.expected(env.T, reads, 2, windows, M, ioff, irows)
    total = int(want[0][-1])
    assert total > 30
    for cap in (total - 1, int(want[0][5]) + 1, 1, 0):
        off, rows, st, tt = WU.call_mems(env.lib, env.ix, WU.BOTH, reads, windows, M, ioff, irows, cap=cap)
        WU.agrees((off, rows[:cap], st, tt), (want[0], want[1][:cap], want[2], want[3]))
        assert (rows[cap:] == -7).all(), "rows past the capacity were written"
    bare = WU.call_mems(env.lib, env.ix, WU.BOTH, reads, windows, M, ioff, irows, cap=total, status=False, totals=False)
    assert bare[2] is None and bare[3] is None and np.array_equal(bare[1][:total], want[1])
    off, rows, st, tt = WU.call_mems(env.lib, env.ix, WU.BOTH, [], np.zeros((0, 2), np.int32), M, cap=4)
    assert off.tolist() == [0] and tt.tolist() == [0, 0, 0] and (rows == -7).all()
    down = ioff[::-1].copy()
    WU.call_mems(env.lib, env.ix, WU.BOTH, reads, windows, M, down, irows, cap=total, want_rc=WU.INVALID)


def test_more_searched_units_than_one_grid_of_waves(env):
    rng = np.random.default_rng(64)
    pool, n_units, m = 250, 70000, 8
    reads, windows = WU.planted_units(rng, env.T, [20] * pool, [40] * pool, m, S=1, subs=0.05)
    off, rows, st, tt = WU.expected(env.T, reads, 1, windows, m)
    reps = n_units // pool
    assert reps * pool == n_units and st.tolist() == [1] * pool and tt[0] > pool // 2
    per = np.diff(off)
    want_off = np.zeros(n_units + 1, np.int64)
    want_off[1:] = np.cumsum(np.tile(per, reps))
    want = (want_off, np.tile(rows, (reps, 1)), np.tile(st, reps), tt * reps)
    got = WU.sized_call(env.lib, env.ix, 0, reads * reps, np.tile(windows, (reps, 1)), m)
    WU.agrees(got, want)


# ------------------------------------------------------------------ the planner
BORDERS = [(0, 0), (0, 1), (1, 0), (1, 1), (1, 6), (6, 6), (8, 8), (8, 9), (1, 64), (1, 65), (64, 64), (300, 2), (2, 300), (0, 300)]
TABLE = np.asarray([0, 7000, N_REF], np.int64)


def _plan_batch(rng, counts):
    b = PU.random_batch(rng, counts, scores=(30, 60))
    b["records"][:, 5] = b["records"][:, 5] % 7300 + 1               # inside the 16 kb reference, some behind their contig's end
    b["pairs"] = PU.expected(b, PU.DEFAULTS._replace(orient=7))["pairs"]
    N = b["sel_offsets"].size - 1
    b["read_offsets"] = np.zeros(N + 1, np.int64)
    b["read_offsets"][1:] = np.cumsum(rng.integers(0, 3, N) * 75)    # a third of the reads without bases
    return b


def _plan_exact(env, b, table, orient, isize_max, anchor, **kw):
    want = WU.plan(N_REF, table, b["read_offsets"], b["sel_offsets"], b["records"], b["pairs"], orient, isize_max, anchor, kw.get("n_records"))
    got = WU.call_plan(env.lib, env.ix, b, table, orient, isize_max, anchor, **kw)
    WU.agrees(got, want)
    return want


def test_the_planner_on_the_pair_borders(env):
    rng = np.random.default_rng(65)
    b = _plan_batch(rng, BORDERS + [(1, 1)] * 40 + [(2, 0), (0, 2)] * 10)
    seen = np.zeros(3, np.int64)
    for orient in range(1, 8):
        for table in (TABLE, None):
            for isize_max, anchor in ((1000, 40), (1, 0), (WU.WINDOW_MAX // 2, 55)):
                seen += _plan_exact(env, b, table, orient, isize_max, anchor)[1]
    assert (seen > 100).all()
    so = b["sel_offsets"]
    total = int(so[-1])
    for n_records in (int(so[5]) + 4, int(so[4]) + 2, int(so[3]), 1, 0, total - 1, total + 5):      # n_records cuts a pair
        _plan_exact(env, b, TABLE, 7, 1000, 40, n_records=n_records)
    bare = WU.call_plan(env.lib, env.ix, b, TABLE, 7, 1000, 40, totals=False)
    assert bare[1] is None
    e = {"sel_offsets": np.zeros(1, np.int64), "records": np.zeros((0, 12), np.int32), "pairs": np.zeros((0, 8), np.int32),
         "read_offsets": np.zeros(1, np.int64)}
    win, tt = WU.call_plan(env.lib, env.ix, e, TABLE, 7, 1000, 40)   # N == 0: zero totals and nothing else
    assert win.shape == (0, 2) and tt.tolist() == [0, 0, 0]
    WU.call_plan(env.lib, env.ix, dict(b, sel_offsets=so[::-1].copy()), TABLE, 7, 1000, 40, want_rc=WU.INVALID)


def test_the_python_layer(env):
    rng = np.random.default_rng(66)
    reads, windows = WU.planted_units(rng, env.T, [150] * 6, [500] * 6, M, S=2)
    bases, roff = WU.csr(reads)
    want = WU.expected(env.T, reads, 2, windows, M)
    got = env.ix.window_mems(bases, roff, windows, M, both_strands=True, rows_hint=2)      # a hint too small: the call is made again
    WU.agrees([t.cpu().numpy() for t in got], want)
    b = _plan_batch(rng, [(1, 1)] * 6 + [(1, 0)] * 6)
    win, tt = env.ix.rescue_windows(b["read_offsets"], b["sel_offsets"], b["records"], b["pairs"], None, orient="any", isize_max=500,
                                    min_anchor_score=35)
    WU.agrees((win.cpu().numpy(), tt.cpu().numpy()),
              WU.plan(N_REF, None, b["read_offsets"], b["sel_offsets"], b["records"], b["pairs"], 7, 500, 35))
