"""GPU: the memory contract of genie_window_mems and genie_rescue_windows, on the guarded buffers of tests/guarded.py through the
raw calls of tests/window_util.py, the way tests/test_pair_contract_gpu.py checks genie_pair_alignments:

  - every output and the workspace have exactly the declared bytes, the weakest alignment the header allows and 4 KiB of guard on
    each side; every guard holds its poison afterwards, the inputs (reads, windows, input rows, records, pair rows, index image)
    are unchanged; rows of d_rows past the total are not written;
  - the result does not depend on what outputs and workspace held before: the same bytes under the poisons 0x00, 0xFF, 0x5A;
  - windows that are negative, reversed, past n or longer than GENIE_WINDOW_MAX, garbage input rows, and garbage pair rows and
    records for the planner change no byte outside the outputs, and the call returns; every window the planner writes satisfies
    0 <= wb <= we <= n and we - wb <= GENIE_WINDOW_MAX; decreasing input offsets give GENIE_E_INVALID.  These are runs on valid
    allocations; none is meant to fault.

Every well-formed result is also compared with the brute force.  All comparisons are exact."""
import numpy as np
import pytest

import contract_calls as CC
import pair_util as PU
import window_util as WU
from guarded import POISONS, Arena

pytestmark = pytest.mark.gpu

N_REF = 1 << 14
M = 12
TABLE = np.asarray([0, 7000, N_REF], np.int64)
WILD = [-2**31, -10**6, -41, -1, 0, 1, 2, 3, 500, 9000, 10**6, 2**30, 2**31 - 1]


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import genie_smem_amd as g

    class Env:
        pass
    e = Env()
    e.lib = g._native.lib()
    e.T = np.random.default_rng(8).integers(0, 4, N_REF).astype(np.uint8)
    e.ix = g.GenieIndex.build(e.T, 0).to("cuda")
    rng = np.random.default_rng(97)
    e.reads, e.windows = WU.planted_units(rng, e.T, [150, 33, 64, 1, 700, 150, 20, 150], [400, 64, 65, 5, 1000, 0, 40, 128], M, S=2)
    n = N_REF
    offs, rows = [0], []
    for u, (Q, w) in enumerate(zip(WU.MS.strand_reads(e.reads, 2), e.windows)):      # half of the true rows, and rows of their own
        mine = [r[:3] + (int(rng.integers(0, n)),) for r in WU.window_rows(e.T, Q, *WU.clamp_window(w, n), M) if rng.random() < 0.5]
        mine += [(int(rng.integers(0, len(Q) + 1)), len(Q), int(rng.integers(1, n)), int(rng.integers(0, n))) for _ in range(u % 4)]
        rows += sorted(mine, key=lambda r: (r[0], r[3]))
        offs.append(len(rows))
    e.in_offsets, e.in_rows = np.asarray(offs, np.int64), np.asarray(rows, np.int32).reshape(-1, 4)
    b = PU.random_batch(rng, [(3, 2), (0, 4), (9, 8), (1, 1), (70, 1), (0, 0), (1, 0), (0, 1), (12, 6), (5, 0)], scores=(30, 60))
    b["records"][:, 5] = b["records"][:, 5] % 7300 + 1
    b["pairs"] = PU.expected(b, PU.DEFAULTS._replace(orient=7))["pairs"]
    N = b["sel_offsets"].size - 1
    b["read_offsets"] = np.zeros(N + 1, np.int64)
    b["read_offsets"][1:] = np.cumsum(rng.integers(0, 3, N) * 75)
    e.b = b
    return e


def _three(env, make, want_rc=0):
    import torch
    results = []
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    for poison in POISONS:
        a = Arena("cuda", poison)
        a.freeze(env.ix.blob, "index image")
        torch.cuda.synchronize()                       # the arena's fill is done before anything runs on another stream
        with torch.cuda.stream(stream):                # the input copies go ahead of the call on its stream
            call = make(a, stream.cuda_stream)
        torch.cuda.synchronize()
        a.check()
        a.check_frozen()
        if want_rc:
            assert call.rc == want_rc, call.rc
            continue
        results.append(call.result())
    for other in results[1:]:
        CC.same(results[0], other)
    return results[0] if results else None


def _mems(env, windows, in_offsets, in_rows, cap, flags=WU.BOTH, want_rc=0, **kw):
    return _three(env, lambda a, s: WU.guarded_mems(env.lib, env.ix, a, s, flags, env.reads, windows, M, in_offsets, in_rows, cap,
                                                     want_rc=want_rc, **kw), want_rc)


def test_window_mems_memory_contract(env):
    want = WU.expected(env.T, env.reads, 2, env.windows, M, env.in_offsets, env.in_rows)
    total = int(want[0][-1])
    assert total > 20 and want[3][1] > 5 and set(want[2].tolist()) == {0, 1}
    for cap, kw in ((total, {}), (total + 9, {}), (total - 1, {}), (int(want[0][3]) + 1, {}), (0, {}), (total, dict(status=False)),
                    (total, dict(totals=False))):
        res = _mems(env, env.windows, env.in_offsets, env.in_rows, cap, **kw)
        assert np.array_equal(res["offsets"], want[0]) and np.array_equal(res["rows"], want[1][:cap])
        assert ("status" in res) == kw.get("status", True) and ("totals" in res) == kw.get("totals", True)
        if "status" in res:
            assert np.array_equal(res["status"], want[2])
        if "totals" in res:
            assert np.array_equal(res["totals"], want[3])
    bare = WU.expected(env.T, env.reads, 2, env.windows, M)          # without input rows
    res = _mems(env, env.windows, None, None, int(bare[0][-1]))
    assert np.array_equal(res["rows"], bare[1]) and np.array_equal(res["totals"], bare[3])


def test_garbage_windows_stay_inside_the_outputs(env):
    rng = np.random.default_rng(98)
    n = N_REF
    for windows in ([(-5, 70), (90, 20), (n - 40, n + 400), (n + 5, n + 9), (-9, -1), (2**31 - 1, -2**31), (-2**31, 2**31 - 1), (0, 2**31 - 1),
                     (3, 3), (n, n), (-2**31, 40), (n - 1, n), (100, 100 + WU.WINDOW_MAX + 5), (1, 0), (0, 0), (7000, 7100)],
                    rng.choice(WILD, (16, 2))):
        windows = np.asarray(windows, np.int64).astype(np.int32)
        want = WU.expected(env.T, env.reads, 2, windows, M, env.in_offsets, env.in_rows)      # the clamping is defined: exact
        res = _mems(env, windows, env.in_offsets, env.in_rows, int(want[0][-1]) + 4)
        for key, w in zip(("offsets", "rows", "status", "totals"), want):
            assert np.array_equal(res[key], w), key


def test_garbage_input_rows_stay_inside_the_outputs(env):
    rng = np.random.default_rng(99)
    rows = rng.choice(WILD, env.in_rows.shape).astype(np.int32)
    want = WU.expected(env.T, env.reads, 2, env.windows, M, env.in_offsets, rows)      # the union and its order are defined on any integers
    res = _mems(env, env.windows, env.in_offsets, rows, int(want[0][-1]) + 4)
    for key, w in zip(("offsets", "rows", "status", "totals"), want):
        assert np.array_equal(res[key], w), key
    spread = np.zeros_like(env.in_offsets)                           # every input row in one unit, the others empty
    spread[5:] = env.in_rows.shape[0]
    want = WU.expected(env.T, env.reads, 2, env.windows, M, spread, rows)
    res = _mems(env, env.windows, spread, rows, int(want[0][-1]))
    assert np.array_equal(res["rows"], want[1])


def test_decreasing_input_offsets_are_refused(env):
    off = env.in_offsets
    total = env.in_rows.shape[0]
    for bad in (off[::-1].copy(), np.concatenate([off[:4], off[3:4] - 1, off[5:]]), np.concatenate([[1], off[1:]]), -off, off + total):
        _mems(env, env.windows, bad, env.in_rows, 50, want_rc=WU.INVALID)      # the guards and the inputs hold here too


def _plan(env, b, table=TABLE, orient=7, isize_max=1000, anchor=40, want_rc=0, **kw):
    return _three(env, lambda a, s: WU.guarded_plan(env.lib, env.ix, a, s, b, table, orient, isize_max, anchor, want_rc=want_rc, **kw), want_rc)


def test_rescue_windows_memory_contract(env):
    b = env.b
    total = b["records"].shape[0]
    for kw in (dict(), dict(totals=False), dict(n_records=total - 1), dict(n_records=int(b["sel_offsets"][5]) + 3), dict(n_records=0),
               dict(n_records=total + 7)):
        for table in (TABLE, None):
            want = WU.plan(N_REF, table, b["read_offsets"], b["sel_offsets"], b["records"], b["pairs"], 7, 1000, 40, kw.get("n_records"))
            res = _plan(env, b, table, **kw)
            assert np.array_equal(res["windows"], want[0]) and ("totals" in res) == kw.get("totals", True)
            if "totals" in res:
                assert np.array_equal(res["totals"], want[1])
    assert WU.plan(N_REF, TABLE, b["read_offsets"], b["sel_offsets"], b["records"], b["pairs"], 7, 1000, 40)[1][0] > 3


@pytest.mark.parametrize("what", ["records", "pairs", "table", "everything"])
def test_garbage_records_and_pair_rows_stay_inside_the_outputs(env, what):
    rng = np.random.default_rng(100)
    b = {k: v.copy() for k, v in env.b.items()}
    table = TABLE.copy()
    if what in ("records", "everything"):
        hit = rng.random(b["records"].shape) < 0.5
        b["records"][hit] = rng.choice(WILD, int(hit.sum())).astype(np.int32)
    if what in ("pairs", "everything"):
        hit = rng.random(b["pairs"].shape) < 0.6
        b["pairs"][hit] = rng.choice(WILD + [4, 5, 6, 7, 20, 40], int(hit.sum())).astype(np.int32)
    if what in ("table", "everything"):
        table = np.asarray([5, -3, 2**40], np.int64)                 # a table genie_contigs_validate would refuse
    for isize_max in (1000, WU.WINDOW_MAX // 2):
        res = _plan(env, b, table, isize_max=isize_max)              # guards, inputs and poison-independence
        want = WU.plan(N_REF, table, b["read_offsets"], b["sel_offsets"], b["records"], b["pairs"], 7, isize_max, 40)
        assert np.array_equal(res["windows"], want[0]) and np.array_equal(res["totals"], want[1])      # the clamps are defined: exact
        w = res["windows"].astype(np.int64)
        assert ((0 <= w[:, 0]) & (w[:, 0] <= w[:, 1]) & (w[:, 1] <= N_REF) & (w[:, 1] - w[:, 0] <= WU.WINDOW_MAX)).all()


def test_decreasing_record_offsets_are_refused(env):
    so = env.b["sel_offsets"]
    for bad in (so[::-1].copy(), np.concatenate([[1], so[1:]]), -so):
        _plan(env, dict(env.b, sel_offsets=bad), want_rc=WU.INVALID)
