"""GPU: the memory contract of genie_chain_mems, on the guarded buffers of tests/guarded.py through the raw call of
tests/chain_util.py, the way tests/test_mems_contract_gpu.py checks genie_find_mems:

  - d_chain_offsets, d_chains, the three anchor arrays, d_totals and the workspace have exactly the declared bytes, the
    weakest alignment the header allows and 4 KiB of guard on each side; every guard holds its poison afterwards, the inputs
    (offsets, rows, contig table, index image) are unchanged; chains past cap_chains and anchors past off[U] are not written;
  - the result does not depend on what outputs and workspace held before: the same bytes under the poisons 0x00, 0xFF, 0x5A;
  - rows that break the call's assumptions (unsorted starts, pos outside [1, n], end <= start) change no byte outside the
    outputs, and the call returns;
  - offsets that the device check refuses give GENIE_E_INVALID.

Every well-formed result is also compared with the brute force.  All comparisons are exact."""
import numpy as np
import pytest

import chain_util as CU
import contract_calls as CC
from guarded import POISONS, Arena

pytestmark = pytest.mark.gpu

P = CU.Params
N_REF = 1 << 14
TABLE = np.asarray([0, 3000, 3000, 9000, N_REF], np.int64)
PRM = P(900, 100, 2, 0, 30)


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
    e.ix = g.GenieIndex.build(np.random.default_rng(8).integers(0, 4, N_REF).astype(np.uint8), 0).to("cuda")
    e.offs, e.rows = CU.synth_batch(np.random.default_rng(13), [0, 1, 63, 64, 65, 0, 130, 600, 2100, 7], N_REF)
    return e


def _three(env, offs, rows, prm, table, cap, anchors=(True, True, True), totals=True, want_rc=0, slack=0):
    import torch
    results = []
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    for poison in POISONS:
        a = Arena("cuda", poison)
        a.freeze(env.ix.blob, "index image")
        torch.cuda.synchronize()                       # the arena's fill is done before anything runs on another stream
        with torch.cuda.stream(stream):                # the input copies go ahead of the call on its stream
            call = CU.guarded_call(env.lib, env.ix, a, stream.cuda_stream, offs, rows, prm, table, cap, anchors, totals, want_rc, slack)
        torch.cuda.synchronize()
        res = call.result() if want_rc == 0 else None
        assert call.rc == want_rc
        a.check()
        a.check_frozen()
        results.append(res)
    for other in results[1:]:
        if want_rc == 0:
            CC.same(results[0], other)
    return results[0]


@pytest.mark.parametrize("table", [None, TABLE], ids=["no_table", "table"])
def test_memory_contract(env, table):
    want = CU.expected(env.offs, env.rows, PRM, table)
    total = want["chains"].shape[0]
    assert total > 20 and want["totals"][1] > 20
    for cap, anchors, totals, slack in ((total, (True, True, True), True, 0), (total // 3, (True, False, True), False, 5),
                                        (total + 9, (False, True, False), True, 0), (0, (False, False, False), False, 3)):
        res = _three(env, env.offs, env.rows, PRM, table, cap, anchors, totals, slack=slack)
        assert np.array_equal(res["offsets"], want["offsets"])
        assert np.array_equal(res["chains"], want["chains"][:min(cap, total)])
        for k, w in zip(("anchor_chain", "anchor_pred", "anchor_score"), anchors):
            assert (k in res) == w and (not w or np.array_equal(res[k], want[k]))
        assert ("totals" in res) == totals and (not totals or np.array_equal(res["totals"], want["totals"]))


@pytest.mark.parametrize("what", ["unsorted", "position", "length"])
def test_rows_that_break_the_assumptions_stay_inside_the_outputs(env, what):
    rng = np.random.default_rng(14)
    rows = env.rows.copy()
    R = rows.shape[0]
    hit = rng.random(R) < 0.2
    if what == "unsorted":
        rows[hit, 0] = rng.integers(-2**31, 2**31 - 1, int(hit.sum()))
    elif what == "position":
        rows[hit, 2] = rng.choice([0, -1, -2**31, 2**31 - 1, N_REF + 1, N_REF + 5000], int(hit.sum()))
    else:
        rows[hit, 1] = rows[hit, 0] - rng.integers(0, 50, int(hit.sum()))
        rows[::97, 1] = -2**31
    for table in (None, TABLE):
        res = _three(env, env.offs, rows, PRM, table, R, slack=4)      # guards, inputs and poison-independence are checked there
        co = res["offsets"]
        assert co[0] == 0 and (np.diff(co) >= 0).all() and co[-1] <= R
        assert ((res["anchor_pred"] >= -1) & (res["anchor_pred"] < np.diff(env.offs).max())).all()


def test_bad_offsets_are_refused_on_the_device(env):
    R = env.rows.shape[0]
    for bad in (lambda o: o + 1,                                               # off[0] != 0
                lambda o: np.concatenate([o[:4], [o[4] - 70], o[5:]]),         # decreasing
                lambda o: np.concatenate([o[:-1], [R + 1]]),                   # off[U] above total_rows
                lambda o: np.concatenate([[0, -5], o[2:]])):                   # negative
        offs = bad(env.offs.copy())
        assert _three(env, offs, env.rows, PRM, TABLE, 10, want_rc=CU.INVALID) is None
