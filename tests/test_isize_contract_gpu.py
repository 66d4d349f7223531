"""GPU: the memory contract of genie_insert_size_stats, on the guarded buffers of tests/guarded.py through the raw call of
tests/isize_util.py, the way tests/test_pair_contract_gpu.py checks genie_pair_alignments:

  - d_stats, d_samples, d_totals and the workspace have exactly the declared bytes, the weakest alignment the header allows and
    4 KiB of guard on each side; every guard holds its poison afterwards, the inputs (record offsets, records, index image) are
    unchanged;
  - the result does not depend on what outputs and workspace held before: the same bytes under the poisons 0x00, 0xFF, 0x5A;
  - records that break the call's assumptions (in-range garbage: the kernels clamp the record ranges, count no span outside
    [1, max_span] and loop over bins alone) change no byte outside the outputs, and the call returns; decreasing record offsets
    give GENIE_E_INVALID.  These are runs on valid allocations; none is meant to fault.

Every well-formed result is also compared with the brute force.  All comparisons are exact."""
import numpy as np
import pytest

import contract_calls as CC
import isize_util as IU
from guarded import POISONS, Arena
from pair_util import FR, NO_TYPE, RF, SAME

pytestmark = pytest.mark.gpu

N_REF = 1 << 14
D = IU.Params(20, 6000, 5)
N_PAIRS = 700


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
    rng = np.random.default_rng(97)
    kinds = [FR, FR, FR, RF, SAME, NO_TYPE, "contigs"]
    plan = []
    for k in range(N_PAIRS):
        if k % 23 == 0:
            plan.append(("none", "left", "right")[k % 3])
        else:
            far = IU.LDS_BINS if k % 5 == 0 else 0                  # some spans beyond the range counted in LDS, some past max_span
            plan.append((kinds[int(rng.integers(0, len(kinds)))], int(rng.integers(100, 2200)) + far, int(rng.integers(5, 61))))
    e.b = IU.batch_of(plan, extra=1)
    return e


def _three(env, b, prm, **kw):
    import torch
    results = []
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    for poison in POISONS:
        a = Arena("cuda", poison)
        a.freeze(env.ix.blob, "index image")
        torch.cuda.synchronize()                       # the arena's fill is done before anything runs on another stream
        with torch.cuda.stream(stream):                # the input copies go ahead of the call on its stream
            call = IU.guarded_call(env.lib, env.ix, a, stream.cuda_stream, b, prm, **kw)
        torch.cuda.synchronize()
        a.check()
        a.check_frozen()
        if kw.get("want_rc"):
            assert call.rc == kw["want_rc"], call.rc
            continue
        results.append(call.result())
    for other in results[1:]:
        CC.same(results[0], other)
    return results[0] if results else None


def test_memory_contract(env):
    total = env.b["records"].shape[0]
    so = env.b["sel_offsets"]
    for prm, kw in ((D, dict()), (D, dict(totals=False)), (D, dict(samples=False)), (D, dict(samples=False, totals=False)),
                    (D, dict(n_records=total - 1)), (D, dict(n_records=int(so[5]) + 1)), (D, dict(n_records=total + 7)),
                    (D, dict(n_records=0)), (D._replace(max_span=1), dict()), (D._replace(max_span=IU.LDS_BINS - 1), dict()),
                    (D._replace(max_span=IU.LDS_BINS), dict()), (D._replace(max_span=IU.WINDOW_MAX // 2, min_mapq=0), dict())):
        want = IU.expected(env.b, prm, kw.get("n_records"))
        res = _three(env, env.b, prm, **kw)
        for key in res:
            assert np.array_equal(res[key], want[key]), (prm, kw, key)
        assert ("totals" in res) == kw.get("totals", True) and ("samples" in res) == kw.get("samples", True)


@pytest.mark.parametrize("what", ["kinds", "strands", "contigs", "offsets", "spans", "scores", "mapq", "everything"])
def test_inputs_that_break_the_assumptions_stay_inside_the_outputs(env, what):
    rng = np.random.default_rng(98)
    b = {k: v.copy() for k, v in env.b.items()}
    T = b["records"].shape[0]
    wild = [-2**31, -10**6, -41, -1, 0, 1, 2, 3, 500, 10**6, 2**30, 2**31 - 1]

    def spoil(col, share=0.5):
        hit = rng.random(T) < share
        b["records"][hit, col] = rng.choice(wild, int(hit.sum())).astype(np.int32)
    for name, cols in (("kinds", (0, 1, 2)), ("strands", (3,)), ("contigs", (4,)), ("offsets", (5,)), ("spans", (6,)), ("scores", (9, 10)),
                       ("mapq", (11,))):
        if what in (name, "everything"):
            for col in cols:
                spoil(col)
    for prm, kw in ((D, dict()), (D, dict(n_records=T - 5)), (D._replace(max_span=IU.WINDOW_MAX // 2, min_mapq=0, min_samples=1), dict())):
        res = _three(env, b, prm, **kw)                  # guards, inputs and poison-independence
        stats, samples, totals = res["stats"], res["samples"], res["totals"]
        assert stats.shape == (3, 12) and samples.shape == (N_PAIRS, 2)
        took = samples[:, 0] >= 0
        assert ((samples[:, 0] >= -1) & (samples[:, 0] <= 2)).all() and (samples[~took, 1] == 0).all()
        assert ((samples[took, 1] >= 1) & (samples[took, 1] <= prm.max_span)).all()      # a span outside is never counted
        assert (totals >= 0).all() and totals[0] == totals[1:].sum() and totals[0] <= N_PAIRS and totals[1] == took.sum()
        assert stats[:, 0].sum() == totals[1] and ((stats >= 0) & (stats <= 2**31)).all() and (stats[:, 11] <= prm.max_span).all()
        if what in ("kinds", "scores", "mapq"):                      # columns the definition clamps, or does not read at all
            want = IU.expected(b, prm, kw.get("n_records"))
            for key in res:
                assert np.array_equal(res[key], want[key]), (what, key)


def test_decreasing_record_offsets_are_refused(env):
    so = env.b["sel_offsets"]
    for bad in (so[::-1].copy(), np.concatenate([so[:4], so[3:4] - 1, so[5:]]), np.concatenate([[1], so[1:]]), -so):
        assert not ((np.diff(bad) >= 0).all() and bad[0] == 0)
        _three(env, dict(env.b, sel_offsets=bad), D, want_rc=IU.INVALID)      # the guards and the inputs hold here too
