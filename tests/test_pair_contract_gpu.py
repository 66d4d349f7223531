"""GPU: the memory contract of genie_pair_alignments, on the guarded buffers of tests/guarded.py through the raw call of
tests/pair_util.py, the way tests/test_select_contract_gpu.py checks genie_select_alignments:

  - d_pairs, d_sam, d_totals and the workspace have exactly the declared bytes, the weakest alignment the header allows and 4 KiB
    of guard on each side; every guard holds its poison afterwards, the inputs (record offsets, records, class rows, index image)
    are unchanged; rows of d_sam at or past R are not written;
  - the result does not depend on what outputs and workspace held before: the same bytes under the poisons 0x00, 0xFF, 0x5A;
  - records and class rows that break the call's assumptions (in-range garbage: the kernels clamp the record ranges and the chain
    index, and bound a pair's work by the product of its record counts) change no byte outside the outputs, and the call returns;
    decreasing record offsets give GENIE_E_INVALID.  These are runs on valid allocations; none is meant to fault.

Every well-formed result is also compared with the brute force.  All comparisons are exact."""
import numpy as np
import pytest

import contract_calls as CC
import pair_util as PU
from guarded import POISONS, Arena

pytestmark = pytest.mark.gpu

N_REF = 1 << 14
D = PU.DEFAULTS._replace(orient=7)
COUNTS = [(3, 2), (0, 4), (9, 8), (1, 1), (70, 1), (0, 0), (2, PU.TILE + 40), (12, 6), (5, 0)]


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
    e.b = PU.random_batch(np.random.default_rng(95), COUNTS)
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
            call = PU.guarded_call(env.lib, env.ix, a, stream.cuda_stream, b, prm, **kw)
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
    caps = env.b["klass"].shape[0]
    so = env.b["sel_offsets"]
    for kw in (dict(), dict(totals=False), dict(n_records=total - 1), dict(n_records=int(so[5]) + 3), dict(n_records=total + 7),
               dict(n_records=0), dict(cap=0), dict(cap=caps - 50), dict(cap=caps + 3)):
        want = PU.expected(env.b, D, kw.get("n_records"), kw.get("cap"))
        res = _three(env, env.b, D, **kw)
        for key in res:
            assert np.array_equal(res[key], want[key]), (kw, key)
        assert ("totals" in res) == kw.get("totals", True)


@pytest.mark.parametrize("what", ["kinds", "contigs", "chains", "offsets", "spans", "scores", "class", "everything"])
def test_inputs_that_break_the_assumptions_stay_inside_the_outputs(env, what):
    rng = np.random.default_rng(96)
    b = {k: v.copy() for k, v in env.b.items()}
    T, Cn = b["records"].shape[0], b["klass"].shape[0]
    wild = [-2**31, -10**6, -41, -1, 0, 1, 2, 3, 500, 10**6, 2**30, 2**31 - 1]

    def spoil(col, share=0.5):
        hit = rng.random(T) < share
        b["records"][hit, col] = rng.choice(wild, int(hit.sum())).astype(np.int32)
    if what in ("kinds", "everything"):
        spoil(2)
        spoil(3)
    if what in ("contigs", "everything"):
        spoil(4)
    if what in ("chains", "everything"):
        spoil(1)
        spoil(0)
    if what in ("offsets", "everything"):
        spoil(5)
    if what in ("spans", "everything"):
        spoil(6)
    if what in ("scores", "everything"):
        spoil(9)
        spoil(11)
    if what in ("class", "everything"):
        b["klass"][:] = rng.choice(wild, (Cn, 4)).astype(np.int32)
    for kw in (dict(), dict(n_records=T - 5), dict(cap=7)):
        res = _three(env, b, D, **kw)                    # guards, inputs and poison-independence
        R = min(T, kw.get("n_records", T))
        pairs, sam = res["pairs"], res["sam"]
        assert pairs.shape == (len(COUNTS), 8) and sam.shape == (R, 4)
        assert ((pairs[:, :2] >= -1) & (pairs[:, :2] < R)).all() and ((pairs[:, 2] >= 0) & (pairs[:, 2] < 32)).all()
        assert ((sam[:, 2] >= -1) & (sam[:, 2] < R)).all() and (sam[:, 0] & 1).all() and not (sam[:, 0] & ~0x9fb).any()
        assert (res["totals"] >= 0).all() and res["totals"][0] + res["totals"][3] <= len(COUNTS)


def test_decreasing_record_offsets_are_refused(env):
    so = env.b["sel_offsets"]
    for bad in (so[::-1].copy(), np.concatenate([so[:4], so[3:4] - 1, so[5:]]), np.concatenate([[1], so[1:]]), -so):
        assert not ((np.diff(bad) >= 0).all() and bad[0] == 0)
        _three(env, dict(env.b, sel_offsets=bad), D, want_rc=PU.INVALID)      # the guards and the inputs hold here too
