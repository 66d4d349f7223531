"""GPU: the memory contract of genie_align_chains, on the guarded buffers of tests/guarded.py through the raw call of
tests/align_util.py, the way tests/test_chains_contract_gpu.py checks genie_chain_mems:

  - d_aln, d_totals and the workspace have exactly the declared bytes, the weakest alignment the header allows and 4 KiB of
    guard on each side; every guard holds its poison afterwards, the inputs (bases, the three offset arrays, rows, anchor arrays,
    chain rows, contig table, index image) are unchanged; rows of d_aln past min(total, cap_chains) are not written;
  - the result does not depend on what outputs and workspace held before: the same bytes under the poisons 0x00, 0xFF, 0x5A;
  - rows, chain rows, anchor arrays, chain offsets and tables that break the call's assumptions (in-range garbage: the kernels
    clamp every index and position) change no byte outside the outputs, and the call returns;
  - read offsets and row offsets that the device check refuses give GENIE_E_INVALID.

Every well-formed result is also compared with the brute force.  All comparisons are exact."""
import numpy as np
import pytest

import align_util as AU
import contract_calls as CC
from guarded import POISONS, Arena

pytestmark = pytest.mark.gpu

N_REF = 1 << 14
TABLE = np.asarray([0, 3000, 3000, 9000, N_REF], np.int64)
PRM = AU.Params(1, 2, 2, 1, 40, 30, 3)


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
    rng = np.random.default_rng(13)
    units = []
    for k in range(30):
        g_ = int(rng.choice([0, 2, 3]))
        chains, Qs = [], []
        for _ in range(int(rng.integers(0, 3)) if k % 5 else 0):
            spec = [(int(rng.integers(3, 25)), int(rng.integers(0, 20)), int(rng.integers(0, 20))) for _ in range(int(rng.integers(1, 40)))]
            if len(spec) > 3 and rng.random() < 0.3:
                spec[1] = (spec[1][0], 2, 40)                        # |B - A| above max_indel: a skipped chain
            span = sum(l + B for l, A, B in spec)
            t0 = int(rng.integers(TABLE[g_], TABLE[g_ + 1] - span))
            Q, rows = AU.synth_chain(rng, e.T, t0, spec, int(rng.integers(0, 70)), int(rng.integers(0, 70)), 0.1)
            chains.append((rows, g_))
            Qs.append(Q)
        Q, shift, moved = np.concatenate(Qs + [rng.integers(0, 4, 9).astype(np.uint8)]), 0, []
        for (rows, c), q in zip(chains, Qs):
            moved.append(([(s + shift, e_ + shift, pos) for s, e_, pos in rows], c))
            shift += len(q)
        units += [(Q, moved), (AU.revcomp(Q), [])] if k % 2 else [(AU.revcomp(Q), []), (Q, moved)]
    e.b = AU.make_batch(units, 2)
    return e


def _three(env, b, table, cap, totals=True, want_rc=0, slack=0):
    import torch
    results = []
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    for poison in POISONS:
        a = Arena("cuda", poison)
        a.freeze(env.ix.blob, "index image")
        torch.cuda.synchronize()                       # the arena's fill is done before anything runs on another stream
        with torch.cuda.stream(stream):                # the input copies go ahead of the call on its stream
            call = AU.guarded_call(env.lib, env.ix, a, stream.cuda_stream, b, PRM, table, cap, totals, want_rc, slack)
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
    total = int(env.b["chain_offsets"][-1])
    assert total > 20
    for cap, totals, slack in ((total, True, 0), (total // 3, False, 5), (total + 9, True, 0), (0, True, 3)):
        want = AU.expected(env.b, PRM, env.T, table, cap)
        res = _three(env, env.b, table, cap, totals, slack=slack)
        assert np.array_equal(res["aln"], want[0])
        assert ("totals" in res) == totals and (not totals or np.array_equal(res["totals"], want[1]))
    assert want[1].tolist() == [0, 0] and (AU.expected(env.b, PRM, env.T, table)[0][:, 5] == 4).sum() >= 2


@pytest.mark.parametrize("what", ["rows", "positions", "lengths", "chains", "pred", "chain", "chain_offsets", "table"])
def test_inputs_that_break_the_assumptions_stay_inside_the_outputs(env, what):
    rng = np.random.default_rng(14)
    b = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in env.b.items()}
    R, Cn = b["rows"].shape[0], b["chains"].shape[0]
    hit = rng.random(R) < 0.2
    table = TABLE
    if what == "rows":
        b["rows"][hit, 0] = rng.integers(-2**31, 2**31 - 1, int(hit.sum()))
    elif what == "positions":
        b["rows"][hit, 2] = rng.choice([0, -1, -2**31, 2**31 - 1, N_REF + 1, N_REF + 5000], int(hit.sum()))
    elif what == "lengths":
        b["rows"][hit, 1] = b["rows"][hit, 0] - rng.integers(0, 50, int(hit.sum()))
        b["rows"][::97, 1] = -2**31
        b["rows"][1::97, 1] = 2**31 - 1
    elif what == "chains":
        b["chains"][::2, 6] = rng.choice([-1, -2**31, 2**31 - 1, 4, 1], b["chains"][::2].shape[0])
        b["chains"][1::3, 7] = rng.choice([-1, -2**31, 2**31 - 1, R, 0], b["chains"][1::3].shape[0])
    elif what == "pred":
        b["anchor_pred"][hit] = rng.integers(-2**31, 2**31 - 1, int(hit.sum()))
        b["anchor_pred"][::7] = np.arange(R)[::7] % 40                # in range, and often not below the row itself
    elif what == "chain":
        b["anchor_chain"][:] = rng.integers(-2, 3, R)
    elif what == "chain_offsets":
        co = b["chain_offsets"]
        co[1:-1] = rng.integers(-5, Cn + 5, co.size - 2)
    else:
        table = np.asarray([5000, -7, 2**40, 100, -2**62], np.int64)
    for cap in (Cn, Cn // 2):
        res = _three(env, b, table, cap, slack=4)      # guards, inputs and poison-independence are checked there
        assert res["aln"].shape == (cap, 8) and sum(res["totals"]) == cap
    if what == "chain_offsets":
        b["chain_offsets"][-1] = -3                                   # no chain at all
        res = _three(env, b, table, Cn)
        assert res["aln"].shape[0] == 0 and res["totals"].tolist() == [0, 0]


def test_bad_offsets_are_refused_on_the_device(env):
    def changed(key, f):
        b = dict(env.b)
        b[key] = f(env.b[key].copy())
        return b
    R, nb = env.b["rows"].shape[0], env.b["bases"].size
    for key, bad in (("offsets", lambda o: o + 1),                                              # off[0] != 0
                     ("offsets", lambda o: np.concatenate([o[:4], [o[4] - 70], o[5:]])),        # decreasing
                     ("offsets", lambda o: np.concatenate([o[:-1], [R + 1]])),                  # off[U] above total_rows
                     ("offsets", lambda o: np.concatenate([[0, -5], o[2:]])),                   # negative
                     ("read_offsets", lambda o: np.concatenate([o[:3], [o[3] - 5000], o[4:]])), # decreasing
                     ("read_offsets", lambda o: np.concatenate([o[:-1], [nb + 1]])),            # above total_bases
                     ("read_offsets", lambda o: np.concatenate([[-1], o[1:]]))):                # negative
        assert _three(env, changed(key, bad), TABLE, 10, want_rc=AU.INVALID) is None
