"""GPU: the memory contract of genie_select_alignments, on the guarded buffers of tests/guarded.py through the raw call of
tests/select_util.py, the way tests/test_cigars_contract_gpu.py checks genie_chain_cigars:

  - d_class, d_sel_offsets, d_sel, d_records, d_read_counts, d_totals and the workspace have exactly the declared bytes, the
    weakest alignment the header allows and 4 KiB of guard on each side; every guard holds its poison afterwards, the inputs (read
    offsets, chain offsets, chain rows, d_aln, contig table, index image) are unchanged; rows of d_class at or past C and entries
    past min(total, cap_sel) are not written;
  - the result does not depend on what outputs and workspace held before: the same bytes under the poisons 0x00, 0xFF, 0x5A;
  - d_aln and chain rows that break the call's assumptions (in-range garbage: the kernels clamp every position and the contig
    index, and bound the rounds of a read by its chain count) change no byte outside the outputs, and the call returns.  These
    are runs on valid allocations; none is meant to fault.

Every well-formed result is also compared with the brute force.  All comparisons are exact."""
import numpy as np
import pytest

import contract_calls as CC
import select_util as SU
from guarded import POISONS, Arena

pytestmark = pytest.mark.gpu

N_REF = 1 << 14
TABLE = np.asarray([0, 3000, 3000, 9000, N_REF], np.int64)
D = SU.DEFAULTS
COUNTS = [3, 0, 9, 8, 70, 1, 2, SU.TILE + 40, 12, 0, 5]


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
    e.b = SU.random_batch(np.random.default_rng(61), COUNTS, 2, skipped=0.1, contigs=4)
    return e


def _three(env, b, prm, table, cap, cap_sel, **kw):
    import torch
    results = []
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    for poison in POISONS:
        a = Arena("cuda", poison)
        a.freeze(env.ix.blob, "index image")
        torch.cuda.synchronize()                       # the arena's fill is done before anything runs on another stream
        with torch.cuda.stream(stream):                # the input copies go ahead of the call on its stream
            call = SU.guarded_call(env.lib, env.ix, a, stream.cuda_stream, b, prm, table, cap, cap_sel, **kw)
        torch.cuda.synchronize()
        res = call.result()
        a.check()
        a.check_frozen()
        results.append(res)
    for other in results[1:]:
        CC.same(results[0], other)
    return results[0]


@pytest.mark.parametrize("table", [None, TABLE], ids=["no_table", "table"])
def test_memory_contract(env, table):
    total = int(env.b["chain_offsets"][-1])
    n_sel = int(SU.expected(env.b, D, table)["offsets"][-1])
    assert n_sel > 20
    for kw in (dict(cap_sel=n_sel), dict(cap_sel=0, sizing=True), dict(cap_sel=n_sel - 1), dict(cap_sel=n_sel + 7, extras=False),
               dict(cap_sel=0), dict(cap_sel=n_sel, cap=total - 20), dict(cap_sel=n_sel, cap=total + 3), dict(cap_sel=3, cap=0)):
        cap = kw.pop("cap", total)
        want = SU.expected(env.b, D, table, cap, kw["cap_sel"])
        res = _three(env, env.b, D, table, cap, **kw)
        for key in res:
            assert np.array_equal(res[key], want[key]), (kw, key)
        assert ("sel" in res) == (not kw.get("sizing") and kw["cap_sel"] > 0) and ("totals" in res) == kw.get("extras", True)


@pytest.mark.parametrize("what", ["query", "reference", "flags", "scores", "contigs", "lengths"])
def test_inputs_that_break_the_assumptions_stay_inside_the_outputs(env, what):
    rng = np.random.default_rng(62)
    b = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in env.b.items()}
    Cn = b["aln"].shape[0]
    wild = [-2**31, -10**6, -41, -1, 0, 1, 500, 10**6, 2**30, 2**31 - 1]
    hit = rng.random(Cn) < 0.5
    if what == "query":
        for col in (1, 2):
            rows_ = rng.random(Cn) < 0.5
            b["aln"][rows_, col] = rng.choice(wild, int(rows_.sum())).astype(np.int32)
    elif what == "reference":
        for col in (3, 4):
            b["aln"][hit, col] = rng.choice(wild, int(hit.sum())).astype(np.int32)
    elif what == "flags":
        b["aln"][:, 5] = rng.integers(-2**31, 2**31 - 1, Cn)
        b["aln"][:, 6:] = rng.integers(-2**31, 2**31 - 1, (Cn, 2))
    elif what == "scores":
        b["aln"][hit, 0] = rng.choice(wild, int(hit.sum())).astype(np.int32)
    elif what == "contigs":
        b["chains"][:, 6] = rng.choice([-1, -2**31, 2**31 - 1, 4, 5, 1], Cn)
    else:
        b["read_offsets"] = np.cumsum(np.concatenate([[0], rng.choice([0, 1, 7, 2**31 + 5, 2**40], len(COUNTS))])).astype(np.int64)
    for cap_sel in (0, 5, Cn):
        res = _three(env, b, D, TABLE, Cn, cap_sel)      # guards, inputs and poison-independence
        klass, off = res["klass"], res["offsets"]
        assert klass.shape == (Cn, 4) and np.isin(klass[:, 0], (0, 1, 2, 3)).all()
        assert ((klass[:, 3] >= 0) & (klass[:, 3] <= 60)).all() and (klass[:, 2] >= -1).all()
        chosen = np.add.reduceat(np.concatenate([klass[:, 2] >= 0, [False]]).astype(np.int64), env.b["chain_offsets"][:-1:2])
        chosen[np.asarray(COUNTS) == 0] = 0
        assert np.array_equal(np.diff(off), chosen) and res["totals"][3] == off[-1]
        assert np.array_equal(res["totals"][:3], res["counts"][:, :3].sum(0))
        if cap_sel:
            assert np.array_equal(klass[res["sel"], 2] + off[res["records"][:, 0]], np.arange(res["sel"].size))
