"""GPU: the memory contract of genie_chain_cigars, on the guarded buffers of tests/guarded.py through the raw call of
tests/cigar_util.py, the way tests/test_align_contract_gpu.py checks genie_align_chains:

  - d_cigar_offsets, d_cigar, d_info, d_dir_need, d_totals and the workspace have exactly the declared bytes, the weakest
    alignment the header allows and 4 KiB of guard on each side; every guard holds its poison afterwards, the inputs (bases, the
    three offset arrays, rows, anchor arrays, chain rows, d_aln, d_sel, contig table, index image) are unchanged; ops past
    min(total, cap_ops) are not written;
  - the result does not depend on what outputs and workspace held before: the same bytes under the poisons 0x00, 0xFF, 0x5A;
  - rows, chain rows, anchor arrays, d_aln rows and selections that break the call's assumptions (in-range garbage: the kernels
    clamp every index and position, check every end cell and bound every trace) change no byte outside the outputs, and the
    call returns.  These are runs on valid allocations; none is meant to fault.

Every well-formed result is also compared with the brute force.  All comparisons are exact."""
import numpy as np
import pytest

import align_util as AU
import cigar_util as CU
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
    rng = np.random.default_rng(15)
    units = []
    for k in range(16):
        g_ = int(rng.choice([0, 2, 3]))
        chains, Qs = [], []
        for _ in range(int(rng.integers(0, 3)) if k % 5 else 0):
            spec = [(int(rng.integers(3, 25)), int(rng.integers(0, 20)), int(rng.integers(0, 20))) for _ in range(int(rng.integers(1, 12)))]
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
    e.aln = {"none": AU.expected(e.b, PRM, e.T, None)[0], "table": AU.expected(e.b, PRM, e.T, TABLE)[0]}
    return e


def _three(env, b, aln, table, cap, **kw):
    import torch
    results = []
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    for poison in POISONS:
        a = Arena("cuda", poison)
        a.freeze(env.ix.blob, "index image")
        torch.cuda.synchronize()                       # the arena's fill is done before anything runs on another stream
        with torch.cuda.stream(stream):                # the input copies go ahead of the call on its stream
            call = CU.guarded_call(env.lib, env.ix, a, stream.cuda_stream, b, PRM, aln, table, cap, **kw)
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
    aln = env.aln["none" if table is None else "table"]
    total = int(env.b["chain_offsets"][-1])
    assert total >= 10
    full = CU.expected(env.b, PRM, env.T, aln, table)
    ops, need = int(full["offsets"][-1]), int(full["totals"][2])
    assert (full["info"][:, 1] == 4).sum() >= 1 and need > 0
    sel = [total - 1, 0, 3, 3, -1, total, 2]
    for kw in (dict(cap_ops=ops, dir_bytes=need), dict(cap_ops=0, dir_bytes=need), dict(cap_ops=ops - 1, dir_bytes=need + 100),
               dict(cap_ops=ops, dir_bytes=need // 2), dict(cap_ops=ops + 7, dir_bytes=0, extras=False),
               dict(cap_ops=ops, dir_bytes=need, sel=sel), dict(cap_ops=3, dir_bytes=need, sel=[]), dict(cap_ops=ops, dir_bytes=need, cap=total // 2)):
        cap = kw.pop("cap", total)
        want = CU.expected(env.b, PRM, env.T, aln, table, kw.get("sel"), cap, kw["cap_ops"], kw["dir_bytes"])
        res = _three(env, env.b, aln, table, cap, **kw)
        for key in res:
            assert np.array_equal(res[key], want[key]), (kw, key)
        assert ("cigar" in res) == (kw["cap_ops"] > 0) and ("totals" in res) == kw.get("extras", True)


@pytest.mark.parametrize("what", ["rows", "positions", "lengths", "chains", "pred", "chain", "aln", "aln_flags", "sel"])
def test_inputs_that_break_the_assumptions_stay_inside_the_outputs(env, what):
    rng = np.random.default_rng(16)
    b = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in env.b.items()}
    aln = env.aln["table"].copy()
    R, Cn = b["rows"].shape[0], b["chains"].shape[0]
    hit = rng.random(R) < 0.2
    sel = None
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
    elif what == "aln":
        # end points outside the read, the contig and the band, and off by a little: inside the rectangle but not the optimum's
        for col in (1, 2, 3, 4):
            rows_ = rng.random(Cn) < 0.5
            aln[rows_, col] += rng.choice([-2**31, -10**6, -41, -3, -1, 1, 2, 41, 500, 10**6, 2**30], int(rows_.sum())).astype(np.int32)
    elif what == "aln_flags":
        aln[:, 5] = rng.integers(-2**31, 2**31 - 1, Cn)
        aln[:, 0] = rng.integers(-2**31, 2**31 - 1, Cn)
        aln[:, 6:] = rng.integers(-2**31, 2**31 - 1, (Cn, 2))
    else:
        sel = [int(v) for v in rng.choice([-1, -2**63, 2**63 - 1, Cn, Cn + 1, 2**31, 0, 1, Cn - 1], 40)]
    n = Cn if sel is None else len(sel)
    for cap_ops, dir_bytes in ((0, 1 << 20), (64, 1 << 20), (1 << 14, 1 << 12), (1 << 14, 1 << 22)):
        res = _three(env, b, aln, TABLE, Cn, sel=sel, cap_ops=cap_ops, dir_bytes=dir_bytes)      # guards, inputs and poison-independence
        assert res["info"].shape == (n, 8) and sum(res["totals"][:2]) == n
        flagged = res["info"][:, 1] != 0
        assert not res["info"][flagged, 2:].any() and (res["info"][:, 1] & ~28 == 0).all()
        assert np.array_equal(np.diff(res["offsets"]), res["info"][:, 2]) and res["totals"][1] == flagged.sum()
        assert res["totals"][2] == res["need"].sum() and (res["need"] >= 0).all()
    if what == "sel":
        assert (res["info"][:, 1] == 16).sum() >= 20 and (res["info"][:, 1] == 0).sum() >= 5
    if what == "aln":
        assert (res["info"][:, 1] == 16).sum() >= 3
