"""GPU tests of the mapping chain on batches wider than one grid (run with -m gpu on an MI355X): genie_chain_mems,
genie_align_chains, genie_chain_cigars and SMEM.map_reads over more than 2 G units, chains and selected chains, G = 16 waves per
CU being the stride of their grid-stride loops; more than three rounds of the one-block scans of 1024; direction storage past
2^31 bytes.  Every comparison is exact equality with the brute forces of tests/chain_util.py, tests/align_util.py and
tests/cigar_util.py, for the align and CIGAR calls put together from templates by tests/wide_map_util.py (which
tests/test_wide_map_host.py proves against the brute forces run directly).  Each test first asserts that its batch passes the
thresholds it is there for."""
import re

import numpy as np
import pytest

import align_util as AU
import chain_util as CH
import cigar_util as CU
import wide_map_util as W

pytestmark = pytest.mark.gpu

SWEEP = CH.Params(1500, 200, 2, 0, 30)       # windows of about 1500 rows: candidates leave the ring of 512
SETS = {1: None, 2: W.TABLE}


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import genie_smem_amd as g

    class Env:
        pass
    e = Env()
    e.g = g
    e.lib = g._native.lib()
    e.T = W.reference()
    e.ix = g.GenieIndex.build(e.T, 0).to("cuda")
    e.G = W.grid_waves(torch.cuda.get_device_properties(0).multi_processor_count)
    return e


def _wide(env, S):
    w = W.wide_batch(W.templates(env.T, SETS[S], 100 + S), S, SETS[S], 200 + S, env.G)
    return w, W.template_expectation(w, W.PRM, env.T)


@pytest.fixture(scope="module")
def wide1(env):
    return _wide(env, 1)


@pytest.fixture(scope="module")
def wide2(env):
    return _wide(env, 2)


# ------------------------------------------------------------------ 1. genie_chain_mems
def test_chain_mems_over_more_than_two_grids_of_units(env):
    G = env.G
    ix = env.g.GenieIndex.build(np.random.default_rng(7).integers(0, 4, 1 << 16).astype(np.uint8), 0).to("cuda")      # supplies only n
    offs, rows, sizes, heavy = W.chain_units(41, G)
    U = offs.size - 1
    assert U == 2 * G + 300 and rows.shape[0] > 4 * 256 and max(sizes) == 1500
    assert sum(1 for u in heavy if u < G and sizes[u + G] <= 6 and sizes[u + 2 * G] > 64) == 10
    assert sum(1 for u in heavy if G <= u < 2 * G and sizes[u - G] <= 6 and sizes[u + G] <= 6) == 10
    want = CH.expected(offs, rows, SWEEP, W.TABLE_CHAINS)
    total = want["chains"].shape[0]
    assert total > W.SCAN and want["totals"][1] > W.SCAN and want["ties"] > 100 and len(set(want["chains"][:, 6].tolist())) >= 3
    CH.agrees(CH.sized_call(env.lib, ix, offs, rows, SWEEP, W.TABLE_CHAINS), want)
    for cap in (total - 1, 0):
        got = CH.call(env.lib, ix, offs, rows, SWEEP, W.TABLE_CHAINS, cap=cap, spare=2)
        CH.agrees(got, want, cap)
        assert got["offsets"][-1] == total and (got["chains"][cap:] == -7).all()
    for k in range(3):
        anchors = tuple(j != k for j in range(3))
        got = CH.call(env.lib, ix, offs, rows, SWEEP, W.TABLE_CHAINS, cap=total, anchors=anchors, totals=k != 1)
        assert got[("anchor_chain", "anchor_pred", "anchor_score")[k]] is None and (got["totals"] is None) == (k == 1)
        CH.agrees(got, want)
    got = CH.call(env.lib, ix, offs, rows, SWEEP, W.TABLE_CHAINS, chains=False, anchors=(False, False, False), totals=False)
    assert np.array_equal(got["offsets"], want["offsets"])


# ------------------------------------------------------------------ 2. genie_align_chains
@pytest.mark.parametrize("S", (1, 2))
def test_align_chains_over_more_than_two_grids_of_chains(env, request, S):
    G = env.G
    w, te = request.getfixturevalue("wide1" if S == 1 else "wide2")
    total = w.tchain.size
    assert total > 2 * G + 256 and w.b["offsets"].size - 1 > 2 * G and total > 2 * W.SCAN
    assert te["ties"] > 20
    full = W.wide_aln(w, te)
    assert full[1][1] >= total // W.SCAN                             # skipped chains throughout
    AU.agrees(AU.call(env.lib, env.ix, w.b, W.PRM, w.table), full)
    for cap in (G, G + 1, total - 1, 1):
        AU.agrees(AU.call(env.lib, env.ix, w.b, W.PRM, w.table, cap=cap, spare=3), W.wide_aln(w, te, cap))
    if S == 2:                                                       # without the table the extensions run on across the contig bounds
        bare = W.template_expectation(w, W.PRM, env.T, table=None, cigars=False)
        other = W.wide_aln(w, bare)
        assert (other[0] != full[0]).any(1).sum() > 100
        AU.agrees(AU.call(env.lib, env.ix, w.b, W.PRM, None), other)


# ------------------------------------------------------------------ 3. genie_chain_cigars
def _sample(res, every):
    """Every `every`-th entry of a result, as a result of its own."""
    ks = np.arange(0, res["info"].shape[0], every)
    ops = [res["cigar"][res["offsets"][k]:res["offsets"][k + 1]] for k in ks]
    offsets = np.zeros(ks.size + 1, np.int64)
    offsets[1:] = np.cumsum([o.size for o in ops])
    return {"info": res["info"][ks], "offsets": offsets, "cigar": np.concatenate(ops)}


@pytest.mark.parametrize("S", (1, 2))
def test_chain_cigars_over_more_than_two_grids_of_selected_chains(env, request, S):
    G = env.G
    w, te = request.getfixturevalue("wide1" if S == 1 else "wide2")
    total = w.tchain.size
    assert total > 2 * G + 256 and total > 2 * W.SCAN
    aln = W.wide_aln(w, te)[0]
    want = W.wide_cigars(w, te)
    assert (want["need"] > 0).sum() > 2 * G and want["totals"][1] >= total // W.SCAN
    got = CU.call(env.lib, env.ix, w.b, W.PRM, aln, w.table)
    CU.agrees(got, want)
    part = _sample(got, 13)
    assert part["info"].shape[0] >= 500 and part["info"][-1, 0] > 2 * G
    assert CU.check_result(w.b, W.PRM, env.T, aln, part) >= 450


@pytest.fixture(scope="module")
def picked(env, wide1):
    """The selection of 3 x 1024 + 5 entries on the S == 1 batch: (sel, bad positions, the positions that need room, expectation)."""
    w, te = wide1
    needy = np.flatnonzero(te["need"][w.tchain] > 0)
    n = 3 * W.SCAN + 5
    at = (1022, 1023, 1024, 2047, 2048, n - 1)
    sel, bad = W.wide_selection(31, w.tchain.size, n, needy, at)
    return sel, bad, at, W.wide_cigars(w, te, sel)


def test_a_selection_of_three_rounds_and_five(env, wide1, picked):
    w, te = wide1
    sel, bad, at, want = picked
    assert sel.size == 3 * W.SCAN + 5 and {k // W.SCAN for k in bad} == {0, 1, 3} and (sel == 2**40).any() and (sel < 0).any()
    good = np.delete(sel, bad)
    assert np.unique(good).size < good.size and (np.diff(good) == -1).sum() > 1000
    assert (want["info"][bad, 1] == CU.BAD).all() and want["totals"][1] >= len(bad) + 10
    aln = W.wide_aln(w, te)[0]
    got = CU.call(env.lib, env.ix, w.b, W.PRM, aln, None, sel)
    CU.agrees(got, want)
    assert CU.check_result(w.b, W.PRM, env.T, aln, _sample(got, 5), None) >= 500


# ------------------------------------------------------------------ 4. the direction budget across rounds
def test_the_direction_budget_across_rounds(env, wide1, picked):
    w, te = wide1
    sel, bad, at, want = picked
    aln = W.wide_aln(w, te)[0]
    need, n = want["need"], sel.size
    run = np.cumsum(need)
    assert (need[list(at)] > 0).all()
    full = CU.cigar_strings(want["offsets"], want["cigar"])
    for k in at:
        for budget in (int(run[k]), int(run[k]) - 1):
            exp = W.wide_cigars(w, te, sel, dir_bytes=budget)
            got = CU.call(env.lib, env.ix, w.b, W.PRM, aln, None, sel, dir_bytes=budget)
            CU.agrees(got, exp)
            tight = np.flatnonzero(got["info"][:, 1] & CU.NO_ROOM)
            later = np.flatnonzero(need[k + 1:] > 0)
            first = k if budget < run[k] else (k + 1 + int(later[0]) if later.size else n)
            # flag 8 from exactly the first entry that needs room the budget does not have, on every entry behind it
            assert np.array_equal(tight, np.arange(first, n)), (k, budget, tight[:3], first)
            assert got["totals"][2] == run[-1] and np.array_equal(got["need"], need)
            free = np.flatnonzero(got["info"][:, 1] == 0)
            assert free.size == (want["info"][:first, 1] == 0).sum()
            texts = CU.cigar_strings(got["offsets"], got["cigar"])
            assert all(texts[j] == full[j] for j in free.tolist())
    # cap_ops inside a chain of the third round: nothing behind it is written (CU.call looks at the ops behind cap_ops)
    nops = np.diff(want["offsets"])
    k = int(np.flatnonzero(nops[2 * W.SCAN + 100:] >= 3)[0]) + 2 * W.SCAN + 100
    assert 2 * W.SCAN < k < 3 * W.SCAN
    cap_ops = int(want["offsets"][k]) + 1
    got = CU.call(env.lib, env.ix, w.b, W.PRM, aln, None, sel, cap_ops=cap_ops, dir_bytes=int(run[-1]))
    CU.agrees(got, dict(want, cigar=want["cigar"][:cap_ops]))
    assert got["offsets"][-1] == want["offsets"][-1] > cap_ops


# ------------------------------------------------------------------ 5. direction storage past 2^31 bytes
def test_direction_storage_past_two_gib(env):
    """A chain whose gap runs at 1024 diagonals over 829 rows needs about 430 KB; selected about 5000 times, with a narrow
    chain between them, the direction offsets pass 2^31."""
    import torch
    if torch.cuda.mem_get_info()[0] < 8 << 30:
        pytest.skip("needs 8 GiB of free device memory: the workspace alone is 2.3 GiB")
    rng = np.random.default_rng(1200)
    prm = AU.Params(1, 4, 6, 1, 100, 823, 5)
    units = []
    for A, B in ((829, 6), (9, 7)):
        Q, rows = W.chain(rng, env.T, [(20, A, B), (20, 0, 0)], 30, 30, rate=0.05)
        units.append((Q, [(rows, 0)]))
    b = AU.make_batch(units)
    aln = AU.expected(b, prm, env.T)[0]
    one = CU.expected(b, prm, env.T, aln)
    big, small = int(one["need"][0]), int(one["need"][1])
    assert big >= 829 * 16 * 32 and 0 < small < 64 * 1024
    reps = ((1 << 31) + big) // big + 2
    # as many of the narrow chain, in random order: two entries 1024 or a grid apart do not begin at the same place of their round
    sel = rng.permutation(np.tile(np.asarray([0, 1], np.int64), reps))
    want = CU.expected(b, prm, env.T, aln, None, sel)               # memoised per chain: the brute force runs twice
    assert want["totals"].tolist() == [2 * reps, 0, reps * (big + small)] and want["totals"][2] > (1 << 31) + big
    starts = np.cumsum(want["need"]) - want["need"]
    assert (starts > 1 << 31).sum() >= 2 and starts[-1] % big != 0   # chains that begin past 2^31, at no multiple of one need
    inside = starts - starts[np.arange(sel.size) // W.SCAN * W.SCAN]      # where an entry begins inside its round of the scan
    assert (inside[:-W.SCAN] != inside[W.SCAN:]).mean() > 0.9
    got = CU.call(env.lib, env.ix, b, prm, aln, None, sel, cap_ops=int(want["offsets"][-1]))
    CU.agrees(got, want)
    texts, single = np.asarray(CU.cigar_strings(got["offsets"], got["cigar"])), CU.cigar_strings(one["offsets"], one["cigar"])
    for c in (0, 1):                                                 # all entries of one chain are identical
        assert set(texts[sel == c].tolist()) == {single[c]} and (got["info"][sel == c, 1:] == one["info"][c, 1:]).all()


# ------------------------------------------------------------------ 6. SMEM.map_reads
def _ops(text):
    return re.findall(r"(\d+)([SIDX=])", text)


def test_map_reads_over_more_than_two_grids_of_strand_reads(env):
    g, G = env.g, env.G
    rng = np.random.default_rng(1700)
    rs = g.ReferenceSet(["a", "b", "c"], W.TABLE, env.T)
    m = g.ExactMatch("wide_map_reads.fa")
    m.set_reference("".join("ACGT"[c] for c in env.T))
    sm = g.SMEM(m, 4)
    N = G + 200
    nowhere = set(np.linspace(7, N - 3, 10).astype(int).tolist())    # in every pass of the strand-reads
    assert 2 * N > 2 * G and len({(2 * r) // G for r in nowhere}) == 3 and len(nowhere) == 10
    reads, truth = [], []
    for r in range(N):
        L = int(rng.integers(80, 121))
        c = int(rng.integers(0, 3))
        at = int(rng.integers(int(W.TABLE[c]), int(W.TABLE[c + 1]) - L))
        q = env.T[at:at + L].copy()
        n_sub = 0
        if r % 5 == 4:
            where = rng.choice(np.arange(20, L - 20), int(rng.integers(1, 4)), replace=False)
            q[where] = (q[where] + rng.integers(1, 4, where.size)) & 3
            n_sub = where.size
        strand = int(rng.integers(0, 2))
        if r in nowhere:
            q, strand = np.asarray([0, 1, 2, 3] * (L // 4), np.uint8), -1
        reads.append(AU.revcomp(q) if strand == 1 else q)
        truth.append((strand, c, at - int(W.TABLE[c]) + 1, len(q), n_sub))
    assert 0.4 < np.mean([t[0] == 1 for t in truth]) < 0.6
    strs = ["".join("ACGT"[c] for c in q) for q in reads]
    hits, offs, cigar = sm.map_reads(strs, 15, rs, min_score=25)
    hits, texts = hits.cpu().numpy(), g.cigar_strings(offs, cigar)
    assert hits.shape == (N, 6) and len(texts) == N
    for r, ((strand, c, off1, L, n_sub), hit, text) in enumerate(zip(truth, hits, texts)):
        if strand < 0:
            assert hit.tolist() == [-1, 0, -1, 0, 0, 0] and text == "", (r, hit, text)
            continue
        assert hit[0] >= 0 and hit[1:4].tolist() == [strand, c, off1], (r, hit, strand, c, off1)
        if not n_sub:
            assert text == f"{L}=" and hit[4] == L + 10 and hit[5] == 0, (r, text, hit)
        else:
            assert "S" not in text and hit[5] == sum(int(n) for n, o in _ops(text) if o in "XID"), (r, text, hit)
            assert sum(int(n) for n, o in _ops(text) if o in "=XI") == L
