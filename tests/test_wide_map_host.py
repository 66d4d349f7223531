"""Host tests of tests/wide_map_util.py (no GPU): the wide batches pass the thresholds they are there for, on a device of 256
CUs (G = 4096 waves to a grid), their templates mix what shares a wave, and the expectation put together from the templates'
brute force equals AU.expected and CU.expected run directly on 600 consecutive units."""
import numpy as np
import pytest

import align_util as AU
import chain_util as CH
import cigar_util as CU
import wide_map_util as W

G = W.grid_waves(256)
SETS = {1: None, 2: W.TABLE}
_CACHE = {}


def _world(S):
    """(reference, wide batch, the templates' brute force), once."""
    if S not in _CACHE:
        T = W.reference()
        w = W.wide_batch(W.templates(T, SETS[S], 100 + S), S, SETS[S], 200 + S, G)
        _CACHE[S] = (T, w, W.template_expectation(w, W.PRM, T))
    return _CACHE[S]


@pytest.mark.parametrize("S", (1, 2))
def test_the_wide_batch_passes_its_thresholds(S):
    T, w, te = _world(S)
    b, C_ = w.b, w.tchain.size
    U = b["offsets"].size - 1
    assert C_ > 2 * G + 256 and U > 2 * G and C_ > 8 * W.SCAN
    assert (te["need"][w.tchain] > 0).sum() > 2 * G                  # chains the fill kernel has work for
    assert len(w.tmpl) == W.N_TEMPLATES and all(W.N_TEMPLATES % d for d in range(2, 16))      # prime
    # units u, u + G, u + 2 G and u + 1024 hold different templates (with S == 2 the units that carry chains do)
    slot = np.arange(U) // S
    for d in (G, 2 * G, W.SCAN):
        assert (w.slots[slot[:U - d]] != w.slots[slot[d:]]).all()
    # ... and so do most chains a grid apart
    aln, totals = W.wide_aln(w, te)
    for d in (G, 2 * G):
        assert (aln[:C_ - d] != aln[d:]).any(1).mean() > 0.95
    # a skipped chain in every round of 1024, in the batch and in the selection of all chains
    skipped = (aln[:, 5] & 4) != 0
    assert all(skipped[k:k + W.SCAN].any() for k in range(0, C_, W.SCAN)) and totals[1] == skipped.sum() > C_ // 60
    if S == 2:                                                       # the chain-carrying strand alternates: empty units between
        n = np.diff(b["chain_offsets"])
        assert (n[0::2] > 0).sum() > U // 6 and (n[1::2] > 0).sum() > U // 6 and (n == 0).sum() >= U // 2
        assert len(set(b["chains"][:, 6].tolist())) == 3


@pytest.mark.parametrize("S", (1, 2))
def test_the_templates_mix_what_shares_a_wave(S):
    T, w, te = _world(S)
    tb, prm = w.tb, W.PRM
    assert te["ties"] > 20, te["ties"]                               # the brute force alone: 24 (S = 1) and 23 (S = 2)
    per = np.diff(tb["chain_offsets"])
    assert set(per.tolist()) == {0, 1, 2, 3}
    gaps, ext, lone = [], set(), 0
    for u in range(per.size):
        lo, L = int(tb["offsets"][u]), len(AU.strand_read(tb["bases"], tb["read_offsets"], S, u))
        for c in range(int(tb["chain_offsets"][u]), int(tb["chain_offsets"][u + 1])):
            mem = AU.members_of(tb["rows"][lo:], tb["anchor_chain"][lo:], tb["anchor_pred"][lo:], tb["chains"][c, 7], c - int(tb["chain_offsets"][u]))
            lone += len(mem) == 1
            ext |= {mem[-1][0], L - (mem[0][0] + mem[0][1])}        # the rows of the left and right extension
            for (s1, l1, t1), (s0, l0, t0) in zip(mem, mem[1:]):
                gaps.append((s1 - (s0 + l0), t1 - (t0 + l0)))
    gaps = np.asarray(gaps)
    d = np.abs(gaps[:, 1] - gaps[:, 0])
    proper = (gaps[:, 0] > 0) & (gaps[:, 1] > 0)
    assert (proper & (d >= 390) & (d <= 400) & (gaps[:, 1] > gaps[:, 0])).sum() >= 8      # 8 chunks of diagonals, both ways
    assert (proper & (d >= 390) & (d <= 400) & (gaps[:, 1] < gaps[:, 0])).sum() >= 8
    assert (proper & (d == 0)).sum() >= 30                           # 2 chunks
    assert ((gaps[:, 0] == 0) & (gaps[:, 1] > 0)).sum() >= 10 and ((gaps[:, 1] == 0) & (gaps[:, 0] > 0)).sum() >= 10      # closed forms
    assert (d > prm.max_indel).sum() >= 8 and lone >= 30
    assert ext >= {0, 1, 64, 65, 130}
    aln = te["aln"]
    live = (aln[:, 5] & 4) == 0
    assert ((te["need"] == 0) & live).sum() >= 15                    # trivial chains: closed forms alone
    assert (aln[live, 6] < tb["chains"][live, 5]).sum() >= 10        # members dropped by trimming
    assert (tb["bases"] == 4).sum() >= 20                            # breaks
    assert len(set(aln[live, 5].tolist())) == 4                      # every pair of extension ends
    assert CU.check_result(tb, prm, T, aln, te["cigars"]) == live.sum()      # the members are true matches where they are used
    letters = {int(v) & 15 for o in te["ops"] for v in o}
    assert letters == {CU.OP_I, CU.OP_D, CU.OP_S, CU.OP_EQ, CU.OP_X}
    if S == 2:                                                       # the table matters: extensions stop at contig bounds
        other = AU.expected(tb, prm, T, None)[0]
        assert 5 <= (other != aln).any(1).sum() < aln.shape[0]


@pytest.mark.slow
@pytest.mark.parametrize("S", (1, 2))
def test_the_assembled_expectation_is_the_brute_force(S):
    """600 consecutive units of the wide batch, across the unit G: AU.expected and CU.expected run directly."""
    T, w, te = _world(S)
    lo = (G - 280) // S
    cut = w.cut(lo, lo + 600 // S)
    b = cut.b
    assert b["offsets"].size - 1 == 600
    first = int(w.b["chain_offsets"][lo * S])
    for k in ("bases", "rows", "chains"):                            # the slice is the wide batch's own units
        n = b[k].shape[0]
        at = {"bases": int(w.b["read_offsets"][lo]), "rows": int(w.b["offsets"][lo * S]), "chains": first}[k]
        assert np.array_equal(b[k], w.b[k][at:at + n])
    aln, totals, _ = AU.expected(b, W.PRM, T, SETS[S])
    C_ = aln.shape[0]
    assert C_ > 400
    got = W.wide_aln(cut, te)
    assert np.array_equal(got[0], aln) and np.array_equal(got[1], totals)
    assert np.array_equal(W.wide_aln(w, te)[0][first:first + C_], aln)
    for cap in (C_ - 1, 1):
        want = AU.expected(b, W.PRM, T, SETS[S], cap)
        got = W.wide_aln(cut, te, cap)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    full = CU.expected(b, W.PRM, T, aln, SETS[S])
    CU.agrees(W.wide_cigars(cut, te), full)
    assert full["totals"][1] >= 5 and full["totals"][2] > 10**6
    rng = np.random.default_rng(5)
    sel = rng.integers(0, C_, 300).tolist()
    sel[10:14] = [sel[9]] * 4
    sel[100:200] = list(range(C_ - 1, C_ - 101, -1))
    for k, v in ((0, -1), (50, C_), (51, 2**40), (250, -2**40), (299, C_ + 3)):
        sel[k] = v
    want = CU.expected(b, W.PRM, T, aln, SETS[S], sel)
    CU.agrees(W.wide_cigars(cut, te, sel), want)
    assert (want["info"][:, 1] == CU.BAD).sum() == 5 and (want["info"][:, 1] == CU.SKIPPED).sum() >= 3
    run = np.cumsum(want["need"])
    k = int(np.flatnonzero(want["need"] > 0)[80])
    for budget in (int(run[k]), int(run[k]) - 1):
        cutw = CU.expected(b, W.PRM, T, aln, SETS[S], sel, dir_bytes=budget)
        CU.agrees(W.wide_cigars(cut, te, sel, dir_bytes=budget), cutw)
        assert (cutw["info"][:, 1] & CU.NO_ROOM).any() and (cutw["info"][:, 1] == (CU.SKIPPED | CU.NO_ROOM)).any()
    ops = int(want["offsets"][-1])
    CU.agrees(W.wide_cigars(cut, te, sel, cap_ops=ops // 2), CU.expected(b, W.PRM, T, aln, SETS[S], sel, cap_ops=ops // 2))


def test_the_selection_of_three_rounds_and_five():
    T, w, te = _world(1)
    C_ = w.tchain.size
    needy = np.flatnonzero(te["need"][w.tchain] > 0)
    n = 3 * W.SCAN + 5
    at = (1022, 1023, 1024, 2047, 2048, n - 1)
    sel, bad = W.wide_selection(31, C_, n, needy, at)
    assert sel.size == n and {k // W.SCAN for k in bad} == {0, 1, 3} and (2**40 == sel).any() and (sel < 0).any()
    want = W.wide_cigars(w, te, sel)
    assert (want["need"][list(at)] > 0).all() and (want["info"][bad, 1] == CU.BAD).all()
    good = np.delete(sel, bad)
    assert np.unique(good).size < good.size and (np.diff(good) == -1).sum() > 1000      # repeats and reversed stretches
    assert (want["info"][:, 1] == CU.SKIPPED).sum() >= 10
    assert want["info"][bad, 0].tolist() == [int(np.int64(v).astype(np.int32)) for v in sel[bad]]


def test_the_chain_units_pass_their_thresholds():
    offs, rows, sizes, heavy = W.chain_units(41, G)
    U = offs.size - 1
    assert U == 2 * G + 300 and len(heavy) == 30 and rows.shape[0] > 256
    light = lambda u: sizes[u] <= 6      # noqa: E731
    hlh = [u for u in heavy if u < G and not light(u + 2 * G) and light(u + G)]
    lhl = [u for u in heavy if G <= u < 2 * G and light(u - G) and light(u + G)]
    assert len(hlh) == 10 and len(lhl) == 10
    assert {int(sizes[u]) for u in heavy} == set(W.HEAVY)
    rest = np.delete(sizes, heavy)
    assert rest.max() == 6 and 0.09 < (rest == 0).mean() < 0.16
    assert np.array_equal(np.diff(offs), sizes)
    ctg = CH.contig_of(W.TABLE_CHAINS, rows[:, 2].astype(np.int64) - 1)
    assert len(set(ctg.tolist())) >= 3
