"""GPU tests of genie_chain_cigars (run with -m gpu on an MI355X).  Every comparison is exact equality of cigar_offsets, cigar,
info, the direction needs and the totals with form (2) of the brute force of tests/cigar_util.py (checked against form (1) on the
host by tests/test_cigars_host.py), on the d_aln rows of the brute force of tests/align_util.py; the checks that hold whatever
the tie-breaks run on the device's output as well.  Synthetic chains at every size at which the kernels take another path: one
chunk of 64 diagonals or two with E runs across the border, one staging of 64 rows or several, 1024 diagonals, every kind of
extension end, both strands, breaks, trimmed and skipped members, skipped chains; the selection, the sizing call, a capacity
below the total, a direction budget below the need; a random batch through the device pipeline; SMEM.map_reads."""
import numpy as np
import pytest

import align_util as AU
import cigar_util as CU
import match_stats_util as MS

pytestmark = pytest.mark.gpu

P = AU.Params
D = AU.DEFAULTS
N_REF = 1 << 14
TABLE = np.asarray([0, 3000, 9000, N_REF], np.int64)


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
    e.T = np.random.default_rng(7).integers(0, 4, N_REF).astype(np.uint8)
    e.ix = g.GenieIndex.build(e.T, 0).to("cuda")
    return e


def _chain(rng, T, spec, left, right, lo=0, hi=None, rate=0.1, t0=None, overlap=0.0, dup=0.0):
    hi = len(T) if hi is None else hi
    span = sum(l + B for l, A, B in spec[:-1]) + spec[-1][0]
    if t0 is None:
        t0 = int(rng.integers(lo + left + 40, max(lo + left + 41, hi - span - right - 40)))
    Q, rows = AU.synth_chain(rng, T, t0, spec, left, right, rate)
    out = []
    for k, (s, e, pos) in enumerate(rows):
        if k + 1 < len(rows) and rng.random() < overlap:
            e = min(e + int(rng.integers(1, 6)), rows[k + 1][1] - 1, len(Q))
        if k and rng.random() < dup and s - 1 > rows[k - 1][0]:
            out.append((s - 1, min(s + 2, len(Q)), pos))            # the same reference position as the member behind it: skipped
        out.append((s, e, pos))
    return Q, out


def _run(env, units, prm, S=1, table=None, sel=None, **kw):
    """The call on the batch against the brute force, and the tie-break-free checks on what the device wrote."""
    b = AU.make_batch(units, S)
    aln = AU.expected(b, prm, env.T, table)[0]
    want = CU.expected(b, prm, env.T, aln, table, sel)
    got = CU.call(env.lib, env.ix, b, prm, aln, table, sel, **kw)
    CU.agrees(got, want)
    CU.check_result(b, prm, env.T, aln, got, sel)
    return b, aln, want, got


def _letters(res):
    return {int(v) & 15 for v in res["cigar"]}


@pytest.mark.parametrize("w,o", ((40, 6), (31, 6), (40, 0), (31, 0)))
def test_chunk_border_in_the_band(env, w, o):
    """2 w + 1 = 81 diagonals (two chunks, the second 17 lanes wide) and 63 (one chunk); gaps of about 70 x 70 with deletions
    and insertions, so that E runs cross the chunk border; o = 0: open and extend tie."""
    rng = np.random.default_rng(1000 + w + o)
    prm = P(1, 3, o, 1, w, 64, 3)
    units = []
    for A, B in ((70, 70), (70, 76), (76, 70), (64, 90), (90, 66), (71, 69), (40, 100), (100, 45)):
        if abs(B - A) > prm.max_indel:
            continue
        Q, rows = _chain(rng, env.T, [(12, A, B), (14, 0, 0)], 75, 80, rate=0.12)
        units.append((Q, [(rows, 0)]))
    b, aln, want, got = _run(env, units, prm)
    # o = 0 and e = 1: two one-base gaps (-2) beat a mismatch (-3), so no X is left
    assert want["totals"][0] == len(units) and _letters(want) >= ({CU.OP_I, CU.OP_D, CU.OP_EQ, CU.OP_X} if o else {CU.OP_I, CU.OP_D, CU.OP_EQ})
    runs = [int(v) >> 4 for v in want["cigar"] if int(v) & 15 == CU.OP_D]
    assert max(runs) >= 6                                           # an E run of some length
    assert want["need"].min() > 70 * (64 if w == 40 else 32)


def test_staging_border_in_the_rows(env):
    """Pieces of 63, 64, 65 and 130 rows (64 rows per staging): as gaps and as both extensions."""
    rng = np.random.default_rng(1100)
    prm = P(2, 3, 4, 1, 20, 30, 50)                                  # the bonus takes every extension to the end
    units = []
    for n in (63, 64, 65, 130, 1, 2):
        Q, rows = _chain(rng, env.T, [(10, n, n + int(rng.integers(-3, 4))), (9, 0, 0)], n, n, rate=0.08)
        units.append((Q, [(rows, 0)]))
    b, aln, want, got = _run(env, units, prm)
    assert (aln[:, 5] == 3).all() and want["totals"].tolist()[:2] == [6, 0]
    assert want["need"][0] >= 3 * 63 * 32 and want["need"][3] >= 3 * 130 * 32


def test_the_widest_band(env):
    """w = 100, max_indel = 823: a chain with a 300-base deletion (501 diagonals) and one whose gap is 823 bases longer in the
    reference: 1024 diagonals, sixteen chunks."""
    rng = np.random.default_rng(1200)
    prm = P(1, 4, 6, 1, 100, 823, 5)
    units = []
    for A, B in ((50, 350), (6, 829), (829, 6), (120, 130)):
        Q, rows = _chain(rng, env.T, [(20, A, B), (20, 0, 0)], 30, 30, rate=0.05)
        units.append((Q, [(rows, 0)]))
    b, aln, want, got = _run(env, units, prm)
    assert want["totals"][0] == 4
    assert want["need"][1] >= 6 * 16 * 32 and want["need"][2] >= 829 * 16 * 32
    assert max(int(v) >> 4 for v in want["cigar"] if int(v) & 15 == CU.OP_D) >= 290
    assert max(int(v) >> 4 for v in want["cigar"] if int(v) & 15 == CU.OP_I) >= 800


def test_extensions(env):
    """i* = 0 at both ends; a local end short of the read's end; to the end on a tie; an extension cut by the contig's end (B <
    A) and the left extension at the contig's start, on a 3-contig table."""
    rng = np.random.default_rng(1300)
    T = env.T
    sub = lambda v: (v + 1) & 3      # noqa: E731
    units = []
    units.append((T[5000:5040].copy(), [([(0, 40, 5001)], 1)]))                                   # i* = 0 twice
    junk = lambda n: rng.integers(0, 4, n).astype(np.uint8)      # noqa: E731
    # local at both ends: the read goes on with the complement of what the reference has there
    units.append((np.concatenate([3 - T[5070:5100], T[5100:5150], 3 - T[5150:5190]]), [([(30, 80, 5101)], 1)]))
    units.append((np.concatenate([T[5200:5229], [sub(T[5229])]]), [([(0, 20, 5201)], 1)]))        # G + end_bonus == M with bonus 4
    units.append((np.concatenate([[sub(T[5300])], T[5301:5330]]), [([(10, 30, 5311)], 1)]))       # ... and at the left end
    units.append((T[8950:9020].copy(), [([(0, 30, 8951)], 1)]))                                   # the contig ends after 20 more bases
    units.append((np.concatenate([junk(6), T[3000:3040]]), [([(16, 46, 3011)], 1)]))              # clo 10 bases in front of the member
    units.append((np.concatenate([T[2990:3000], T[3000:3040]]), [([(15, 50, 3006)], 1)]))         # the read runs on into contig 0
    Q, rows = _chain(rng, T, [(25, 3, 5), (25, 0, 0)], 60, 60, 9000, N_REF, rate=0.3)              # noisy ends
    units.append((Q, [(rows, 2)]))
    for bonus in (4, 3, 0):
        prm = D._replace(end_bonus=bonus, band=8)
        b, aln, want, got = _run(env, units, prm, table=TABLE)
        assert want["totals"].tolist()[:2] == [8, 0]
        texts = CU.cigar_strings(want["offsets"], want["cigar"])
        assert texts[0] == "40=" and want["need"][0] == 0
        assert texts[2] == ("29=1X" if bonus == 4 else "29=1S") and texts[3] == ("1X29=" if bonus == 4 else "1S29=")
        assert texts[1] == "30S50=40S" and texts[4].endswith("S") and aln[4, 4] <= 9001 and aln[5, 3] >= 3001 and aln[6, 3] >= 3001


def test_both_strands_breaks_overlaps_and_skipped_chains(env):
    rng = np.random.default_rng(1400)
    prm = D._replace(max_indel=20)
    units = []
    for r in range(24):
        g = int(rng.integers(0, 3))
        spec = [(int(rng.integers(8, 30)), int(rng.integers(0, 12)), int(rng.integers(0, 12))) for _ in range(int(rng.integers(1, 6)))]
        if r % 8 == 5:
            spec[0] = (spec[0][0], 4, 30)                            # |B - A| = 26 > max_indel: skipped
            spec.append((10, 0, 0))
        Q, rows = _chain(rng, env.T, spec, int(rng.integers(0, 50)), int(rng.integers(0, 50)), int(TABLE[g]), int(TABLE[g + 1]),
                         overlap=0.4, dup=0.3)
        if r % 3 == 0:                                               # breaks inside gaps and extensions (not inside members)
            free = [q for q in range(len(Q)) if not any(s <= q < e for s, e, _ in rows)]
            if free:
                Q = Q.copy()
                Q[rng.choice(free, min(3, len(free)), replace=False)] = 4
        if r % 2:
            units += [(AU.revcomp(Q), []), (Q, [(rows, g)])]         # the reverse strand carries the chain
        else:
            units += [(Q, [(rows, g)]), (AU.revcomp(Q), [])]
    b, aln, want, got = _run(env, units, prm, S=2, table=TABLE)
    assert want["totals"].tolist()[:2] == [21, 3] and (want["info"][:, 1] == CU.SKIPPED).sum() == 3
    assert (aln[:, 6] < b["chains"][:, 5]).sum() >= 3                # members skipped by trimming
    assert _letters(want) == {CU.OP_I, CU.OP_D, CU.OP_S, CU.OP_EQ, CU.OP_X}


@pytest.fixture(scope="module")
def mixed(env):
    """Twelve chains, some trivial, shared by the selection, capacity and budget tests: (b, aln, prm, full expectation)."""
    rng = np.random.default_rng(1500)
    prm = D
    units = []
    for r in range(12):
        if r in (0, 1, 7):                                           # trivial: one member, the whole read
            at = 4000 + 100 * r
            units.append((env.T[at:at + 50].copy(), [([(0, 50, at + 1)], 0)]))
            continue
        spec = [(int(rng.integers(8, 30)), int(rng.integers(1, 12)), int(rng.integers(1, 12))) for _ in range(int(rng.integers(2, 5)))]
        Q, rows = _chain(rng, env.T, spec, int(rng.integers(5, 50)), int(rng.integers(5, 50)))
        units.append((Q, [(rows, 0)]))
    b = AU.make_batch(units)
    aln = AU.expected(b, prm, env.T)[0]
    return b, aln, prm, CU.expected(b, prm, env.T, aln)


def test_selection(env, mixed):
    b, aln, prm, full = mixed
    CU.agrees(CU.call(env.lib, env.ix, b, prm, aln), full)          # NULL: every chain
    assert full["totals"].tolist()[:2] == [12, 0] and (full["need"][[0, 1, 7]] == 0).all() and (full["need"] > 0).sum() == 9
    for sel in ([11, 9, 8, 4, 2], [3, 3, 5, 3], [-1, 12, 6, 2**40, -2**40, 0], [], [7]):
        want = CU.expected(b, prm, env.T, aln, None, sel)
        got = CU.call(env.lib, env.ix, b, prm, aln, None, sel)
        CU.agrees(got, want)
        CU.check_result(b, prm, env.T, aln, got, None)
    rep = CU.call(env.lib, env.ix, b, prm, aln, None, [3, 3, 5, 3])
    texts = CU.cigar_strings(rep["offsets"], rep["cigar"])
    assert texts[0] == texts[1] == texts[3] != texts[2] and np.array_equal(rep["info"][0], rep["info"][3])
    bad = CU.call(env.lib, env.ix, b, prm, aln, None, [-1, 12, 6, 2**40, -2**40, 0])
    assert bad["info"][:, 1].tolist() == [16, 16, 0, 16, 16, 0] and bad["totals"].tolist()[:2] == [2, 4]
    assert bad["info"][:, 0].tolist()[:3] == [-1, 12, 6]
    none = CU.call(env.lib, env.ix, b, prm, aln, None, [])
    assert none["offsets"].tolist() == [0] and none["totals"].tolist() == [0, 0, 0]
    # a capacity of chains below the total: the chains behind it are bad indices
    want = CU.expected(b, prm, env.T, aln, None, [1, 4, 5], cap=5)
    CU.agrees(CU.call(env.lib, env.ix, b, prm, aln, None, [1, 4, 5], cap=5), want)
    assert want["info"][:, 1].tolist() == [0, 0, 16]
    CU.agrees(CU.call(env.lib, env.ix, b, prm, aln, None, None, cap=5), CU.expected(b, prm, env.T, aln, None, None, cap=5))
    # no unit at all
    empty = AU.make_batch([])
    got = CU.call(env.lib, env.ix, empty, prm, np.zeros((0, 8), np.int32))
    assert got["offsets"].tolist() == [0] and got["totals"].tolist() == [0, 0, 0]
    got = CU.call(env.lib, env.ix, empty, prm, np.zeros((0, 8), np.int32), None, [0, 5])
    assert got["info"][:, 1].tolist() == [16, 16] and got["offsets"].tolist() == [0, 0, 0]


def test_the_sizing_call_and_a_capacity_below_the_total(env, mixed):
    b, aln, prm, full = mixed
    total, need = int(full["offsets"][-1]), int(full["totals"][2])
    sized = CU.call(env.lib, env.ix, b, prm, aln, dir_bytes=need, sizing=True)
    assert sized["cigar"] is None
    CU.agrees(sized, full)
    for cap_ops in (total - 1, total // 2, 1, 0):
        got = CU.call(env.lib, env.ix, b, prm, aln, cap_ops=cap_ops, dir_bytes=need)      # call() checks nothing lies past cap_ops
        CU.agrees(got, dict(full, cigar=full["cigar"][:cap_ops]))
        assert got["offsets"][-1] == total
    CU.agrees(CU.call(env.lib, env.ix, b, prm, aln, cap_ops=total + 5, dir_bytes=need + 1000), full)


def test_the_direction_budget(env, mixed):
    b, aln, prm, full = mixed
    sel = [5, 0, 3, 7, 2, 1]
    want = CU.expected(b, prm, env.T, aln, None, sel)
    two = int(want["need"][:3].sum())                               # chain 0 is trivial: the first two that need room are 5 and 3
    assert want["need"][1] == 0 and want["need"][0] > 0 and want["need"][2] > 0
    # chain 7 behind them is trivial: the running sum through it is still the budget, so it is written too
    for budget, flags in ((two, [0, 0, 0, 0, 8, 8]), (two - 1, [0, 0, 8, 8, 8, 8]), (int(want["need"][0]), [0, 0, 8, 8, 8, 8]),
                          (int(want["need"].sum()), [0] * 6), (0, [8] * 6)):
        exp = CU.expected(b, prm, env.T, aln, None, sel, dir_bytes=budget)
        got = CU.call(env.lib, env.ix, b, prm, aln, None, sel, dir_bytes=budget)
        CU.agrees(got, exp)
        assert got["info"][:, 1].tolist() == flags, (budget, got["info"][:, 1])
        assert got["totals"][2] == got["need"].sum() == want["need"].sum()
    # dir_bytes = 0 with only trivial chains writes everything
    got = CU.call(env.lib, env.ix, b, prm, aln, None, [0, 1, 7, 1], dir_bytes=0)
    assert got["totals"].tolist() == [4, 0, 0] and CU.cigar_strings(got["offsets"], got["cigar"]) == ["50="] * 4


def _reads(ref, rng, count, lo, hi, rate):
    out = []
    for _ in range(count):
        L = int(rng.integers(lo, hi + 1))
        at = int(rng.integers(0, len(ref) - L - 40))
        r = AU.mutate(rng, ref[at:at + L + 40], rate).tolist()
        for _ in range(max(1, L // 100)):
            k = int(rng.integers(5, len(r) - 5))
            if rng.random() < 0.5:
                del r[k:k + int(rng.integers(1, 4))]
            else:
                r[k:k] = rng.integers(0, 4, int(rng.integers(1, 4))).tolist()
        r = np.asarray(r[:L], np.uint8)
        out.append(AU.revcomp(r) if rng.random() < 0.5 else r)
    return out


def test_a_random_batch_through_the_device_pipeline(env):
    """200 reads of 60 to 400 bases, 8 % substitutions and indels, both strands, 3 contigs, default parameters: find_mems_contigs,
    chain_mems, align_chains and chain_cigars on the device, the last two against the brute force."""
    import torch
    g, ix = env.g, env.ix
    rng = np.random.default_rng(1600)
    reads = _reads(env.T, rng, 200, 60, 400, 0.08)
    rs = g.ReferenceSet(["a", "b", "c"], TABLE, env.T)
    bases, roffs = MS.csr(reads)
    offs, rows, _, _ = ix.find_mems_contigs(rs, bases, roffs, 12, both_strands=True)
    chained = ix.chain_mems(offs, rows, rs, min_score=25)
    aln, _ = ix.align_chains((bases, roffs), offs, rows, chained, rs, True)
    host = lambda t: t.cpu().numpy()      # noqa: E731
    b = {"S": 2, "bases": np.asarray(bases), "read_offsets": np.asarray(roffs), "offsets": host(offs), "rows": host(rows),
         "anchor_chain": host(chained[2]), "anchor_pred": host(chained[3]), "chain_offsets": host(chained[0]), "chains": host(chained[1])}
    want_aln = AU.expected(b, D, env.T, TABLE)[0]
    assert np.array_equal(host(aln), want_aln) and want_aln.shape[0] >= 150
    want = CU.expected(b, D, env.T, want_aln, TABLE)
    co, cg, info = ix.chain_cigars((bases, roffs), offs, rows, chained, aln, None, rs, True)
    got = {"offsets": host(co), "cigar": host(cg.view(torch.int32)).view(np.uint32), "info": host(info), "need": None, "totals": None}
    CU.agrees(got, want)
    assert CU.check_result(b, D, env.T, want_aln, got) == want["totals"][0] >= 150
    assert _letters(want) == {CU.OP_I, CU.OP_D, CU.OP_S, CU.OP_EQ, CU.OP_X}
    # the hints: too small at first, the result is the same
    co2, cg2, info2 = ix.chain_cigars((bases, roffs), offs, rows, chained, aln, None, rs, True, ops_hint=3, dir_bytes_hint=100)
    assert np.array_equal(host(co2), host(co)) and np.array_equal(host(info2), host(info))
    assert np.array_equal(host(cg2.view(torch.int32)), host(cg.view(torch.int32)))
    assert g.cigar_strings(co, cg) == CU.cigar_strings(want["offsets"], want["cigar"])


def test_map_reads(env):
    """50 reads simulated from the 3-contig reference, half of them from the reverse strand: contig, offset and strand of every
    read come back, and the CIGAR of an unmutated read is "{L}="."""
    g = env.g
    rng = np.random.default_rng(1700)
    rs = g.ReferenceSet(["a", "b", "c"], TABLE, env.T)
    m = g.ExactMatch("map_reads.fa")
    m.set_reference("".join("ACGT"[c] for c in env.T))
    sm = g.SMEM(m, 4)
    reads, truth = [], []
    for r in range(50):
        L = int(rng.integers(80, 200))
        c = int(rng.integers(0, 3))
        at = int(rng.integers(int(TABLE[c]), int(TABLE[c + 1]) - L))
        q = env.T[at:at + L].copy()
        if r % 5 == 4:
            q = AU.mutate(rng, q, 0.04)
            q[:12], q[-12:] = env.T[at:at + 12], env.T[at + L - 12:at + L]      # the ends match: the alignment covers the read
        strand = r % 2
        reads.append(AU.revcomp(q) if strand else q)
        truth.append((strand, c, at - int(TABLE[c]) + 1, L, r % 5 == 4))
    strs = ["".join("ACGT"[c] for c in q) for q in reads]
    hits, offs, cigar = sm.map_reads(strs, 15, rs, min_score=25)
    hits, texts = hits.cpu().numpy(), g.cigar_strings(offs, cigar)
    assert hits.shape == (50, 6) and len(texts) == 50
    for (strand, c, off1, L, mutated), hit, text in zip(truth, hits, texts):
        assert hit[0] >= 0 and hit[1:4].tolist() == [strand, c, off1], (hit, strand, c, off1)
        if not mutated:
            assert text == f"{L}=" and hit[4] == L + 10 and hit[5] == 0
        else:
            assert "S" not in text and hit[5] == sum(int(n) for n, o in _ops(text) if o in "XID")
    # a read that maps nowhere
    hits2, offs2, cigar2 = sm.map_reads([strs[0], "ACGT" * 20, strs[1]], 15, rs, min_score=25)
    assert hits2.cpu().numpy()[1].tolist() == [-1, 0, -1, 0, 0, 0]
    assert g.cigar_strings(offs2, cigar2) == [texts[0], "", texts[1]]


def _ops(text):
    import re
    return re.findall(r"(\d+)([SIDX=])", text)
