"""GPU tests of genie_align_chains (run with -m gpu on an MI355X).  Every comparison is exact, against form (2) of the brute
force of tests/align_util.py (checked against form (1) on the host by tests/test_align_host.py): synthetic chains over every
band width, diagonal count, gap shape, extension length and chain length at which the kernel takes another path (one chunk of
64 diagonals or several, one staging of 64 rows or several, the closed forms for one-sided gaps), overlapping and skipped
members, skipped chains, units without chains, a capacity below the total, both strands and a contig table; the parameter
grid; the rows and chains the device pipeline writes for random and repeat-rich references; and the Python layer."""
import numpy as np
import pytest

import align_util as AU
import lookup_util as U
import match_stats_util as MS

pytestmark = pytest.mark.gpu

P = AU.Params
N_REF = 1 << 14
TABLE = np.asarray([0, 3000, 3000, 9000, 9040, N_REF], np.int64)
FAMILY = U.family()
_CACHE = {}


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


def _chain(rng, T, spec, left, right, lo=0, hi=None, rate=0.1, overlap=0.0, dup=0.0, t0=None):
    """A strand-read with one chain inside the reference window [lo, hi): AU.synth_chain, then some members made longer so that
    they overlap the next one (trimmed), and some rows put in that start where the next member starts in the reference (skipped)."""
    hi = len(T) if hi is None else hi
    span = sum(l + B for l, A, B in spec[:-1]) + spec[-1][0]
    if t0 is None:
        t0 = int(rng.integers(lo, max(lo + 1, hi - span)))
    Q, rows = AU.synth_chain(rng, T, t0, spec, left, right, rate)
    out = []
    for k, (s, e, pos) in enumerate(rows):
        if k + 1 < len(rows) and rng.random() < overlap:
            e = min(e + int(rng.integers(1, 6)), rows[k + 1][1] - 1, len(Q))
        if k and rng.random() < dup and s - 1 > rows[k - 1][0]:
            out.append((s - 1, min(s + 2, len(Q)), pos))                        # the same reference position as the member behind it
        out.append((s, e, pos))
    return Q, out


def _check(env, units, prm, S=1, table=None, cap=None, spare=0, floor=None):
    b = AU.make_batch(units, S)
    want = AU.expected(b, prm, env.T, table, cap)
    AU.agrees(AU.call(env.lib, env.ix, b, prm, table, cap=cap, spare=spare), want)
    return b, want


GAPS = [(0, 1), (1, 0), (1, 1), (2, 1), (1, 2), (2, 2), (0, 63), (63, 0), (63, 64), (64, 64), (65, 63), (64, 0), (0, 65), (200, 200),
        (200, 190), (65, 1), (2, 64)]


@pytest.mark.parametrize("w", (0, 1, 31, 32, 33, 100, 511))
def test_band_widths_gap_shapes_and_extension_lengths(env, w):
    rng = np.random.default_rng(100 + w)
    prm = P(1, 1, 1, 1, w, min(64, 1023 - 2 * w), 2)
    units, ties = [], 0
    ext = [0, 1, 63, 64, 65, 300]
    for k, (A, B) in enumerate(GAPS):
        if abs(B - A) > prm.max_indel:
            continue
        Q, rows = _chain(rng, env.T, [(int(rng.integers(1, 30)), A, B), (int(rng.integers(1, 30)), 0, 0)], ext[k % 6], ext[(k // 2 + 1) % 6])
        units.append((Q, [(rows, 0)]))
    for left in ext:                                                 # every pair of extension lengths, at both ends of the reference
        for right in ext:
            t0 = 10 if (left + right) % 2 else None
            Q, rows = _chain(rng, env.T, [(20, 0, 0)], left, right, t0=t0, rate=0.2)
            units.append((Q, [(rows, 0)]))
        Q, rows = _chain(rng, env.T, [(20, 0, 0)], left, 65, t0=N_REF - 20 - 30, rate=0.2)
        units.append((Q, [(rows, 0)]))
    b, want = _check(env, units, prm)
    assert want[1][0] == len(units) and want[2] > 4, want[2]           # ties: the brute force alone counts 6 to 15 per width
    assert len(set(want[0][:, 5].tolist())) >= 3


@pytest.mark.parametrize("w,d", ((31, 1), (32, 0), (63, 1), (64, 0), (63, -1), (500, 23), (500, -23), (0, 1023), (0, -1023), (5, 1013)))
def test_diagonal_counts(env, w, d):
    """2 w + |B - A| + 1 = 64, 65, 128, 129 and exactly 1024 diagonals."""
    rng = np.random.default_rng(200 + w)
    assert 2 * w + abs(d) + 1 in (64, 65, 128, 129, 1024)
    prm = P(2, 3, 2, 1, w, abs(d), 3)
    units = []
    for A in (1, 30, 70):
        B = A + d if d >= 0 else A
        A = A if d >= 0 else A - d
        Q, rows = _chain(rng, env.T, [(15, A, B), (12, 0, 0)], 5, 7)
        units.append((Q, [(rows, 0)]))
    b, want = _check(env, units, prm)
    assert want[1].tolist() == [3, 0]


def test_chain_lengths_overlaps_skips_and_capacity(env):
    rng = np.random.default_rng(300)
    prm = P(1, 2, 2, 1, 8, 6, 1)
    units = []
    for n in (1, 2, 64, 65, 600, 3, 0, 130):
        chains = []
        Qs = []
        for c in range(0 if n == 0 else (3 if n == 3 else 1)):
            spec = [(int(rng.integers(4, 12)), int(rng.integers(0, 4)), int(rng.integers(0, 4))) for _ in range(n)]
            if n == 130:
                spec[40] = (9, 2, 12)                                # |B - A| = 10 > max_indel: the chain is skipped
            Q, rows = _chain(rng, env.T, spec, 9, 11, overlap=0.3, dup=0.2)
            chains.append((rows, 0))
            Qs.append(Q)
        if not Qs:
            units.append((rng.integers(0, 4, 30).astype(np.uint8), []))
            continue
        # the chains of one unit share the strand-read: the members of the second and third are moved behind the first's read
        Q, shift, moved = np.concatenate(Qs), 0, []
        for (rows, g), q in zip(chains, Qs):
            moved.append(([(s + shift, e + shift, pos) for s, e, pos in rows], g))
            shift += len(q)
        units.append((Q, moved))
    b, want = _check(env, units, prm)
    total = want[0].shape[0]
    assert total == 9 and want[1].tolist() == [8, 1]
    used = want[0][:, 6]
    assert used.max() >= 500 and (used < np.asarray([c[5] for c in b["chains"]])).sum() >= 4      # members skipped by trimming
    # a capacity below the total: the rows behind it stay untouched
    for cap in (0, 1, total - 1):
        AU.agrees(AU.call(env.lib, env.ix, b, prm, cap=cap, spare=3), AU.expected(b, prm, env.T, None, cap))
    assert AU.call(env.lib, env.ix, b, prm, totals=False)[1] is None
    # no unit at all
    none = AU.make_batch([])
    got = AU.call(env.lib, env.ix, none, prm, cap=0, spare=2)
    assert (got[0] == -7).all() and got[1].tolist() == [0, 0]


def test_both_strands_breaks_and_a_contig_table(env):
    rng = np.random.default_rng(400)
    prm = P(1, 4, 6, 1, 32, 64, 5)
    units = []
    for r in range(40):
        g = int(rng.choice([0, 2, 3, 4]))
        clo, chi = int(TABLE[g]), int(TABLE[g + 1])
        spec = [(int(rng.integers(3, 9)), 0, 0)] if g == 3 else [(int(rng.integers(8, 30)), int(rng.integers(0, 9)), int(rng.integers(0, 9)))
                                                              for _ in range(int(rng.integers(1, 5)))]
        near = rng.random() < 0.4                                    # next to the contig's start: the left extension is clipped
        Q, rows = _chain(rng, env.T, spec, int(rng.integers(0, 50)), int(rng.integers(0, 50)), clo, chi, t0=clo + 3 if near else None)
        if r % 3 == 0:
            Q = Q.copy()
            Q[rng.integers(0, len(Q), 2)] = 4                        # breaks, also inside members: the members' score is a l' all the same
        if r % 2:
            units += [(AU.revcomp(Q), []), (Q, [(rows, g)])]
        else:
            units += [(Q, [(rows, g)]), (AU.revcomp(Q), [])]
    b, want = _check(env, units, prm, S=2, table=TABLE)
    assert want[0].shape[0] == 40 and len(set(want[0][:, 5].tolist())) == 4 and want[2] > 0
    got = AU.call(env.lib, env.ix, b, prm, TABLE, flags=AU.SPLIT)     # accepted, changes nothing
    AU.agrees(got, want)
    # without the table the extensions run on across the contig bounds
    other = AU.expected(b, prm, env.T, None)
    AU.agrees(AU.call(env.lib, env.ix, b, prm, None), other)
    assert not np.array_equal(other[0], want[0])


@pytest.mark.parametrize("a,b_,o,e,bonus", ((1, 4, 6, 1, 5), (1, 4, 0, 1, 5), (2, 0, 3, 2, 0), (5, 7, 1, 3, 20), (64, 64, 64, 64, 32768),
                                            (1, 1, 0, 1, 0), (3, 2, 6, 1, 1)))
def test_parameter_grid(env, a, b_, o, e, bonus):
    if "grid" not in _CACHE:
        rng = np.random.default_rng(500)
        units = []
        for k in range(24):
            spec = [(int(rng.integers(2, 20)), int(rng.integers(0, 12)), int(rng.integers(0, 12))) for _ in range(int(rng.integers(1, 6)))]
            if k % 4 == 0:
                spec = [(l, 1, 1) for l, _, _ in spec]               # one-base gaps: with o == 0 two gaps beat a mismatch
            Q, rows = _chain(rng, env.T, spec, int(rng.integers(0, 40)), int(rng.integers(0, 40)), rate=0.25, overlap=0.2)
            units.append((Q, [(rows, 0)]))
        _CACHE["grid"] = units
    ties = 0
    for w in (0, 2, 40):
        b, want = _check(env, _CACHE["grid"], P(a, b_, o, e, w, 16, bonus))
        assert want[1][0] >= 20
        ties += want[2]
    assert ties >= (100 if (a, b_, o, e, bonus) == (1, 1, 0, 1, 0) else 5)      # the brute force alone: 116, and 5 at the least


# ------------------------------------------------------------------ the rows and chains the device pipeline writes
def _reads(ref, seed, count, L, indels=True):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        at = int(rng.integers(0, len(ref) - L - 20))
        r = AU.mutate(rng, ref[at:at + L + 20], 0.04).tolist()
        for _ in range(3 if indels else 0):
            k = int(rng.integers(5, len(r) - 5))
            if rng.random() < 0.5:
                del r[k:k + int(rng.integers(1, 4))]
            else:
                r[k:k] = rng.integers(0, 4, int(rng.integers(1, 4))).tolist()
        out.append(np.asarray(r[:L], np.uint8))
    return out


def _real_index(env, name):
    if ("ix", name) not in _CACHE:
        _CACHE["ix", name] = env.g.GenieIndex.build(FAMILY[name], 0, dir_bits=7).to("cuda")
    return _CACHE["ix", name]


def _pipeline(env, ix, ref, table, reads, min_len, both, split, chain_opts, prm):
    """find_mems_contigs -> chain_mems -> align_chains on the device, the last against the brute force."""
    rs = env.g.ReferenceSet([str(i) for i in range(len(table) - 1)], table, ref)
    bases, roffs = MS.csr(reads)
    offs, rows, _, _ = ix.find_mems_contigs(rs, bases, roffs, min_len, both_strands=both, split_breaks=split)
    chained = ix.chain_mems(offs, rows, rs, **chain_opts)
    aln, totals = ix.align_chains((bases, roffs), offs, rows, chained, rs, both, **prm._asdict())
    host = lambda t: t.cpu().numpy()      # noqa: E731
    b = {"S": 2 if both else 1, "bases": np.asarray(bases), "read_offsets": np.asarray(roffs), "offsets": host(offs), "rows": host(rows),
         "anchor_chain": host(chained[2]), "anchor_pred": host(chained[3]), "chain_offsets": host(chained[0]), "chains": host(chained[1])}
    want = AU.expected(b, prm, ref, table)
    assert np.array_equal(host(aln), want[0]) and list(totals) == want[1].tolist()
    return b, want


@pytest.mark.parametrize("n_contigs", (1, 2, 25))
@pytest.mark.parametrize("name", ("rand4096", "tandem7"))
def test_real_pipeline(env, name, n_contigs):
    ref = FAMILY[name]
    ix = _real_index(env, name)
    table = np.linspace(0, len(ref), n_contigs + 1).astype(np.int64)
    reads = _reads(ref, 21, 4 if name == "rand4096" else 1, 150)      # a tandem read has hundreds of chains
    reads.append(ref[int(table[1]) - 100:int(table[1])].copy())      # a read that ends where its contig ends ...
    reads.append(ref[5:120].copy())                                  # ... and one next to the reference's start
    broken = reads[0].copy()
    broken[[30, 31, 90]] = 4
    reads.append(broken)
    chain_opts = dict(max_dist=300, bandwidth=50, gap_cost=2, max_pred=64, min_score=25)
    b, want = _pipeline(env, ix, ref, table, reads, 12 if name == "rand4096" else 15, True, True, chain_opts, AU.DEFAULTS)
    aln = want[0]
    assert aln.shape[0] >= len(reads) and want[1][1] == 0
    if name == "rand4096":
        exact = (aln[:, 0] == 100 + 10) & (aln[:, 5] == 3) & (aln[:, 1] == 0) & (aln[:, 2] == 100)
        assert exact.any() and aln[exact][0, 4] == table[1] + 1      # the exact read ends where its contig ends
        assert ((aln[:, 5] & 3) == 3).sum() >= 2                     # the two exact reads at the least
        assert (aln[:, 6] >= 2).sum() >= 1


def test_one_long_read_end_to_end(env):
    ref = np.concatenate([FAMILY["rand4096"]] + [np.random.default_rng(40 + k).integers(0, 4, 4096).astype(np.uint8) for k in range(3)])
    ix = env.g.GenieIndex.build(ref, 0, dir_bits=7).to("cuda")
    read = _reads(ref[2000:], 41, 1, 10**4)[0]
    chain_opts = dict(max_dist=1000, bandwidth=100, gap_cost=2, max_pred=50, min_score=200)
    b, want = _pipeline(env, ix, ref, np.asarray([0, len(ref)], np.int64), [read], 14, False, False, chain_opts, AU.DEFAULTS)
    best = want[0][np.argmax(want[0][:, 0])]
    assert best[2] - best[1] >= 9900 and best[6] >= 100 and best[0] > 5000


def test_python_layer(env):
    g = env.g
    ref = FAMILY["tandem7"]
    ix = _real_index(env, "tandem7")
    reads = _reads(ref, 31, 2, 60, indels=False)                     # a tandem read has hundreds of chains: two short ones do
    strs = ["".join("ACGT"[c] for c in r) for r in reads]
    m = g.ExactMatch("find_alignments.fa")
    m.set_reference("".join("ACGT"[c] for c in ref))
    sm = g.SMEM(m, 4)
    opts = dict(max_dist=300, bandwidth=50, gap_cost=2, max_pred=64, min_score=25)
    al = dict(match=2, mismatch=3, gap_open=4, gap_extend=1, band=16, max_indel=40, end_bonus=3)
    mems, chains, aln = sm.find_alignments(strs, 15, both_strands=True, align_options=al, **opts)
    plain = ix.chain_mems(mems[0], mems[1], **opts)
    for x, y in zip(chains[:5], plain[:5]):
        assert np.array_equal(x.cpu().numpy(), y.cpu().numpy())
    host = lambda t: t.cpu().numpy()      # noqa: E731
    bases, roffs = MS.csr(reads)
    b = {"S": 2, "bases": np.asarray(bases), "read_offsets": np.asarray(roffs), "offsets": host(mems[0]), "rows": host(mems[1]),
         "anchor_chain": host(plain[2]), "anchor_pred": host(plain[3]), "chain_offsets": host(plain[0]), "chains": host(plain[1])}
    want = AU.expected(b, P(**al), ref)
    assert want[0].shape[0] > 20 and np.array_equal(host(aln), want[0])
    again, totals = sm.align_chains(strs, mems[0], mems[1], plain, both_strands=True, **al)
    assert np.array_equal(host(again), want[0]) and list(totals) == want[1].tolist()
    # by_score: chains and aln come in chain_mems' by_score order, anchor_chain renumbered with it
    ranked = ix.chain_mems(mems[0], mems[1], by_score=True, **opts)
    mems2, chains2, aln2 = sm.find_alignments(strs, 15, both_strands=True, align_options=al, by_score=True, **opts)
    for x, y in zip(chains2[:5], ranked[:5]):
        assert np.array_equal(host(x), host(y))
    co, a0, a1, c0, c1 = host(plain[0]), host(aln), host(aln2), host(plain[1]), host(ranked[1])
    moved = 0
    for u in range(co.size - 1):
        order = np.lexsort((c0[co[u]:co[u + 1], 7], -c0[co[u]:co[u + 1], 4].astype(np.int64)))
        assert np.array_equal(c1[co[u]:co[u + 1]], c0[co[u]:co[u + 1]][order]) and np.array_equal(a1[co[u]:co[u + 1]], a0[co[u]:co[u + 1]][order])
        moved += int((order != np.arange(len(order))).any())
    assert moved > 0
    # the defaults are the wrapper's
    d_aln, _ = ix.align_chains((bases, roffs), mems[0], mems[1], plain, both_strands=True)
    e_aln, _ = ix.align_chains((bases, roffs), mems[0], mems[1], plain, both_strands=True, **AU.DEFAULTS._asdict())
    assert np.array_equal(host(d_aln), host(e_aln)) and not np.array_equal(host(d_aln), want[0])
