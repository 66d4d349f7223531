"""GPU tests of genie_chain_mems (run with -m gpu on an MI355X).  Every comparison is exact, against the brute force of
tests/chain_util.py (checked against itself on the host by tests/test_chains_host.py): synthetic rows over every unit size at
which the kernels take another path (the wave width, the LDS ring of 512 anchors, candidates read back from the workspace),
the parameter grid, the sizing call and capacities, the rows genie_find_mems_contigs writes for repeat-rich and random
references under 1, 2 and 25 contigs, a read across a contig junction, one long read end to end, and the Python layer."""
import numpy as np
import pytest

import chain_util as CU
import contig_util as CT
import lookup_util as U
import match_stats_util as MS
import mems_util as MM

pytestmark = pytest.mark.gpu

P = CU.Params
N_REF = 1 << 16
TABLE = np.asarray([0, 9000, 9000, 30000, 30011, N_REF], np.int64)
BIG = (255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 2 * 4096 + 3, 20000)
SWEEP = P(1500, 200, 2, 0, 30)            # windows of about 1500 rows: candidates leave the ring of 512
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
    e.ix = g.GenieIndex.build(np.random.default_rng(7).integers(0, 4, N_REF).astype(np.uint8), 0).to("cuda")      # supplies only n
    return e


def _sweep():
    """The batch of every unit size, with its expected outputs under TABLE: computed once, never changed."""
    if "sweep" not in _CACHE:
        rng = np.random.default_rng(11)
        sizes = [0, 1, 20000, 0, 1] + list(range(131)) + list(BIG[:-1])
        offs, rows = CU.synth_batch(rng, sizes, N_REF)
        _CACHE["sweep"] = (offs, rows, CU.expected(offs, rows, SWEEP, TABLE))
    return _CACHE["sweep"]


def test_every_unit_size(env):
    offs, rows, want = _sweep()
    assert np.diff(offs).max() == 20000 and (np.diff(offs) == 0).sum() >= 3 and want["ties"] > 100
    assert want["chains"].shape[0] > 300 and want["totals"][1] > 300 and len(set(want["chains"][:, 6].tolist())) >= 3
    CU.agrees(CU.sized_call(env.lib, env.ix, offs, rows, SWEEP, TABLE), want)


def test_sizing_capacity_and_optional_outputs(env):
    offs, rows, want = _sweep()
    total = want["chains"].shape[0]
    for cap in (0, total - 1):
        got = CU.call(env.lib, env.ix, offs, rows, SWEEP, TABLE, cap=cap, spare=2)
        CU.agrees(got, want, cap)
        assert got["offsets"][-1] == total and (got["chains"][cap:] == -7).all()      # only the trailing chains are dropped
    for k in range(3):
        anchors = tuple(j != k for j in range(3))
        got = CU.call(env.lib, env.ix, offs, rows, SWEEP, TABLE, cap=total, anchors=anchors, totals=k != 1)
        assert got[("anchor_chain", "anchor_pred", "anchor_score")[k]] is None
        CU.agrees(got, want)
    got = CU.call(env.lib, env.ix, offs, rows, SWEEP, TABLE, chains=False, anchors=(False, False, False), totals=False)
    assert np.array_equal(got["offsets"], want["offsets"])
    # rows behind off[U] are no anchors: their elements stay as they were
    got = CU.call(env.lib, env.ix, offs[:40], rows, SWEEP, TABLE, cap=total)
    used = int(offs[39])
    for k in ("anchor_chain", "anchor_pred", "anchor_score"):
        assert np.array_equal(got[k][:used], want[k][:used]) and (got[k][used:] == -7).all()
    assert np.array_equal(got["offsets"], want["offsets"][:40])
    # no unit, and units without rows
    got = CU.call(env.lib, env.ix, [0], np.zeros((0, 4), np.int32), SWEEP, None, cap=3)
    assert got["offsets"].tolist() == [0] and got["totals"].tolist() == [0, 0] and (got["chains"] == -7).all()
    got = CU.call(env.lib, env.ix, [0, 0, 0], np.zeros((0, 4), np.int32), SWEEP, TABLE, cap=3)
    assert got["offsets"].tolist() == [0, 0, 0] and got["totals"].tolist() == [0, 0]


def _grid_batch():
    if "grid" not in _CACHE:
        rng = np.random.default_rng(12)
        offs, rows = CU.synth_batch(rng, [0, 1, 2, 17, 64, 65, 130], N_REF)
        # a unit of distinct starts, one base apart: max_pred (or max_dist) = 64 / 65 is a window of exactly 64 / 65 candidates,
        # and without a limit the window passes the ring of 512
        n = 700
        s = np.arange(n, dtype=np.int64) + 5
        t = s + 1000 + rng.integers(-1, 2, n)
        line = np.stack([s, s + rng.integers(1, 41, n), t + 1, np.zeros(n, np.int64)], 1).astype(np.int32)
        _CACHE["grid"] = (np.concatenate([offs, [offs[-1] + n]]), np.concatenate([rows, line]))
    return _CACHE["grid"]


@pytest.mark.parametrize("gap_cost", (0, 2, 255))
@pytest.mark.parametrize("max_dist", (1, 7, 300, 2**22))
def test_parameter_grid(env, max_dist, gap_cost):
    offs, rows = _grid_batch()
    links = 0
    for bandwidth in (0, min(5, max_dist), max_dist):
        for max_pred in (0, 1, 63, 64, 65, 5000):
            fp = None
            for min_score in (0, 40, 10**6):
                prm = P(max_dist, bandwidth, gap_cost, max_pred, min_score)
                want = CU.expected(offs, rows, prm, None if max_pred == 1 else TABLE)
                assert fp is None or np.array_equal(fp, want["anchor_pred"])
                fp = want["anchor_pred"]
                CU.agrees(CU.call(env.lib, env.ix, offs, rows, prm, None if max_pred == 1 else TABLE, cap=want["chains"].shape[0]), want)
            links += int((fp >= 0).sum())
    if max_dist >= 7:
        assert links > 1000


# ------------------------------------------------------------------ the rows genie_find_mems_contigs writes
def _reads(ref, seed, count=4, L=200):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        at = int(rng.integers(0, len(ref) - L))
        r = ref[at:at + L].copy()
        hit = rng.random(L) < 0.03
        r[hit] = (r[hit] + rng.integers(1, 4, int(hit.sum()))) & 3
        out.append(r.astype(np.uint8))
    return out


def _real_index(env, name):
    if ("ix", name) not in _CACHE:
        _CACHE["ix", name] = env.g.GenieIndex.build(FAMILY[name], 0, dir_bits=7).to("cuda")
    return _CACHE["ix", name]


@pytest.mark.parametrize("n_contigs", (1, 2, 25))
@pytest.mark.parametrize("name", ("rand4096", "tandem3", "tandem7"))
def test_real_rows(env, name, n_contigs):
    ref = FAMILY[name]
    ix = _real_index(env, name)
    table = np.linspace(0, len(ref), n_contigs + 1).astype(np.int64)
    bases, roffs = MS.csr(_reads(ref, 21, count={"rand4096": 4, "tandem3": 2, "tandem7": 3}[name]))
    prm = P(300, 50, 2, 0, 25)                                       # no max_pred: a start of a tandem read has hundreds of rows
    ties = chains = 0
    for flags in CT.FLAGS:
        offs, rows, _, _ = CT.sized_call(env.lib, ix, table, flags, bases, roffs, 12 if name == "rand4096" else 15)
        assert rows.shape[0] > 8
        want = CU.expected(offs, rows, prm, table)
        CU.agrees(CU.sized_call(env.lib, ix, offs, rows, prm, table), want)
        if n_contigs == 1:                                          # one contig is no table
            CU.agrees(CU.call(env.lib, ix, offs, rows, prm, None, cap=want["chains"].shape[0]), want)
        ties, chains = ties + want["ties"], chains + want["chains"].shape[0]
    assert chains > 0
    if name == "tandem7":
        assert ties >= 1000, ties                                    # the tie rule cannot go untested


def test_a_read_across_a_contig_junction(env):
    ref = FAMILY["rand4096"]
    ix = _real_index(env, "rand4096")
    table = np.asarray([0, 2048, 4096], np.int64)
    read = ref[1900:2200].copy()
    read[[40, 90, 200, 260]] ^= 1
    bases, roffs = MS.csr([read])
    offs, rows, _, _ = CT.sized_call(env.lib, ix, table, 0, bases, roffs, 12)
    prm = P(5000, 500, 2, 0, 0)
    side = CU.contig_of(table, rows[:, 2].astype(np.int64) - 1)
    assert set(side.tolist()) == {0, 1}
    for tab, mixed in ((table, False), (None, True)):
        got = CU.sized_call(env.lib, ix, offs, rows, prm, tab)
        CU.agrees(got, CU.expected(offs, rows, prm, tab))
        per_chain = [set(side[got["anchor_chain"] == c].tolist()) for c in range(int(got["offsets"][-1]))]
        assert any(len(s) == 2 for s in per_chain) == mixed
        assert not mixed or max(got["chains"][:, 5]) >= 4


# ------------------------------------------------------------------ one long read, end to end, through the Python layer
ORIGIN, SANE_SEED = 1000, 4


def sane_read():
    """2000 bases cut from rand4096 at ORIGIN, one 30-base deletion behind the first 1000, 2 % substitutions."""
    ref = FAMILY["rand4096"]
    rng = np.random.default_rng(SANE_SEED)
    read = np.concatenate([ref[ORIGIN:ORIGIN + 1000], ref[ORIGIN + 1030:ORIGIN + 2030]]).copy()
    hit = rng.random(read.size) < 0.02
    read[hit] = (read[hit] + rng.integers(1, 4, int(hit.sum()))) & 3
    return read.astype(np.uint8)


def check_sane(chains):
    best = chains[np.lexsort((chains[:, 7], -chains[:, 4]))[0]]
    assert best[1] - best[0] >= 1800 and best[5] >= 2
    assert best[2] <= ORIGIN + 1 < best[3] and best[3] <= ORIGIN + 2030 + 1
    return best


def test_end_to_end_sanity(env):
    ix = _real_index(env, "rand4096")
    read = sane_read()
    offs, rows, st, _ = ix.find_mems(read, np.asarray([0, read.size]), 12)
    co, chains, ac, ap, asc, dropped = ix.chain_mems(offs, rows)
    want = CU.expected(offs.cpu().numpy(), rows.cpu().numpy(), CU.DEFAULTS)
    assert np.array_equal(chains.cpu().numpy(), want["chains"]) and dropped == want["totals"][1]
    best = check_sane(chains.cpu().numpy())
    # the reverse complement of the read, both strands: strand 1 is the read itself
    offs2, rows2, _, _ = ix.find_mems(MS.rc(read), np.asarray([0, read.size]), 12, both_strands=True)
    co2, chains2, *_ = ix.chain_mems(offs2, rows2)
    strand1 = chains2[int(co2[1]):int(co2[2])].cpu().numpy()
    assert np.array_equal(strand1, chains.cpu().numpy()) and np.array_equal(check_sane(strand1), best)


def test_python_layer(env):
    g = env.g
    ref = FAMILY["tandem7"]
    ix = _real_index(env, "tandem7")
    reads = _reads(ref, 31, count=6, L=150)
    bases, roffs = MS.csr(reads)
    offs, rows, _, _ = ix.find_mems(bases, roffs, 15, both_strands=True)
    opts = dict(max_dist=300, bandwidth=50, gap_cost=2, max_pred=64, min_score=25)
    plain = ix.chain_mems(offs, rows, **opts)
    want = CU.expected(offs.cpu().numpy(), rows.cpu().numpy(), P(**opts))
    got = {"offsets": plain[0].cpu().numpy(), "chains": plain[1].cpu().numpy(), "anchor_chain": plain[2].cpu().numpy(),
           "anchor_pred": plain[3].cpu().numpy(), "anchor_score": plain[4].cpu().numpy(), "totals": np.asarray([plain[1].shape[0], plain[5]])}
    CU.agrees(got, want)
    assert want["chains"].shape[0] > 20
    # by_score: a permutation inside every unit, (score descending, last ascending), anchor_chain renumbered with it
    ranked = ix.chain_mems(offs, rows, by_score=True, **opts)
    co, a, b = plain[0].cpu().numpy(), plain[1].cpu().numpy(), ranked[1].cpu().numpy()
    assert np.array_equal(ranked[0].cpu().numpy(), co) and ranked[5] == plain[5]
    moved = 0
    ac0, ac1, ro = plain[2].cpu().numpy(), ranked[2].cpu().numpy(), offs.cpu().numpy()
    for u in range(co.size - 1):
        x, y = a[co[u]:co[u + 1]], b[co[u]:co[u + 1]]
        order = np.lexsort((x[:, 7], -x[:, 4].astype(np.int64)))
        assert np.array_equal(y, x[order])
        moved += int((order != np.arange(len(order))).any())
        rank = np.empty(len(order), np.int64)
        rank[order] = np.arange(len(order))
        old = ac0[ro[u]:ro[u + 1]]
        assert np.array_equal(ac1[ro[u]:ro[u + 1]], np.where(old >= 0, rank[np.maximum(old, 0)] if len(rank) else old, -1))
    assert moved > 0
    for k in (3, 4):
        assert np.array_equal(ranked[k].cpu().numpy(), plain[k].cpu().numpy())
    # SMEM.chain_mems and SMEM.find_chains: find_mems[_contigs] followed by chain_mems
    m = g.ExactMatch("find_chains.fa")
    m.set_reference("".join("ACGT"[c] for c in ref))
    sm = g.SMEM(m, 4)
    strs = ["".join("ACGT"[c] for c in r) for r in reads]
    mems, chained = sm.find_chains(strs, 15, both_strands=True, **opts)
    assert np.array_equal(mems[0].cpu().numpy(), offs.cpu().numpy()) and np.array_equal(mems[1].cpu().numpy(), rows.cpu().numpy())
    again = sm.chain_mems(mems[0], mems[1], **opts)
    for x, y, z in zip(chained[:5], plain[:5], again[:5]):
        assert np.array_equal(x.cpu().numpy(), y.cpu().numpy()) and np.array_equal(z.cpu().numpy(), y.cpu().numpy())
    assert chained[5] == plain[5] == again[5]
    # with a ReferenceSet the rows are genie_find_mems_contigs's and the chains stay inside one contig
    table = np.linspace(0, len(ref), 26).astype(np.int64)
    rs = g.ReferenceSet([str(i) for i in range(25)], table, ref)
    mems, chained = sm.find_chains(strs, 15, contigs=rs, both_strands=True, **opts)
    want = CU.expected(mems[0].cpu().numpy(), mems[1].cpu().numpy(), P(**opts), table)
    assert np.array_equal(chained[1].cpu().numpy(), want["chains"]) and np.array_equal(chained[2].cpu().numpy(), want["anchor_chain"])
    assert len(set(want["chains"][:, 6].tolist())) > 3
