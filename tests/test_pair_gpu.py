"""GPU: genie_pair_alignments against the brute force of tests/pair_util.py, every output exactly equal.  Synthetic records,
class rows and offsets exercise the call without the pipeline in front of it: record counts of the two mates on both sides of
the lane / wave border, of the wave's 64 lanes and of the LDS tile, scores from a range of two so that ties decide, every
orientation mask and the ends of every parameter's range, n_records cutting a pair in two, cap_chains == 0, more narrow pairs
than one grid of lanes and more wide pairs than one grid of waves.  Then the pipeline on the 16 kb reference with the planted
300-base duplication of tests/test_select_gpu.py: a mate inside the duplication is placed next to its unique mate, mates 5 kb
apart stay unpaired, a pair with one random mate is half mapped; each expectation is computed by the CPU brute forces before
the GPU is asked."""
import numpy as np
import pytest

import align_util as AU
import pair_util as PU
import select_util as SU

pytestmark = pytest.mark.gpu

P = PU.Params
D = PU.DEFAULTS
N_REF = 1 << 14
TABLE = np.asarray([0, 6000, 12000, N_REF], np.int64)
SETS = (D, P(7, 0, 1000, 300, 8, 16, 17, 40), P(2, 100, 700, 0, 300, 40, 0, 60), P(5, 0, 1 << 30, 500, 1, 5, 30, 0))
BORDERS = [(0, 0), (0, 1), (1, 0), (1, 1), (1, 6), (6, 6), (8, 8), (8, 9), (1, 64), (1, 65), (64, 64), (300, 2), (2, 300), (0, 300)]


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import genie_smem_amd as g

    class Env:
        pass
    e = Env()
    e.g, e.lib = g, g._native.lib()
    T = np.random.default_rng(50).integers(0, 4, N_REF).astype(np.uint8)
    T[9000:9300] = T[2000:2300]                                     # two exact copies of a 300-base segment
    e.T = T
    e.ix = g.GenieIndex.build(T, 0).to("cuda")
    return e


def _exact(env, b, prm, **kw):
    want = PU.expected(b, prm, kw.get("n_records"), kw.get("cap"))
    got = PU.call(env.lib, env.ix, b, prm, **kw)
    PU.agrees(got, want)
    return got, want


@pytest.mark.parametrize("scores", [(60, 90), (60, 62)], ids=["scores", "ties"])
def test_record_counts_around_the_borders(env, scores):
    assert env.g._native.PAIR_LANE_MAX == PU.LANE_MAX == 64 and env.g._native.PAIR_TILE == PU.TILE == 256
    rng = np.random.default_rng(71 + scores[1])
    b = PU.random_batch(rng, BORDERS, scores=scores)
    seen = 0
    for prm in SETS:
        got, want = _exact(env, b, prm)
        seen |= int(np.bitwise_or.reduce(want["pairs"][:, 2]))
    w = PU.expected(b, SETS[1])["pairs"]
    wide = [BORDERS.index(c) for c in ((8, 9), (1, 65), (64, 64), (300, 2), (2, 300))]
    assert seen == 31 and w[BORDERS.index((300, 2)), 6] > 64 and (w[wide, 2] & 1).any() and (w[wide, 2] & 24).any()
    if scores[1] - scores[0] == 2:                                  # ties: a best value shared by two combinations
        assert ((w[:, 3] == w[:, 4]) & (w[:, 6] > 1)).sum() >= 2


def test_candidates_past_the_tile_win(env):
    # the only concordant combination of each pair uses the LAST record of the long mate, beyond the LDS tile
    reads = []
    for long_first in (True, False):
        head = (0, 0, 0, 0, 50001, 100, 80, 0)
        far = [(2, 0, 0, 0, 60001 + 7 * r, 100, 80, 0) for r in range(PU.TILE + 30)]
        near = (2, 0, 0, 0, 1001, 100, 80, 0)
        mate = [(0, 0, 1, 0, 1301, 100, 85, 33), (2, 0, 1, 1, 1301, 100, 85, 0)]
        long_, short = [head] + far + [near], mate
        reads += [long_, short] if long_first else [short, long_]
    b = PU.make_batch(reads)
    got, want = _exact(env, b, D)
    n = PU.TILE + 32
    assert want["pairs"][:, :3].tolist() == [[n - 1, n, 1 | 2 | 4 | 8], [n + 2, 2 * n + 3, 1 | 2 | 4 | 16]]
    assert want["pairs"][:, 6].tolist() == [1, 1]


@pytest.mark.parametrize("mask", range(1, 8))
def test_every_orientation_mask(env, mask):
    rng = np.random.default_rng(80 + mask)
    b = PU.random_batch(rng, [(1, 1)] * 40 + [(3, 4)] * 20 + [(9, 9), (20, 5)])
    got, want = _exact(env, b, D._replace(orient=mask))
    assert 0 < want["totals"][1] < 62 or mask == 7


def test_the_ends_of_every_range(env):
    rng = np.random.default_rng(90)
    b = PU.random_batch(rng, [(1, 1)] * 30 + [(4, 3)] * 20 + [(10, 9), (0, 2), (70, 1)])
    big = 1 << 30
    for change in (dict(isize_min=0, isize_max=0), dict(isize_min=big, isize_max=big), dict(isize_max=big), dict(isize_mean=0),
                   dict(isize_mean=big), dict(isize_mean=big, pen_slope=65536, pen_max=1 << 20), dict(pen_slope=0), dict(pen_slope=65536),
                   dict(pen_max=0), dict(pen_max=1 << 20, pen_slope=65536), dict(pen_unpaired=0), dict(pen_unpaired=1 << 20),
                   dict(mapq_boost=0), dict(mapq_boost=60), dict(orient=7, pen_unpaired=1 << 20, pen_max=1 << 20, pen_slope=65536)):
        got, want = _exact(env, b, D._replace(**change))
        if change.get("isize_max") == 0 or change.get("isize_min") == big:
            assert want["totals"][1] == 0
        if change == dict(pen_unpaired=1 << 20):
            assert want["totals"][1] > 10


def test_n_records_cuts_a_pair_and_no_class_rows(env):
    rng = np.random.default_rng(91)
    counts = [(2, 3), (1, 1), (9, 9), (4, 0), (3, 3), (70, 2)]
    b = PU.random_batch(rng, counts, far=0.0)
    so = b["sel_offsets"]
    total = int(so[-1])
    for n_records in (int(so[5]) + 4, int(so[4]) + 2, int(so[3]), int(so[2]) + 1, 1, 0, total - 1, total + 5):
        _exact(env, b, D._replace(orient=7), n_records=n_records)      # inside a wide pair, between two mates, inside a mate, ...
    got, want = _exact(env, b, D._replace(orient=7), cap=0)
    full = PU.expected(b, D._replace(orient=7))
    assert not (want["pairs"][:, 2] & 24).any() and (full["pairs"][:, 2] & 24).any()
    bare, _ = _exact(env, b, D, totals=False)
    assert "totals" not in bare
    e = PU.make_batch([])
    got, want = _exact(env, e, D)                                    # N == 0: zero totals and nothing else
    assert got["totals"].tolist() == [0, 0, 0, 0]
    down = dict(b, sel_offsets=so[::-1].copy())
    PU.call(env.lib, env.ix, down, D, want_rc=PU.INVALID)


def test_more_narrow_pairs_than_one_grid_of_lanes(env):
    rng = np.random.default_rng(92)
    n = 70000                                                        # 274 blocks of lanes, 69 rounds of the 1024-wide scan
    counts = rng.integers(0, 3, (n, 2))
    # the batch is built with numpy: one contig, mates a few hundred bases apart, every record past the head a secondary of the head
    per_read = counts.reshape(-1)
    so = np.zeros(2 * n + 1, np.int64)
    so[1:] = np.cumsum(per_read)
    T = int(so[-1])
    read = np.repeat(np.arange(2 * n), per_read)
    head = so[read]
    rec, klass = np.zeros((T, 12), np.int32), np.zeros((T, 4), np.int32)
    rec[:, 0], rec[:, 1], rec[:, 2] = read, np.arange(T), np.where(np.arange(T) == head, 0, 2)
    rec[:, 3], rec[:, 5], rec[:, 6] = rng.integers(0, 2, T), 1000 * (read // 2) + rng.integers(1, 900, T), rng.integers(50, 151, T)
    rec[:, 9], rec[:, 11] = rng.integers(60, 64, T), np.where(rec[:, 2] == 0, rng.integers(0, 61, T), 0)
    klass[:, 0], klass[:, 1] = rec[:, 2], head
    b = {"sel_offsets": so, "records": rec, "klass": klass}
    got, want = _exact(env, b, D._replace(orient=3))
    assert want["totals"][1] > 5000 and want["totals"][2] > 500 and want["totals"][3] > 5000


def test_more_wide_pairs_than_one_grid_of_waves(env):
    import torch
    rng = np.random.default_rng(93)
    waves = 4 * 4 * torch.cuda.get_device_properties(0).multi_processor_count      # four blocks of four waves per CU
    n = waves + 150
    assert n < 10000
    b = PU.random_batch(rng, [(5, 13) if k % 2 else (33, 2) for k in range(n)], scores=(60, 64))
    got, want = _exact(env, b, D._replace(orient=7))
    assert want["totals"][1] > n // 2 and want["totals"][2] > n // 4


# ------------------------------------------------------------------ through the pipeline
CHAIN_OPTS = dict(min_score=25)


def _smem(env, name):
    m = env.g.ExactMatch(name)
    m.set_reference("".join("ACGT"[c] for c in env.T))
    return env.g.SMEM(m, 4), env.g.ReferenceSet(["a", "b", "c"], TABLE, env.T)


def _np(t):
    import torch
    return (t.view(torch.int32) if t.dtype == torch.uint32 else t).cpu().numpy()


def _text(q):
    return "".join("ACGT"[c] for c in q)


def test_repeat_far_and_half_mapped_pairs(env):
    T = env.T
    sm, rs = _smem(env, "pair_planted.fa")
    reads = [T[2050:2200].copy(), AU.revcomp(T[9400:9550]),         # inside the duplication; unique, behind the SECOND copy
             T[500:650].copy(), AU.revcomp(T[5500:5650]),           # 5 kb apart on one contig
             T[13000:13150].copy(), np.random.default_rng(94).integers(0, 4, 150).astype(np.uint8)]      # one random mate
    strs = [_text(q) for q in reads]
    mems, chains, aln = sm.find_alignments(strs, 15, rs, both_strands=True, **CHAIN_OPTS)
    host = lambda t: t.cpu().numpy()      # noqa: E731
    csr = sm._csr_reads(strs, False)
    b = {"S": 2, "bases": np.asarray(csr[0]), "read_offsets": np.asarray(csr[1]), "offsets": host(mems[0]), "rows": host(mems[1]),
         "anchor_chain": host(chains[2]), "anchor_pred": host(chains[3]), "chain_offsets": host(chains[0]), "chains": host(chains[1])}
    b["aln"] = AU.expected(b, AU.DEFAULTS, T, TABLE)[0]             # the CPU's alignment of every chain ...
    sel = SU.expected(b, SU.DEFAULTS, TABLE)                        # ... the CPU's selection ...
    pb = {"sel_offsets": sel["offsets"], "records": sel["records"], "klass": sel["klass"]}
    want = PU.expected(pb, D)                                       # ... and the CPU's pairing: the planted cases hold in it
    so, rec = sel["offsets"], sel["records"]
    assert np.diff(so).tolist() == [2, 1, 1, 1, 1, 0]
    # repeat pair: proper; mate 0's chosen record is the copy next to its mate (contig b, 9051 - 6000), whichever kind it had
    r0, r1, flags = want["pairs"][0, :3].tolist()
    assert flags & 7 == 7 and r1 == so[1] and rec[r0, [0, 4, 5]].tolist() == [0, 1, 3051] and rec[r1, [4, 5, 3]].tolist() == [1, 3401, 1]
    assert rec[so[0], 11] == 0 and rec[r0, 11] == 0                  # select alone: mapq 0 inside the duplication
    raised = min(int(want["mapq"][0]), D.mapq_boost)
    assert raised > 0 and want["sam"][r0].tolist() == [99, raised, r1, 500] and want["sam"][r1, [0, 2, 3]].tolist() == [147, r0, -500]
    other = so[0] + so[0] + 1 - r0                                   # mate 0's other record: the copy far from the mate
    assert want["sam"][other, 0] & 0x100 and want["sam"][other, 1] == 0 and want["pairs"][0, 6] == 1
    # far pair: not proper, both heads kept
    assert want["pairs"][1, :3].tolist() == [so[2], so[3], 6] and want["pairs"][1, 5:].tolist() == [5150, 0, 0]
    assert want["sam"][so[2]].tolist() == [97, 60, so[3], 5150] and want["sam"][so[3]].tolist() == [145, 60, so[2], -5150]
    # half-mapped pair
    assert want["pairs"][2].tolist() == [so[4], -1, 2, 0, 0, 0, 0, -1] and want["sam"][so[4]].tolist() == [73, 60, -1, 0]
    assert want["totals"].tolist() == [2, 1, int(r0 != so[0]), 1]
    # the GPU: the pieces, then the whole
    assert np.array_equal(host(aln), b["aln"])
    got_sel = sm.select_alignments(csr[1], chains[0], chains[1], aln, rs, True)
    pairs, sam, totals = sm.pair_alignments(got_sel[0], got_sel[2], got_sel[3])
    PU.agrees({"pairs": host(pairs), "sam": host(sam), "totals": host(totals)}, want)
    out = sm.map_pairs(strs, 15, rs, **CHAIN_OPTS)
    assert len(out) == 7 and np.array_equal(host(out[0]), rec) and np.array_equal(host(out[1]), so)
    PU.agrees({"pairs": host(out[5]), "sam": host(out[6])}, want)
    split = sm.map_pairs((strs[0::2], strs[1::2]), 15, rs, **CHAIN_OPTS)      # two files: the same as the interleaved batch
    for x, y in zip(out, split):
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(_np(x), _np(y))
    wide = sm.map_pairs(strs, 15, rs, pair_options=dict(isize_max=6000, pen_max=0), **CHAIN_OPTS)
    assert host(wide[5])[:, 2].tolist() == [7, 7, 2]                 # options reach the call: the far pair is proper now
    lines = env.g.sam_lines(out[0], out[6], out[4], out[2], out[3], [f"p{i // 2}" for i in range(6)], rs.names, strs)
    assert len(lines) == rec.shape[0] + 1 and lines[-1].split("\t")[:4] == ["p2", "133", "c", "1001"]
    assert [ln.split("\t")[1] for ln in lines if ln.startswith("p0\t")].count("99") == 1
