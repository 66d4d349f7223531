"""GPU: genie_select_alignments against the walk in key order of tests/select_util.py, every output exactly equal.  Synthetic
d_aln / d_chains / offsets exercise the call without the pipeline in front of it: reads on both sides of the lane / wave border
and of the wave's 64 lanes, a read wider than the LDS tile, equal scores, both strands, skipped chains and chains below
min_score, cap_chains cutting a read, the ends of every parameter's range, the sizing call and a cap_sel below the total, a contig
table, more reads than one grid of lanes and more wide reads than one grid of waves.  Then the pipeline on a 16 kb reference:
the primary of every read is SMEM.map_reads' hit, and planted repeats, unique reads and chimeric reads come out as secondary,
unique and supplementary, each expectation computed by the CPU brute forces before the GPU is asked."""
import numpy as np
import pytest

import align_util as AU
import select_util as SU

pytestmark = pytest.mark.gpu

P = SU.Params
D = SU.DEFAULTS
N_REF = 1 << 14
TABLE = np.asarray([0, 6000, 12000, N_REF], np.int64)
SETS = (D, P(0, 100, 1, 22, 7), P(100, 0, 1 << 20, 1, 1), P(30, 90, 0, 1, 40))


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
    """The call against the walk: every output, then the checks that hold whatever the tie-breaks."""
    want = SU.expected(b, prm, kw.get("table"), kw.get("cap"), kw.get("cap_sel"))
    got = SU.call(env.lib, env.ix, b, prm, **kw)
    SU.agrees(got, want, [k for k in want if k in got])
    assert kw.get("sizing") or "sel" in got
    return got, want


BORDER = [0, 1, 2, SU.LANE_MAX - 1, SU.LANE_MAX, SU.LANE_MAX + 1, SU.LANE_MAX + 2]


@pytest.mark.parametrize("S", (1, 2))
def test_candidate_counts_around_the_borders(env, S):
    assert env.g._native.SELECT_LANE_MAX == SU.LANE_MAX and env.g._native.SELECT_TILE == SU.TILE
    rng = np.random.default_rng(51 + S)
    counts = BORDER + [63, 64, 65, 129, 1000, SU.TILE + 88, 3, 0]
    b = SU.random_batch(rng, counts, S, L=(150, 400))
    assert int(np.diff(b["chain_offsets"]).reshape(-1, S).sum(1).max()) > SU.TILE
    for prm in SETS:
        got, want = _exact(env, b, prm)
        SU.check_result(b, prm, got)
    assert want["counts"][counts.index(SU.TILE + 88), 0] > SU.TILE      # candidates, not only chains, beyond the LDS tile
    assert set(want["klass"][:, 0].tolist()) == {0, 1, 2}


def test_many_equal_scores(env):
    rng = np.random.default_rng(53)
    b = SU.random_batch(rng, [5, 9, 70, 200, 8, 600], 2, scores=(30, 31))
    for prm in SETS:
        _exact(env, b, prm)
    b = SU.random_batch(rng, [4, 12, 130], 1, scores=(30, 32), L=(60, 61))
    b["aln"][:, 1], b["aln"][:, 2] = 0, 60                          # every chain covers the read: one primary, the rest its secondaries
    got, want = _exact(env, b, D)
    assert want["counts"][:, 1].tolist() == [1, 1, 1] and want["counts"][:, 2].tolist() == [3, 11, 129]


def test_strand_one_is_converted_to_forward_coordinates(env):
    row = lambda score, qb, qe: (score, qb, qe, 100, 100 + qe - qb, 0, qe - qb, 0)      # noqa: E731
    units = [[row(50, 60, 100)], [row(45, 0, 40)],                  # overlap only when strand 1 is converted: [0, 40) is [60, 100)
             [row(50, 0, 40)], [row(45, 0, 40)],                    # overlap only when it is not
             [row(50, 10, 30)] * 5, [row(50, 70, 90)] * 5]          # the same on the wave path: ten chains, all on [10, 30)
    b = SU.make_batch([100, 100, 100], units, 2)
    got, want = _exact(env, b, D)
    assert want["klass"][:4, 0].tolist() == [0, 2, 0, 1] and want["counts"][2].tolist() == [10, 1, 9, 4]
    assert got["records"][1, [3, 7, 8]].tolist() == [1, 60, 100]


def test_skipped_chains_min_score_and_a_cut_batch(env):
    rng = np.random.default_rng(54)
    counts = [6, 0, 30, 8, 9, 100, 2]
    b = SU.random_batch(rng, counts, 2, skipped=0.3)
    prm = D._replace(min_score=23)
    got, want = _exact(env, b, prm)
    assert (want["klass"][:, 0] == 3).sum() > 40 and want["counts"][:, 0].sum() < sum(counts)
    co = b["chain_offsets"]
    for cap in (int(co[4]) + 7, int(co[2]) + 3, int(co[-1]) - 1, int(co[5]), 0, int(co[-1]) + 5):      # in a wide read, in a narrow one, ...
        _exact(env, b, prm, cap=cap)


def test_the_ends_of_every_range(env):
    rng = np.random.default_rng(55)
    b = SU.random_batch(rng, [7, 20, 3, 0, 66, 8, 9], 1)
    for change in (dict(max_secondary=0), dict(max_secondary=1), dict(max_secondary=1 << 20), dict(mask_level=0), dict(mask_level=100),
                   dict(pri_ratio=0), dict(pri_ratio=100), dict(min_score=1 << 30), dict(mapq_full=1), dict(mapq_full=1 << 20)):
        got, want = _exact(env, b, D._replace(**change))
        if change.get("max_secondary") == 0:
            assert want["totals"][3] == want["totals"][1] and want["totals"][2] > 0
        if change.get("max_secondary") == 1 << 20:
            assert want["totals"][3] > want["totals"][1] + 5
        if "min_score" in change:
            assert not want["totals"].any() and (want["klass"][:, 0] == 3).all()


def test_sizing_call_and_a_small_cap_sel(env):
    rng = np.random.default_rng(56)
    b = SU.random_batch(rng, [7, 20, 3, 0, 66, 8, 9], 2)
    full, want = _exact(env, b, D)
    total = int(want["offsets"][-1])
    assert total > 12
    sized, _ = _exact(env, b, D, sizing=True)
    assert "sel" not in sized and sized["offsets"][-1] == total
    for cap_sel in (total - 1, 5, 0, total + 4):
        got, _ = _exact(env, b, D, cap_sel=cap_sel)
        assert got["offsets"][-1] == total and got["sel"].size == min(total, cap_sel)      # SU.call has looked behind cap_sel
    bare, _ = _exact(env, b, D, extras=False)
    assert "counts" not in bare and np.array_equal(bare["records"], full["records"])


def test_contig_table(env):
    rng = np.random.default_rng(57)
    b = SU.random_batch(rng, [7, 20, 3, 0, 66], 2, contigs=3)
    starts = TABLE[b["chains"][:, 6]]
    b["aln"][:, 3] = starts + 1 + rng.integers(0, 5000, starts.size)      # inside its contig, 1-based in the concatenation
    b["aln"][:, 4] = b["aln"][:, 3] + b["aln"][:, 2] - b["aln"][:, 1]
    got, want = _exact(env, b, D, table=TABLE)
    assert set(want["records"][:, 4].tolist()) == {0, 1, 2} and (want["records"][:, 5] >= 1).all() and (want["records"][:, 5] <= 5000).all()
    plain, _ = _exact(env, b, D)
    assert not plain["records"][:, 4].any() and np.array_equal(plain["records"][:, 5], b["aln"][plain["sel"], 3])


def test_more_narrow_reads_than_one_grid_of_lanes(env):
    rng = np.random.default_rng(58)
    counts = rng.integers(0, 4, 70000)                              # 274 blocks of lanes, 69 rounds of the 1024-wide scan
    b = SU.random_batch(rng, counts, 2)
    got, want = _exact(env, b, D)
    assert want["totals"][0] > 90000 and want["totals"][2] > 1000


def test_more_wide_reads_than_one_grid_of_waves(env):
    import torch
    rng = np.random.default_rng(59)
    waves = 4 * 4 * torch.cuda.get_device_properties(0).multi_processor_count      # four blocks of four waves per CU
    n = waves + 150
    assert n < 10000
    counts = rng.integers(SU.LANE_MAX + 1, SU.LANE_MAX + 4, n)
    b = SU.random_batch(rng, counts, 1, L=(50, 90))
    got, want = _exact(env, b, D)
    assert want["totals"][1] > n and want["totals"][2] > n


# ------------------------------------------------------------------ through the pipeline
CHAIN_OPTS = dict(min_score=25)


def _smem(env, name):
    m = env.g.ExactMatch(name)
    m.set_reference("".join("ACGT"[c] for c in env.T))
    return env.g.SMEM(m, 4), env.g.ReferenceSet(["a", "b", "c"], TABLE, env.T)


def _text(q):
    return "".join("ACGT"[c] for c in q)


def test_the_primary_is_map_reads_hit(env):
    g = env.g
    rng = np.random.default_rng(60)
    sm, rs = _smem(env, "select_map_reads.fa")
    reads = []
    for r in range(40):
        L = int(rng.integers(80, 200))
        c = int(rng.integers(0, 3))
        at = int(rng.integers(int(TABLE[c]), int(TABLE[c + 1]) - L))
        q = env.T[at:at + L].copy()
        if r % 5 == 4:
            q = AU.mutate(rng, q, 0.04)
        reads.append(AU.revcomp(q) if r % 2 else q)
    strs = [_text(q) for q in reads] + ["ACGT" * 20]                  # ... and a read that maps nowhere
    hits, offs, cigar = sm.map_reads(strs, 15, rs, **CHAIN_OPTS)
    records, sel_offsets, c_offs, c_ops, info = sm.map_records(strs, 15, rs, **CHAIN_OPTS)
    hits, records, sel_offsets = hits.cpu().numpy(), records.cpu().numpy(), sel_offsets.cpu().numpy()
    texts, mine = g.cigar_strings(offs, cigar), g.cigar_strings(c_offs, c_ops)
    assert records.shape[0] == info.shape[0] == len(mine) == sel_offsets[-1] and sel_offsets.size == len(strs) + 1
    for i in range(len(strs)):
        rows = records[sel_offsets[i]:sel_offsets[i + 1]]
        if hits[i, 0] < 0:
            assert rows.shape[0] == 0
            continue
        assert rows[0, 2] == 0 and (rows[1:, 2] > 0).all() and (rows[:, 0] == i).all()
        assert rows[0, [1, 3, 4, 5, 9]].tolist() == hits[i, :5].tolist()
        assert mine[sel_offsets[i]] == texts[i]
    assert (hits[:40, 0] >= 0).all() and hits[40, 0] == -1
    lines = g.paf_lines(records, info, c_offs, c_ops, [f"r{i}" for i in range(len(strs))], [len(s) for s in strs], rs.names,
                        np.diff(TABLE))
    assert len(lines) == records.shape[0] and lines[0].split("\t")[0] == "r0" and all(len(ln.split("\t")) == 15 for ln in lines)


def test_planted_repeat_unique_and_chimeric_reads(env):
    T = env.T
    sm, rs = _smem(env, "select_planted.fa")
    chimera = np.concatenate([T[500:650], T[13000:13150]])
    reads = [T[2050:2200].copy(), T[4000:4150].copy(), chimera, AU.revcomp(chimera), T[9100:9250].copy()]
    strs = [_text(q) for q in reads]
    mems, chains, aln = sm.find_alignments(strs, 15, rs, both_strands=True, **CHAIN_OPTS)
    host = lambda t: t.cpu().numpy()      # noqa: E731
    csr = sm._csr_reads(strs, False)
    b = {"S": 2, "bases": np.asarray(csr[0]), "read_offsets": np.asarray(csr[1]), "offsets": host(mems[0]), "rows": host(mems[1]),
         "anchor_chain": host(chains[2]), "anchor_pred": host(chains[3]), "chain_offsets": host(chains[0]), "chains": host(chains[1])}
    b["aln"] = AU.expected(b, AU.DEFAULTS, T, TABLE)[0]             # the CPU's alignment of every chain ...
    want = SU.expected(b, D, TABLE)                                 # ... and the CPU's selection: the planted cases hold in it
    assert want["counts"][0].tolist()[:3] == [2, 1, 1] and want["counts"][4].tolist()[:3] == [2, 1, 1]
    assert want["counts"][1].tolist()[:3] == [1, 1, 0]
    assert want["counts"][2].tolist()[:3] == [2, 2, 0] and want["counts"][3].tolist()[:3] == [2, 2, 0]
    by_read = [want["records"][want["offsets"][i]:want["offsets"][i + 1]] for i in range(5)]
    for i in (0, 4):                                                # inside the repeat: mapq 0, one secondary, in the other copy
        assert by_read[i][:, 2].tolist() == [0, 2] and by_read[i][0, 11] == 0 and by_read[i][0, 10] == by_read[i][0, 9]
        assert by_read[i][by_read[i][:, 4].argsort()][:, [4, 5]].tolist() == [[0, 2051 + (i > 0) * 50], [1, 3051 + (i > 0) * 50]]
    assert by_read[1][:, 2].tolist() == [0] and by_read[1][0, 11] == 60 and by_read[1][0, [4, 5]].tolist() == [0, 4001]
    for i, strand in ((2, 0), (3, 1)):                              # half from contig a, half from contig c: primary and supplementary
        assert by_read[i][:, 2].tolist() == [0, 1] and (by_read[i][:, 3] == strand).all() and (by_read[i][:, 11] > 0).all()
        assert sorted(by_read[i][:, 4].tolist()) == [0, 2]
        first = by_read[i][by_read[i][:, 4] == 0][0]
        assert abs(first[7] - 150 * strand) <= 8 and abs(first[8] - 150 - 150 * strand) <= 8      # forward coordinates on either strand
    assert np.array_equal(host(aln), b["aln"])
    got = sm.select_alignments(csr[1], chains[0], chains[1], aln, rs, True)
    names = ("offsets", "sel", "records", "klass", "counts", "totals")
    SU.agrees({k: host(v) for k, v in zip(names, got)}, want)
    records = sm.map_records(strs, 15, rs, **CHAIN_OPTS)[0]
    assert np.array_equal(host(records), want["records"])
