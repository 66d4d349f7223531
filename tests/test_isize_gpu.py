"""GPU: genie_insert_size_stats against the brute force of tests/isize_util.py, d_stats, d_samples and d_totals exactly equal.
Planted (type, span, mapq) per pair exercise the call without the pipeline in front of it: batch sizes around a wave, mates
without records, mapq at the threshold, two contigs, type 3, every type dominant in turn, spans at both ends of [1, max_span] and
on both sides of the histogram's internal borders (the edge of the range counted in LDS, GENIE_ISIZE_LDS_BINS, and the last bin),
all samples in one bin and one sample per bin, more pairs than one grid of blocks takes in one step, n_records cutting a pair in
two, and NULL for the optional outputs.  Then the pipeline: a 2 kb library that map_pairs' defaults leave without a proper pair
and the estimate pairs completely; each expectation is computed by the CPU brute forces before the GPU is asked."""
import os
import re

import numpy as np
import pytest

import align_util as AU
import isize_util as IU
import pair_util as PU
from pair_util import FR, NO_TYPE, RF, SAME

pytestmark = pytest.mark.gpu

P = IU.Params
HEADER = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "genie_smem.h")).read()
LDS_BINS = int(re.search(r"#define GENIE_ISIZE_LDS_BINS (\d+)", HEADER).group(1))      # spans below it are counted in LDS
MOST = int(re.search(r"#define GENIE_WINDOW_MAX (\d+)", HEADER).group(1)) // 2          # the largest max_span
N_REF = 20000


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
    e.T = np.random.default_rng(60).integers(0, 4, N_REF).astype(np.uint8)
    e.ix = g.GenieIndex.build(e.T, 0).to("cuda")
    return e


def _exact(env, b, p, **kw):
    want = IU.expected(b, p, kw.get("n_records"))
    got = IU.call(env.lib, env.ix, b, p, **kw)
    IU.agrees(got, want)
    return got, want


def _random_plan(rng, n, span=(150, 700)):
    kinds = [FR, FR, FR, FR, RF, SAME, NO_TYPE, "contigs"]
    plan = []
    for _ in range(n):
        u = rng.random()
        if u < 0.1:
            plan.append(("none", "left", "right")[int(rng.integers(0, 3))])
        else:
            plan.append((kinds[int(rng.integers(0, len(kinds)))], int(rng.integers(*span)), int(rng.integers(10, 61))))
    return plan


@pytest.mark.parametrize("pairs", [0, 1, 63, 64, 65])
def test_batch_sizes_around_a_wave(env, pairs):
    assert LDS_BINS == IU.LDS_BINS == env.g._native.ISIZE_LDS_BINS and MOST == 32768
    b = IU.batch_of(_random_plan(np.random.default_rng(100 + pairs), pairs), extra=1)
    got, want = _exact(env, b, P(20, 10000, 3))
    assert got["samples"].shape == (pairs, 2)
    if pairs == 0:
        assert not got["stats"].any() and not got["totals"].any()
    if pairs == 1:
        b = IU.batch_of([(SAME, 421)])
        got, want = _exact(env, b, P(20, 10000, 1))
        assert got["stats"][2].tolist() == [1, 1, 421, 421, 421, 421, 421, 1, 421, 0, 421, 421] and got["totals"].tolist() == [1, 1, 0, 0]
    if pairs >= 63:
        assert want["totals"][1] > 20 and want["totals"][2] > 3 and want["totals"][3] > 5


def test_what_gives_no_sample(env):
    plan = [(FR, 300), (RF, 250, 19), (SAME, 400, 20), (NO_TYPE, 90), ("contigs", 300), "none", "left", "right", (FR, 10001), (FR, 10000),
            (FR, 300, 60, 19), (FR, 300, 19, 60), (RF, 300, 20, 20), (FR, 0), (SAME, 0), (FR, 1), (RF, 1), (SAME, 1), (RF, 2)]
    b = IU.batch_of(plan, extra=2)
    got, want = _exact(env, b, P(20, 10000, 1))
    assert want["samples"][:, 0].tolist() == [0, -1, 2, -1, -1, -1, -1, -1, -1, 0, -1, -1, 1, -1, -1, 0, 1, 2, 1]
    assert want["samples"][:, 1].tolist() == [300, 0, 400, 0, 0, 0, 0, 0, 0, 10000, 0, 0, 300, 0, 0, 1, 1, 1, 2]
    assert want["totals"].tolist() == [16, 8, 3, 5]
    _exact(env, b, P(0, 10000, 1))                                   # no threshold
    got, want = _exact(env, b, P(60, 10000, 1))                      # mapq is clamped to 60, so 60 can still be met
    assert want["totals"][1] == 6
    wild = {k: v.copy() for k, v in b.items()}
    wild["records"][0, 11] = 1000                                    # clamped to 60: a sample
    wild["records"][int(b["sel_offsets"][1]), 11] = 61
    got, want = _exact(env, wild, P(60, 10000, 1))
    assert want["samples"][0].tolist() == [0, 300]


@pytest.mark.parametrize("main", [FR, RF, SAME])
def test_every_type_dominant_in_turn(env, main):
    rng = np.random.default_rng(110 + main)
    second, third = (main + 1) % 3, (main + 2) % 3
    plan = [(main, int(rng.integers(400, 600))) for _ in range(200)] + [(second, int(rng.integers(2000, 2400))) for _ in range(15)]
    plan += [(third, 5000 + k) for k in range(9)]
    order = rng.permutation(len(plan))
    b = IU.batch_of([plan[i] for i in order])
    got, want = _exact(env, b, P(20, 10000, 10))
    assert want["stats"][[main, second, third], 0].tolist() == [200, 15, 9]
    assert want["stats"][[main, second, third], 1].tolist() == [1, 1, 0]                # 20 * 9 < 200, and 9 < 10
    est = env.g.index.insert_size_options(got["stats"])
    assert est.orient == 1 << main and est.estimated and est.isize_min < 400 and 600 <= est.isize_max < 1200


@pytest.mark.parametrize("max_span", [1, 20, LDS_BINS - 2, LDS_BINS - 1, LDS_BINS, LDS_BINS + 1, MOST])
def test_spans_around_every_border(env, max_span):
    """Bin s of a type lives in LDS for s < min(GENIE_ISIZE_LDS_BINS, max_span + 1) and only in the global histogram from there
    on; the last bin is max_span."""
    borders = {0, 1, 2, 19, 20, 21, LDS_BINS - 2, LDS_BINS - 1, LDS_BINS, LDS_BINS + 1, max_span - 1, max_span, max_span + 1, MOST, MOST + 1}
    plan = []
    for s in sorted(borders):
        for t in (FR, RF, SAME):
            plan += [(t, s)] * (1 + (s + t) % 3)
    b = IU.batch_of(plan)
    got, want = _exact(env, b, P(20, max_span, 1))
    inside = sorted(s for s in borders if 1 <= s <= max_span)
    assert sorted(set(want["samples"][want["samples"][:, 0] == SAME, 1].tolist())) == inside
    assert sorted(set(want["samples"][want["samples"][:, 0] == RF, 1].tolist())) == inside
    assert want["stats"][:, 1].tolist() == [1, 1, 1] and (want["stats"][:, 11] <= max_span).all()


def test_one_bin_and_one_sample_per_bin(env):
    b = IU.batch_of([(FR, 300)] * 5000)                              # every lane of every block adds to the same bin
    got, want = _exact(env, b, IU.DEFAULTS)
    assert got["stats"][0].tolist() == [5000, 1, 300, 300, 300, 300, 300, 5000, 300, 0, 300, 300]
    b = IU.batch_of([(RF, LDS_BINS + 7)] * 3000)                     # the same past the range counted in LDS
    got, want = _exact(env, b, IU.DEFAULTS)
    assert got["stats"][1, [0, 1, 3, 9]].tolist() == [3000, 1, LDS_BINS + 7, 0]
    span = LDS_BINS + 500
    b = IU.batch_of([(SAME, s) for s in np.random.default_rng(120).permutation(np.arange(1, span + 1)).tolist()])
    got, want = _exact(env, b, P(20, span, 25))
    assert got["stats"][2, :5].tolist() == [span, 1, (span + 1) // 4 + 1, span // 2 + 1, (3 * span + 1) // 4 + 1]
    assert got["stats"][2, 7] == span and got["stats"][2, 10:].tolist() == [0, span]


def test_many_blocks_merge_to_the_same_bytes_twice(env):
    rng = np.random.default_rng(130)
    n = 70000
    spans = np.clip(np.rint(rng.normal(450, 40, n)), 1, None).astype(np.int64)
    kinds = rng.random(n)
    plan = []
    for k in range(n):
        u = kinds[k]
        if u < 0.9:
            plan.append((FR, int(spans[k]), 60 if u < 0.8 else 10))
        elif u < 0.96:
            plan.append((RF, int(spans[k]) + 3000 + LDS_BINS * (k % 2)))     # one half of them beyond the LDS range
        elif u < 0.98:
            plan.append((SAME, int(rng.integers(1, 9000))))
        else:
            plan.append(("none", "left", "right")[k % 3])
    b = IU.batch_of(plan)
    want = IU.expected(b, IU.DEFAULTS)
    one = IU.call(env.lib, env.ix, b, IU.DEFAULTS)
    two = IU.call(env.lib, env.ix, b, IU.DEFAULTS)
    IU.agrees(one, want)
    for k in one:
        assert one[k].tobytes() == two[k].tobytes(), k
    assert want["stats"][:, 1].tolist() == [1, 1, 0] and want["stats"][0, 0] > 50000 and 440 <= want["stats"][0, 3] <= 460
    assert want["totals"][2] > 5000


def test_n_records_cuts_a_pair_in_two(env):
    b = IU.batch_of([(FR, 300 + k) for k in range(40)], extra=1)
    so, T = b["sel_offsets"], b["records"].shape[0]
    for n_records in (T - 1, T - 2, T - 3, int(so[41]), int(so[41]) + 1, 1, 0, T + 5):
        got, want = _exact(env, b, P(20, 10000, 1), n_records=n_records)
        assert want["totals"][0] == want["totals"][1] == min(40, n_records // 4 + (1 if n_records % 4 == 3 else 0)), n_records


def test_optional_outputs_may_be_null(env):
    b = IU.batch_of(_random_plan(np.random.default_rng(140), 300))
    full, _ = _exact(env, b, P(20, 10000, 3))
    for kw in (dict(samples=False), dict(totals=False), dict(samples=False, totals=False)):
        got, _ = _exact(env, b, P(20, 10000, 3), **kw)
        assert ("samples" in got) == kw.get("samples", True) and ("totals" in got) == kw.get("totals", True)
        assert np.array_equal(got["stats"], full["stats"])


def test_python_call(env):
    import torch
    b = IU.batch_of(_random_plan(np.random.default_rng(150), 500))
    want = IU.expected(b, IU.DEFAULTS)
    stats, samples, totals = env.ix.insert_size_stats(b["sel_offsets"], torch.from_numpy(b["records"]), samples=True)
    assert stats.is_cuda and stats.dtype == torch.int64 and samples.dtype == torch.int32 and totals.dtype == torch.int64
    IU.agrees({"stats": stats.cpu().numpy(), "samples": samples.cpu().numpy(), "totals": totals.cpu().numpy()}, want)
    stats, samples, totals = env.ix.insert_size_stats(b["sel_offsets"], b["records"], min_mapq=0, max_span=400, min_samples=1)
    assert samples is None
    IU.agrees({"stats": stats.cpu().numpy(), "totals": totals.cpu().numpy()}, IU.expected(b, P(0, 400, 1)))


# ------------------------------------------------------------------ through the pipeline
CHAIN_OPTS = dict(min_score=25)
INSERTS = [1900, 1930, 1960, 1975, 1990, 2000, 2000, 2010, 2025, 2040, 2070, 2100]


def _text(q):
    return "".join("ACGT"[c] for c in q)


def _np(t):
    import torch
    return (t.view(torch.int32) if t.dtype == torch.uint32 else t).cpu().numpy()


def _same_results(x, y):
    assert len(x) == len(y)
    for a, b in zip(x, y):
        assert a.dtype == b.dtype and a.shape == b.shape and _np(a).tobytes() == _np(b).tobytes()


def test_a_two_kilobase_library_through_map_pairs(env):
    T = env.T
    m = env.g.ExactMatch("isize_library.fa")
    m.set_reference(_text(T))
    sm = env.g.SMEM(m, 4)
    rng = np.random.default_rng(160)
    reads = []
    for k in range(200):
        ins = INSERTS[k % len(INSERTS)]
        at = int(rng.integers(0, N_REF - ins))
        reads += [_text(T[at:at + 100]), _text(AU.revcomp(T[at + ins - 100:at + ins]))]
    host = lambda t: t.cpu().numpy()      # noqa: E731
    # the CPU first: on the device's records the defaults leave no pair proper
    csr = sm._csr_reads(reads, False)
    mems, chains, aln = sm.find_alignments(reads, 15, None, both_strands=True, **CHAIN_OPTS)
    sel = sm.select_alignments(csr[1], chains[0], chains[1], aln, None, True)
    pb = {"sel_offsets": host(sel[0]), "records": host(sel[2]), "klass": host(sel[3])}
    today = PU.expected(pb, PU.DEFAULTS)
    assert not (today["pairs"][:, 2] & 1).any() and today["totals"][0] >= 195
    so, rec = pb["sel_offsets"], pb["records"]
    unique = np.asarray([so[2 * k + 1] > so[2 * k] and so[2 * k + 2] > so[2 * k + 1] and rec[so[2 * k], 11] >= 20 and
                         rec[min(so[2 * k + 1], len(rec) - 1), 11] >= 20 for k in range(200)])
    assert unique.sum() >= 195
    brute = IU.expected(pb, IU.DEFAULTS)
    want = env.g.index.insert_size_options(brute["stats"])
    assert want.estimated and want.orient == 1 and 1900 <= want.stats[0][3] <= 2100 and want.stats[0][0] == unique.sum()
    assert want.isize_min <= 1900 and 2100 <= want.isize_max <= 10000
    paired = PU.expected(pb, PU.DEFAULTS._replace(orient=want.orient, isize_min=want.isize_min, isize_max=want.isize_max,
                                                  isize_mean=want.isize_mean))
    assert (paired["pairs"][unique, 2] & 1).all()
    # the GPU
    plain = sm.map_pairs(reads, 15, None, **CHAIN_OPTS)
    assert len(plain) == 7 and np.array_equal(host(plain[0]), rec) and not (host(plain[5])[:, 2] & 1).any()
    out = sm.map_pairs(reads, 15, None, insert_size="estimate", **CHAIN_OPTS)
    assert len(out) == 8 and np.array_equal(host(out[0]), rec) and np.array_equal(host(out[1]), so)
    est = out[7]
    assert isinstance(est, env.g.InsertSize) and est == want
    assert np.array_equal(np.asarray(est.stats, np.int64), brute["stats"])
    assert est.estimated and est.orient == env.g._native.PAIR_ORIENT["fr"] and 1900 <= est.stats[0][3] <= 2100
    PU.agrees({"pairs": host(out[5]), "sam": host(out[6])}, paired)
    assert (host(out[5])[unique, 2] & 1).all()
    _same_results(out[:7], sm.map_pairs(reads, 15, None, insert_size={}, **CHAIN_OPTS)[:7])
    strict = sm.map_pairs(reads, 15, None, insert_size=dict(min_samples=10**6), pair_options=dict(isize_max=1234), **CHAIN_OPTS)
    assert strict[7][:5] == (1, 0, 1234, 300, False) and strict[7].stats[0][:2] == (est.stats[0][0], 0)
    # an InsertSize passed back in: no estimate, the same bytes
    again = sm.map_pairs(reads, 15, None, insert_size=est, **CHAIN_OPTS)
    _same_results(out[:7], again[:7])
    assert again[7] is est
    # too few pairs: the fallback, and today's result
    few = sm.map_pairs(reads[:40], 15, None, insert_size="estimate", **CHAIN_OPTS)
    assert len(few) == 8 and not few[7].estimated and few[7][:4] == (1, 0, 1000, 300) and 15 <= few[7].stats[0][0] <= 20
    _same_results(few[:7], sm.map_pairs(reads[:40], 15, None, **CHAIN_OPTS))
    # sam_text takes the longer tuple
    names = [f"p{i // 2}" for i in range(len(reads))]
    a, b = sm.sam_text(out, reads, names), sm.sam_text(out[:7], reads, names)
    _same_results(a, b)
    # rescue looks where the estimate says: a pair whose second mate is random gets a window of isize_max bases
    lone = reads + [_text(T[5000:5100]), _text(np.random.default_rng(161).integers(0, 4, 100).astype(np.uint8))]
    res = sm.map_pairs(lone, 15, None, insert_size="estimate", rescue=True, **CHAIN_OPTS)
    assert len(res) == 9 and res[8] == est and est.isize_max != 1000
    windows = host(res[7][0])
    assert windows.shape == (2 * len(lone), 2) and windows[2 * 401 + 1].tolist() == [5000, 5000 + est.isize_max]
    narrow = sm.map_pairs(lone, 15, None, insert_size=est, rescue=True, rescue_options=dict(isize_max=700), **CHAIN_OPTS)
    assert host(narrow[7][0])[2 * 401 + 1].tolist() == [5000, 5700]
