"""CPU: tests/handout_util.py, so that test_group_handout_gpu.py cannot be wrong on its own.  The gathered expectations of
every order equal smem_util.expected_batch on the explicit list of reads, in every form the GPU test compares (bwa with
min_len 1 and 12, lut, reads with breaks, both strands, slots); every order has the property it is there for; the packed
variant leaves out only the reads that 2 bits cannot carry."""
import numpy as np
import pytest

import handout_util as H
import lookup_util as U
import smem_util as S
from test_tuning_knobs_gpu import _with_breaks

FAMILY = U.family()
REFS = ["rand4096", "tandem7", "noT", "tail_AAAAAAAA"]
N = 2001
K = 8
CAP = 8


def _same(got, want):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)


@pytest.mark.parametrize("name", REFS)
def test_gathered_expectations_are_those_of_the_explicit_batch(name):
    ref = FAMILY[name]
    reads = H.pool(name, "short")[0]
    assert 300 <= len(reads) <= 420 and sum(len(r) == 0 for r in reads) == 1
    for order, pick in H.orders(reads, N, 5).items():
        batch = [reads[i] for i in pick]
        for mode, min_len in (("bwa", 1), ("bwa", 12), ("lut", 1)):
            got = H.gather_expected(H.per_read(name, reads, mode, min_len, K), pick)
            _same(got, S.expected_batch(ref, batch, mode, min_len, K))
            assert min_len > 1 or len(got[1]) > N, (order, mode)
        cut = _with_breaks(reads, K)
        for min_len in (1, 12):
            _same(H.gather_expected(H.per_read(name, cut, "bwa", min_len, split=True), pick),
                  S.expected_batch(ref, [cut[i] for i in pick], "bwa", min_len, split=True))
        both = H.both_strands(reads)
        assert len(both) == 2 * len(reads) and all(np.array_equal(both[2 * i], r) for i, r in enumerate(reads))
        _same(H.gather_expected(H.per_read(name, both, "lut", 1, K), H.both_pick(pick)),
              S.expected_batch(ref, H.both_strands(batch), "lut", 1, K))
        # the slot form: the first min(count, cap) rows of every read, the true count, READ_OVERFLOW above the capacity
        counts, slots, filled, status = H.gather_slots(H.per_read(name, reads, "bwa", 1), pick, CAP)
        off, rows, st = S.expected_batch(ref, batch, "bwa", 1)
        assert counts.tolist() == np.diff(off).tolist() and filled.sum(axis=1).tolist() == np.minimum(counts, CAP).tolist()
        assert (status == H.READ_OVERFLOW).tolist() == (counts > CAP).tolist() and (counts > CAP).any()
        assert status[counts <= CAP].tolist() == st[counts <= CAP].tolist()
        for b in np.concatenate([np.arange(0, N, 97), np.flatnonzero(counts > CAP)[:20]]):
            k = min(int(counts[b]), CAP)
            assert slots[b, :k].tolist() == rows[off[b]:off[b] + k].tolist() and not slots[b, k:].any()


@pytest.mark.parametrize("name", REFS[:2])
def test_gathered_expectations_of_the_mid_pool(name):
    reads = H.pool(name, "mid")[0]
    assert sorted({len(r) for r in reads}) == list(S.MID_LENGTHS)
    for order, pick in H.orders(reads, 301, 6).items():
        _same(H.gather_expected(H.per_read(name, reads, "bwa", 12), pick),
              S.expected_batch(FAMILY[name], [reads[i] for i in pick], "bwa", 12))


def _runs(pick):
    """(value, length) of the runs of equal values."""
    cut = np.flatnonzero(np.diff(pick)) + 1
    starts = np.concatenate([[0], cut])
    return list(zip(pick[starts].tolist(), np.diff(np.concatenate([starts, [len(pick)]])).tolist()))


@pytest.mark.parametrize("name", REFS + ["tandem1"])
@pytest.mark.parametrize("kind", ["short", "mid"])
def test_every_order_has_its_property(name, kind):
    reads, mat, lens = H.pool(name, kind)
    top = int(lens.max())
    assert mat.shape == (len(reads), top + 3) and top == (255 if kind == "short" else 1409)
    for i, r in enumerate(reads):
        assert mat[i, :len(r)].tolist() == r.tolist() and (mat[i, len(r):] == H.JUNK).all()
    n_reads = 2 * len(reads) ** 2 + 1                         # the GPU batches are larger
    order = H.orders(reads, n_reads, 7)
    assert all(p.min() >= 0 and p.max() < len(reads) for p in order.values())
    assert len(np.unique(order["shuffled"])) > 0.9 * len(reads)
    k = H.kinds(reads)
    # the kinds are what they are called
    slow = reads[k["slow"]]
    unit = U._codes(U.TANDEM_UNITS[int(name[6:])]) if U.is_tandem(name) else slow[:1]
    assert len(slow) == top and slow.tolist() == np.tile(unit, top // len(unit) + 1)[:top].tolist()
    assert H.flagged(reads[k["flagged"]]) and len(reads[k["flagged"]]) == top
    assert len(reads[k["longest"]]) == top and not H.flagged(reads[k["longest"]]) and k["longest"] != k["slow"]
    assert len(reads[k["one"]]) == (1 if kind == "short" else 256) and not H.flagged(reads[k["one"]])
    assert (kind == "short") == ("empty" in k) and (kind != "short" or len(reads[k["empty"]]) == 0)
    # runs: every kind meets every run length; at least 300 flagged reads directly after a run of the slow-path read
    runs = _runs(order["runs"])
    for what in k:
        assert {n for v, n in runs[:-1] if v == k[what]} >= set(H.RUN_LENGTHS), what
    assert any(a[0] == k["slow"] and a[1] >= 64 and b[0] == k["flagged"] and b[1] >= 300 for a, b in zip(runs, runs[1:]))
    if "empty" in k:
        assert any(a[0] == k["flagged"] and b[0] == k["empty"] and b[1] >= 300 for a, b in zip(runs, runs[1:]))
    # long_then_short: a longest read directly followed by a shortest one (and by the empty one); every read after every other
    p = order["long_then_short"]
    after = {(int(c) >> 12, int(c) & 4095) for c in np.unique(lens[p[:-1]].astype(np.int64) << 12 | lens[p[1:]])}
    low = int(lens[lens > 0].min())
    assert (top, low) in after and (kind != "short" or (top, 0) in after)
    assert len(np.unique(p[0:-1:2] * len(reads) + p[1::2])) == len(reads) ** 2
    assert {(a, b) for a in set(lens.tolist()) for b in set(lens.tolist()) if a > b} <= after
    # tail: the last reads are one flagged, one empty (shortest) and the longest; before them the shuffled order goes on
    t = order["tail"][-H.TAIL_READS:]
    assert t[0] == k["flagged"] and t[1] == k.get("empty", k["one"]) and (t[2:] == k["longest"]).all() and len(t) == 37
    assert len(np.unique(order["tail"][:-H.TAIL_READS])) > 0.9 * len(reads)
    for pick in order.values():
        assert len(pick) % 2 == 1 and len(pick) % 16 and len(pick) % 256 and len(pick) % 512


@pytest.mark.parametrize("name", REFS + ["tandem1"])
def test_packed_pool_leaves_out_only_the_flagged_reads(name):
    reads = H.pool(name, "short")[0]
    out = [r for r in reads if H.flagged(r)]
    assert 0 < len(out) < len(reads) / 8
    assert all(int(r.max()) == S.BAD_CODE and (r > 3).sum() == 1 for r in out)
    for L in (150, 255):                                     # the fixed-length batches of the packed calls
        keep = [r for r in reads if len(r) == L and not H.flagged(r)]
        assert len(keep) >= 10 and sum(len(r) == L for r in reads) == len(keep) + 1
