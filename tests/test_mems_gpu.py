"""GPU tests of genie_find_mems (run with -m gpu on an MI355X): every maximal exact match of a read batch with its reference
position.  Every comparison is exact: against the brute force of tests/mems_util.py on references of lookup_util.family()
over dir_bits, table_bits and both forms of the match table, against the call without BOTH_STRANDS on the explicit
interleaved batch, against the rows of genie_find_smems_long_ex, and through the Python layer."""
import numpy as np
import pytest

import lookup_util as U
import match_stats_util as MS
import mems_util as MM

pytestmark = pytest.mark.gpu

BOTH, SPLIT = MM.BOTH, MM.SPLIT
FLAGS = (0, BOTH, SPLIT, BOTH | SPLIT)
FAMILY = U.family()
TINY = ["rand1", "rand2", "rand5", "rand37"]
NAMES = TINY + ["tail_AAAAAAAA", "tail_C", "tandem1", "tandem3", "tandem7", "noT", "rand4096"]
KNOBS = [(7, 0), (3, 4)]                                      # (dir_bits, table_bits): the automatic P2 = 8, and a key of 4 bases
# 3 is at most dir_bits 7 (two directory reads) and above dir_bits 3; 33 and 65 leave the inline key at dir_bits 7 and 3 / reach
# the packed reference; 100 compares more than one of its words
MIN_LENS = (3, 12, 20, 33, 65, 100)


@pytest.fixture(scope="module")
def pkg():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import genie_smem_amd as g
    g._native.lib()
    return g


def _index(pkg, name, form="compact", knobs=KNOBS[0]):
    return pkg.GenieIndex.build(FAMILY[name], 0, dir_bits=knobs[0], table_bits=knobs[1], table_format=form).to("cuda")


def _reads(name):
    """Matches that cross and end at the 256-position windows, breaks everywhere, an empty read, reads of one base, and two
    reads longer than the reference."""
    ref = FAMILY[name]
    rng = np.random.default_rng(len(ref) + 2)
    longer = [np.concatenate([ref, ref[:40]]).astype(np.uint8), np.concatenate([rng.integers(0, 4, 5), ref, [7], ref[:9]]).astype(np.uint8)]
    return MS.window_reads(ref) + MS.break_reads(ref) + longer


def _check(pkg, ix, ref, reads, flags, m, tag, max_occ=0, lead=0, tail=0):
    """The sizing call and the call with exactly that room against the restated specification -> (offsets, rows)."""
    lib = pkg._native.lib()
    bases, offs = MS.csr(reads, lead, tail)
    off, rows, st, tt = MM.sized_call(lib, ix, flags, bases, offs, m, max_occ)
    w_off, w_rows, w_st, w_skip = MM.expected(ref, reads, flags, m, max_occ)
    assert np.array_equal(st, w_st), (tag, "status")
    assert np.array_equal(off, w_off), (tag, "offsets", np.flatnonzero(off != w_off)[:5])
    assert rows.shape == w_rows.shape and np.array_equal(rows, w_rows), (tag, "rows", np.flatnonzero((rows != w_rows).any(1))[:5])
    assert tt.tolist() == [w_rows.shape[0], w_skip], (tag, "totals")
    return off, rows


# ------------------------------------------------------------------ brute-force parity
@pytest.mark.parametrize("name", NAMES)
def test_every_mem_against_brute_force(pkg, name):
    ref = FAMILY[name]
    reads = _reads(name)
    forms = [("compact", k) for k in KNOBS] + ([("wide", k) for k in KNOBS] if name == "rand4096" else [])
    most = 0
    for form, knobs in forms:
        ix = _index(pkg, name, form, knobs)
        for m in MIN_LENS + ((1,) if name in TINY else ()):
            for flags in FLAGS:
                off, rows = _check(pkg, ix, ref, reads, flags, m, (name, form, knobs, m, flags))
                most = max(most, rows.shape[0])
    assert most > (0 if name in ("rand1", "rand2") else 50)
    if name == "tandem7":                                           # seeds of hundreds of rows, far more than left-maximal ones
        assert most > 10_000


def test_lengths_beyond_the_longest_match_interval(pkg):
    """Rows of a seed that lie outside the interval of the position's longest match get their length from the reference:
    on tandem3 every position has them.  Counted here so that the path cannot go untested."""
    name = "tandem3"
    ref = FAMILY[name]
    ix = _index(pkg, name)
    reads = MS.window_reads(ref)
    lib = pkg._native.lib()
    bases, offs = MS.csr(reads)
    off, rows = _check(pkg, ix, ref, reads, 0, 12, name)
    ms, lohi, st = MS.call(lib, ix, 0, bases, offs)
    at = np.repeat(offs[:-1], np.diff(off)) + rows[:, 0]
    shorter = rows[:, 1] - rows[:, 0] < ms[at]
    assert shorter.sum() > 100 and (~shorter).sum() > 100
    assert ((rows[shorter, 3] < lohi[at[shorter], 0]) | (rows[shorter, 3] > lohi[at[shorter], 1])).all()


# ------------------------------------------------------------------ both strands
@pytest.mark.parametrize("name", ["rand4096", "noT", "tandem3"])
def test_both_strands_is_the_interleaved_batch(pkg, name):
    lib = pkg._native.lib()
    ix = _index(pkg, name)
    reads = _reads(name)
    for split in (0, SPLIT):
        for m in (3, 33):
            got = MM.sized_call(lib, ix, BOTH | split, *MS.csr(reads, 7, 5), m)
            want = MM.sized_call(lib, ix, split, *MS.csr(MS.strand_reads(reads, 2), 14, 10), m)
            assert all(np.array_equal(x, y) for x, y in zip(got, want)), (name, split, m)
            assert got[1].tobytes() == want[1].tobytes()


# ------------------------------------------------------------------ max_occ
@pytest.mark.parametrize("name", ["tandem1", "rand4096"])
def test_max_occ_skips_positions_and_counts_them(pkg, name):
    ref = FAMILY[name]
    ix = _index(pkg, name)
    reads = _reads(name)
    lib = pkg._native.lib()
    m = 3 if name == "rand4096" else 12                           # 3: seeds of 50 to 90 rows on 4096 random bases
    skipped = {}
    for occ in (1, 5, 3000):
        for flags in (0, BOTH | SPLIT):
            _check(pkg, ix, ref, reads, flags, m, (name, occ, flags), max_occ=occ)
        skipped[occ] = int(MM.call(lib, ix, 0, *MS.csr(reads), m, occ, rows=False)[3][1])
    assert skipped[1] >= skipped[5] > skipped[3000] >= 0
    if name == "rand4096":
        assert skipped[3000] == 0
        free = MM.sized_call(lib, ix, 0, *MS.csr(reads), m, 0)
        deep = MM.sized_call(lib, ix, 0, *MS.csr(reads), m, 3000)
        assert all(np.array_equal(x, y) for x, y in zip(free, deep))


# ------------------------------------------------------------------ capacity
@pytest.mark.parametrize("flags", [0, BOTH | SPLIT])
def test_rows_past_the_capacity_are_dropped(pkg, flags):
    name = "tandem7"
    ref = FAMILY[name]
    ix = _index(pkg, name)
    reads = _reads(name)
    lib = pkg._native.lib()
    bases, offs = MS.csr(reads)
    w_off, w_rows, w_st, _ = MM.expected(ref, reads, flags, 20)
    total = w_rows.shape[0]
    assert total > 1000
    for cap in (0, 1, 63, total // 2, total - 1, total, total + 5):
        off, rows, st, tt = MM.call(lib, ix, flags, bases, offs, 20, cap=cap, spare=70, fill=-9)
        held = min(cap, total)
        assert np.array_equal(off, w_off) and off[-1] == total and tt[0] == total, cap      # the true total
        assert np.array_equal(rows[:held], w_rows[:held]), cap
        assert (rows[held:] == -9).all(), cap                       # nothing past 4 * out_cap_rows ints, nothing past the total


# ------------------------------------------------------------------ consequence 2: the SMEM rows
@pytest.mark.parametrize("name", ["rand4096", "tandem7", "noT"])
def test_every_smem_occurrence_is_a_mem(pkg, name):
    ref = FAMILY[name]
    ix = _index(pkg, name)
    reads = _reads(name)
    sa = U.suffix_rows(ref)
    bases, offs = MS.csr(reads)
    seen = 0
    for flags in FLAGS:
        both, split = bool(flags & BOTH), bool(flags & SPLIT)
        for m in (5, 20):
            off, rows, st, skipped = (t.cpu().numpy() if hasattr(t, "cpu") else t for t in ix.find_mems(bases, offs, m, both, split))
            s_off, s_rows, s_st = (t.cpu().numpy() for t in ix.find_smems_long("bwa", bases, offs, m, both_strands=both,
                                                                                split_breaks=split))
            assert np.array_equal(st, s_st) and skipped == 0
            for q in range(len(off) - 1):
                have = set(map(tuple, rows[off[q]:off[q + 1]].tolist()))
                for s, e, lo, hi in s_rows[s_off[q]:s_off[q + 1]].tolist():
                    assert e - s >= m
                    for r in range(lo, hi + 1):
                        assert (s, e, int(sa[r]) + 1, r) in have, (name, flags, m, q, s, e, r)
                        seen += 1
    assert seen > 100


# ------------------------------------------------------------------ offsets, empty batches
def test_lead_and_tail_bytes_belong_to_no_read(pkg):
    name = "rand4096"
    ref = FAMILY[name]
    ix = _index(pkg, name)
    reads = _reads(name)[:12]
    for flags in FLAGS:
        plain = _check(pkg, ix, ref, reads, flags, 12, ("plain", flags))
        moved = _check(pkg, ix, ref, reads, flags, 12, ("moved", flags), lead=300, tail=77)
        assert all(np.array_equal(x, y) for x, y in zip(plain, moved))


@pytest.mark.parametrize("flags", [0, BOTH])
def test_reads_of_very_different_lengths(pkg, flags):
    """A position finds its strand-read by a guess from v / positions and a gallop from there: one long read in front of,
    behind and between hundreds of reads of 0 to 3 bases puts the guess far off on either side."""
    name = "rand4096"
    ref = FAMILY[name]
    ix = _index(pkg, name)
    rng = np.random.default_rng(23)
    tiny = [ref[s:s + int(rng.integers(0, 4))].copy() for s in rng.integers(0, 4000, 300)]
    long_ = np.concatenate([ref[100:1500], ref[90:700]]).astype(np.uint8)
    for reads in ([long_] + tiny, tiny + [long_], tiny[:150] + [long_] + tiny[150:] + [long_[:999]]):
        off, rows = _check(pkg, ix, ref, reads, flags, 2, ("lengths", flags))
        assert rows.shape[0] > 1000


def test_no_reads_no_bases_and_bad_offsets(pkg):
    lib = pkg._native.lib()
    ix = _index(pkg, "rand4096")
    ref = FAMILY["rand4096"]
    for flags in FLAGS:
        strands = 2 if flags & BOTH else 1
        off, rows, st, tt = MM.call(lib, ix, flags, np.zeros(0, np.uint8), [0], 5, cap=4, fill=-9)
        assert off.tolist() == [0] and tt.tolist() == [0, 0] and st.size == 0 and (rows == -9).all()
        off, rows, st, tt = MM.call(lib, ix, flags, np.full(9, 2, np.uint8), [4], 1, cap=4, fill=-9)      # bases of no read
        assert off.tolist() == [0] and tt.tolist() == [0, 0] and (rows == -9).all()
        off, rows, st, tt = MM.call(lib, ix, flags, np.zeros(0, np.uint8), [0, 0, 0], 1, cap=4, fill=-9)   # empty reads only
        assert off.tolist() == [0] * (2 * strands + 1) and st.tolist() == [0] * (2 * strands) and tt.tolist() == [0, 0]
        assert (rows == -9).all()
        reads = [ref[:300].copy(), ref[500:900].copy()]
        bases, offs = MS.csr(reads)
        for bad in ([0, 400, 300], [0, 300, 701], [-1, 300, 700]):
            assert MM.call(lib, ix, flags, bases, bad, 5, max_len=400, want_rc=-1) is None
        assert MM.call(lib, ix, flags, bases, offs, 5, max_len=399, want_rc=-1) is None      # a read above max_len
        _check(pkg, ix, ref, reads, flags, 5, ("after bad offsets", flags))                   # and the next call is fine


# ------------------------------------------------------------------ wide intervals in many waves at once
def test_wide_seed_intervals_in_many_waves(pkg):
    name = "tandem7"
    ref = FAMILY[name]
    ix = _index(pkg, name)
    rng = np.random.default_rng(17)
    reads = []
    for i in range(300):
        s = int(rng.integers(0, len(ref) - 150))
        r = ref[s:s + 150].copy()
        if i % 2:
            at = int(rng.integers(0, 150))
            r[at] = (r[at] + 1 + rng.integers(0, 3)) & 3
        reads.append(r)
    off, rows = _check(pkg, ix, ref, reads, 0, 20, name)
    per_start = np.bincount(np.repeat(np.arange(300), np.diff(off))[rows[:, 0] == 0], minlength=300)
    assert (per_start > 64).sum() > 200                           # position 0 of a read: every row of its seed is left-maximal
    _check(pkg, ix, ref, reads[:60], BOTH | SPLIT, 33, name)


# ------------------------------------------------------------------ the Python layer
def test_python_layer_on_strings_and_codes(pkg):
    ref = FAMILY["rand4096"]
    m = pkg.ExactMatch("find_mems.fa")
    m.set_reference("".join("ACGT"[c] for c in ref))
    sm = pkg.SMEM(m, 4)
    reads = [ref[10:60].copy(), np.zeros(0, np.uint8), ref[4000:].copy(), MS.window_reads(ref)[2]]
    strs = ["".join("ACGT"[c] for c in r) for r in reads]
    for both in (False, True):
        want = MM.expected(ref, reads, BOTH if both else 0, 12)
        for given in (strs, MS.csr(reads)):
            off, rows, st, skipped = sm.find_mems(given, 12, both_strands=both)
            assert skipped == 0 and rows.dtype.is_floating_point is False and rows.shape[1] == 4
            assert all(np.array_equal(x.cpu().numpy(), y) for x, y in zip((off, rows, st), want))
    # a hint that is too small: the call is made again with room
    ix = sm.matcher.index(sm.lut.lut_size)
    want = MM.expected(ref, reads, 0, 3)
    assert want[1].shape[0] > 100
    off, rows, st, skipped = ix.find_mems(*MS.csr(reads), 3, rows_hint=7)
    assert all(np.array_equal(x.cpu().numpy(), y) for x, y in zip((off, rows, st), want))
    # max_occ through the wrapper, strings with N through encode_lenient
    want = MM.expected(ref, reads, 0, 3, 60)
    off, rows, st, skipped = sm.find_mems(strs, 3, max_occ=60)
    assert skipped == want[3] > 0 and np.array_equal(rows.cpu().numpy(), want[1])
    with_n = [strs[0][:20] + "N" + strs[0][20:], "N", "", "ANNT"]
    codes = [np.asarray(m.encode_lenient(s), np.uint8) for s in with_n]
    got = sm.find_mems(with_n, 12, split_breaks=True)
    assert all(np.array_equal(x.cpu().numpy(), y) for x, y in zip(got[:3], MM.expected(ref, codes, SPLIT, 12)))
