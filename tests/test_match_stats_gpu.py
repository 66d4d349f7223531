"""GPU tests of genie_match_stats (run with -m gpu on an MI355X): the matching statistics of every read position and their
suffix-array intervals.  Every comparison is exact: against the brute force of tests/match_stats_util.py on every reference
of lookup_util.family() in both forms of the match table, against the call without BOTH_STRANDS on the explicit interleaved
batch, against genie_find_smems_long and genie_sa_interval at a size the brute force cannot reach, on guarded buffers
(tests/guarded.py), and through the Python layer."""
import ctypes as C

import numpy as np
import pytest

import lookup_util as U
import match_stats_util as MS
import smem_util as SM

pytestmark = pytest.mark.gpu

BOTH, SPLIT = MS.BOTH, MS.SPLIT
FAMILY = U.family()
FORMS = ["compact", "wide"]
KNOBS = [(7, 0), (3, 4)]                                      # (dir_bits, table_bits): the automatic P2 = 8, and a key of 4 bases


@pytest.fixture(scope="module")
def pkg():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import genie_smem_amd as g
    g._native.lib()
    return g


def _index(pkg, name, form, knobs=KNOBS[0]):
    return pkg.GenieIndex.build(FAMILY[name], 0, dir_bits=knobs[0], table_bits=knobs[1], table_format=form).to("cuda")


def _check(pkg, ix, ref, reads, flags, tag, lead=0, tail=0, ws_mult=1):
    """The call with and without d_lohi against the restated specification; returns (ms, lohi, status)."""
    lib = pkg._native.lib()
    bases, offs = MS.csr(reads, lead, tail)
    want = MS.expected(ref, reads, flags, lead, tail)
    ms, lohi, st = MS.call(lib, ix, flags, bases, offs, ws_mult=ws_mult)
    assert np.array_equal(st, want[2]), (tag, "status")
    assert np.array_equal(ms, want[0]), (tag, "ms", np.flatnonzero(ms != want[0])[:5])
    assert np.array_equal(lohi, want[1]), (tag, "lohi", np.flatnonzero((lohi != want[1]).any(1))[:5])
    ms2, none, st2 = MS.call(lib, ix, flags, bases, offs, intervals=False, fill=-3, ws_mult=ws_mult)
    assert none is None and np.array_equal(ms2, ms) and np.array_equal(st2, st), (tag, "lengths only")
    return ms, lohi, st


def _batches(name):
    b = SM.batches(name)
    shorts = [r for L in SM.SHORT_LENGTHS if L <= 17 or L in (31, 32, 33, 64) for r in b["short"][L]]
    mids = [r for L in SM.MID_LENGTHS for r in b["mid"][L]]
    return [("ragged", b["ragged"]), ("short", shorts), ("mid", mids), ("long", b["long"]), ("windows", MS.window_reads(FAMILY[name]))]


# ------------------------------------------------------------------ brute-force parity
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", list(FAMILY))
def test_every_position_against_brute_force(pkg, name, form):
    ref = FAMILY[name]
    positions = matched = 0
    for knobs in KNOBS:
        ix = _index(pkg, name, form, knobs)
        for label, reads in _batches(name):
            for flags in (0, SPLIT):
                ms, lohi, st = _check(pkg, ix, ref, reads, flags, (name, form, knobs, label, flags))
                positions += ms.size
                matched += int(((ms > 0) & (lohi[:, 0] >= 0)).sum())
    # the batches are the size they are meant to be: the long one alone holds ten reads at least, and it ran four times
    assert positions >= 4 * 10 * SM.LONG_LENGTH and matched > positions // 2


# ------------------------------------------------------------------ breaks
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["rand4096", "noT", "tandem7", "tail_AAAAAAAA", "rand5"])
def test_breaks_with_and_without_split(pkg, name, form):
    ref = FAMILY[name]
    ix = _index(pkg, name, form)
    reads = MS.break_reads(ref)
    for flags in (0, SPLIT, BOTH, BOTH | SPLIT):
        ms, lohi, st = _check(pkg, ix, ref, reads, flags, (name, form, flags), lead=3, tail=70)
        strands = 2 if flags & BOTH else 1
        if flags & SPLIT:
            assert not st.any() and (ms >= 0).all()
        else:
            sreads = MS.strand_reads(reads, strands)
            at = strands * 3
            for q, r in enumerate(sreads):                        # flagged strand-reads hold their defined values
                if (r > 3).any():
                    assert st[q] == MS.READ_BAD_BASE and (ms[at:at + len(r)] == -1).all() and (lohi[at:at + len(r)] == -1).all()
                at += len(r)
            assert {0, 1} <= set(st.tolist())
    if name == "noT":
        assert 3 in MS.expected(ref, reads, 0)[2]


@pytest.mark.parametrize("flags", [SPLIT, BOTH | SPLIT])
def test_more_units_than_the_workspace_holds(pkg, flags):
    """One break in every five positions: the segments outnumber the strand-reads plus one unit per 32 positions, so the exact
    workspace takes several unit passes; a roomy one takes a single pass and gives the same bytes."""
    name = "rand4096"
    ref = FAMILY[name]
    ix = _index(pkg, name, "compact")
    rng = np.random.default_rng(5)
    reads = []
    for i in range(3):
        r = np.concatenate([ref[100 * i:100 * i + 2000], ref[:1200]]).astype(np.uint8)
        r[rng.random(r.size) < 0.2] = 4
        reads.append(r)
    strands = 2 if flags & BOTH else 1
    good = np.concatenate([r < 4 for r in reads])
    units = strands * int(np.count_nonzero(np.diff(np.concatenate([[0], good.astype(np.int8)])) == 1))
    held = strands * len(reads) + strands * sum(len(r) for r in reads) // 32
    assert units > 2 * held
    exact = _check(pkg, ix, ref, reads, flags, ("passes", flags))
    roomy = _check(pkg, ix, ref, reads, flags, ("one pass", flags), ws_mult=8)
    assert all(np.array_equal(x, y) for x, y in zip(exact, roomy))


# ------------------------------------------------------------------ both strands
@pytest.mark.parametrize("form", FORMS)
def test_both_strands_is_the_interleaved_batch(pkg, form):
    lib = pkg._native.lib()
    for name in ("rand4096", "noT", "tandem3"):
        ref = FAMILY[name]
        ix = _index(pkg, name, form)
        b = SM.batches(name)
        reads = b["ragged"] + b["mid"][705][:5] + b["long"][:2] + MS.break_reads(ref)
        for split in (0, SPLIT):
            got = MS.call(lib, ix, BOTH | split, *MS.csr(reads, 7, 5))
            want = MS.call(lib, ix, split, *MS.csr(MS.strand_reads(reads, 2), 14, 10))
            assert all(np.array_equal(x, y) for x, y in zip(got, want)), (name, form, split)
            _check(pkg, ix, ref, reads, BOTH | split, (name, form, split))


def test_no_reads_no_bases_and_bad_offsets(pkg):
    lib = pkg._native.lib()
    ix = _index(pkg, "rand4096", "compact")
    ref = FAMILY["rand4096"]
    for flags in (0, BOTH, SPLIT, BOTH | SPLIT):
        strands = 2 if flags & BOTH else 1
        ms, lohi, st = MS.call(lib, ix, flags, np.zeros(0, np.uint8), [0])
        assert ms.size == 0 and lohi.shape == (0, 2) and st.size == 0
        ms, lohi, st = MS.call(lib, ix, flags, np.full(9, 2, np.uint8), [4])      # bases that belong to no read
        assert (ms == 0).all() and ms.size == strands * 9 and (lohi == -1).all()
        ms, lohi, st = MS.call(lib, ix, flags, np.zeros(0, np.uint8), [0, 0, 0])   # empty reads only
        assert ms.size == 0 and st.tolist() == [0] * (2 * strands)
        reads = [ref[:300].copy(), ref[500:900].copy()]
        bases, offs = MS.csr(reads)
        for bad in ([0, 400, 300], [0, 300, 701], [-1, 300, 700]):
            assert MS.call(lib, ix, flags, bases, bad, max_len=400, want_rc=-1) is None
        assert MS.call(lib, ix, flags, bases, offs, max_len=399, want_rc=-1) is None   # a read above max_len
        _check(pkg, ix, ref, reads, flags, ("after bad offsets", flags))              # and the next call is fine


# ------------------------------------------------------------------ consistency at a size the brute force cannot reach
def test_consistent_with_find_smems_long_and_sa_interval(pkg):
    import torch
    from genie_smem_amd import synth
    N = pkg._native
    codes = synth.synth_ref(100_000, 100_000)
    ix = pkg.GenieIndex.build(codes, 15).to("cuda")
    rng = np.random.default_rng(11)
    pool = synth.reads_from_ref_fast(codes, 2000, 300, 4)
    reads = [pool[i].copy() for i in range(2000)]
    for i, L in enumerate((20_000, 20_000, 20_001)):
        s = int(rng.integers(0, len(codes) - L))
        r = codes[s:s + L].copy()
        hit = rng.random(L) < 0.002                               # substitutions: matches of a few hundred bases
        r[hit] = (r[hit] + 1 + rng.integers(0, 3, int(hit.sum()))) & 3
        reads.insert(700 * i, r)
    bases, offs = MS.csr(reads)
    ms, lohi, st = (t.cpu().numpy() for t in ix.match_stats(bases, offs))
    off, rows, st_long = (t.cpu().numpy() for t in ix.find_smems_long("bwa", bases, offs))
    assert not st.any() and np.array_equal(st, st_long)
    # every SMEM row is the matching statistic of its start
    at = np.repeat(offs[:-1], np.diff(off)) + rows[:, 0]
    assert rows.shape[0] > 4000
    assert np.array_equal(ms[at], rows[:, 1] - rows[:, 0])
    assert np.array_equal(lohi[at], rows[:, 2:])
    # a match shortened by its first base starts one position on
    inner = np.ones(ms.size, bool)
    inner[offs[1:-1] - 1] = False                                 # the last position of a read has no successor in it
    d = ms[1:] - ms[:-1]
    assert (d[inner[:-1]] >= -1).all()
    read_end = np.repeat(offs[1:], np.diff(offs))
    assert (ms >= 1).all() and (np.arange(ms.size) + ms <= read_end).all()
    # genie_sa_interval on a sample: the matched substring has lohi, the substring extended by one base occurs nowhere
    cand = np.flatnonzero(ms <= N.MAX_READ_LEN)
    pick = np.concatenate([rng.choice(cand, 3000, replace=False), cand[np.argsort(ms[cand])[-50:]]])
    longer = pick[pick + ms[pick] < read_end[pick]]
    longer = longer[ms[longer] + 1 <= N.MAX_READ_LEN]
    assert longer.size > 1000
    for pos, extra, want in ((pick, 0, lohi[pick]), (longer, 1, np.full((longer.size, 2), -1, np.int32))):
        lens = (ms[pos] + extra).astype(np.int32)
        pats = np.zeros((pos.size, int(lens.max())), np.uint8)
        for j, (p, l) in enumerate(zip(pos.tolist(), lens.tolist())):
            pats[j, :l] = bases[p:p + l]
        got = ix.sa_interval(torch.as_tensor(pats).cuda(), torch.as_tensor(lens).cuda()).cpu().numpy()
        assert np.array_equal(got, want), extra
    # lengths only, and both strands against the interleaved batch at this size
    ms2, none, _ = ix.match_stats(bases, offs, intervals=False)
    assert none is None and np.array_equal(ms2.cpu().numpy(), ms)
    sub = reads[:200] + [reads[700]]
    got = [t.cpu().numpy() for t in ix.match_stats(*MS.csr(sub), both_strands=True)]
    want = [t.cpu().numpy() for t in ix.match_stats(*MS.csr(MS.strand_reads(sub, 2)))]
    assert all(np.array_equal(x, y) for x, y in zip(got, want))


# ------------------------------------------------------------------ memory contract
@pytest.mark.parametrize("flags", [0, BOTH, SPLIT, BOTH | SPLIT])
def test_memory_contract(pkg, flags):
    import torch
    from guarded import POISONS, Arena
    import contract_calls as CC
    lib = pkg._native.lib()
    name = "noT"
    ref = FAMILY[name]
    ix = _index(pkg, name, "compact")
    b = SM.batches(name)
    reads = b["ragged"][:40] + MS.break_reads(ref) + b["mid"][705][:3] + MS.window_reads(ref)
    want = MS.expected(ref, reads, flags, 77, 13)
    for intervals, status in ((True, True), (False, True), (True, False)):
        results = []
        for poison in POISONS:
            a = Arena("cuda", poison)
            a.freeze(ix.blob, "index image")
            call = MS.guarded_call(lib, ix, a, torch.cuda.current_stream().cuda_stream, flags, reads, 77, 13, intervals, status)
            torch.cuda.synchronize()
            res = call.result()
            a.check()
            a.check_frozen()
            results.append(res)
        for other in results[1:]:
            CC.same(results[0], other)
        assert np.array_equal(results[0]["ms"], want[0])
        if intervals:
            assert np.array_equal(results[0]["lohi"], want[1])
        if status:
            assert np.array_equal(results[0]["status"], want[2])


# ------------------------------------------------------------------ the Python layer
def _smem(pkg, ref_codes, fname):
    m = pkg.ExactMatch(fname)
    m.set_reference("".join("ACGT"[c] for c in ref_codes))
    return m, pkg.SMEM(m, 4)


def test_smem_match_stats_on_strings_and_codes(pkg):
    ref = FAMILY["rand4096"]
    m, sm = _smem(pkg, ref, "match_stats.fa")
    reads = SM.batches("rand4096")["mid"][256][:3] + [ref[10:60].copy(), np.zeros(0, np.uint8), ref[4000:].copy()]
    reads = [r for r in reads if not (r > 3).any()]
    strs = ["".join("ACGT"[c] for c in r) for r in reads]
    for both in (False, True):
        want = MS.expected(ref, reads, BOTH if both else 0)
        got_s = [t.cpu().numpy() for t in sm.match_stats(strs, both_strands=both)]
        got_c = [t.cpu().numpy() for t in sm.match_stats(MS.csr(reads), both_strands=both)]
        for got in (got_s, got_c):
            assert all(np.array_equal(x, y) for x, y in zip(got, want))
    ms, lohi, st = sm.match_stats(strs, intervals=False)
    assert lohi is None and np.array_equal(ms.cpu().numpy(), MS.expected(ref, reads, 0)[0])
    # the per-query helper: forward_extension's longest match and its interval
    q, p = strs[3], 5
    matches, longest = sm.forward_extension(q, p)
    ms, lohi, st = (t.cpu().numpy() for t in sm.match_stats([q]))
    assert longest == q[p:p + ms[p]] and tuple(lohi[p]) == tuple(matches[longest])
    # strings with N: encode_lenient and breaks
    with_n = [strs[3][:20] + "N" + strs[3][20:], "N", "", "ANNT"]
    codes = [np.asarray(m.encode_lenient(s), np.uint8) for s in with_n]
    got = [t.cpu().numpy() for t in sm.match_stats(with_n, split_breaks=True)]
    assert all(np.array_equal(x, y) for x, y in zip(got, MS.expected(ref, codes, SPLIT)))


def test_match_stats_text_on_a_fastq_with_n(pkg):
    ref = FAMILY["rand4096"]
    m, sm = _smem(pkg, ref, "match_stats_text.fa")
    seqs = ["".join("ACGT"[c] for c in ref[100:400]), "N" + "".join("ACGT"[c] for c in ref[7:40]) + "NN" + "ACGTTGCA", "", "NNN",
            "".join("ACGT"[c] for c in ref[3000:3257])]
    text = "".join("@r%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for i, s in enumerate(seqs)).encode()
    codes = [np.asarray(m.encode_lenient(s), np.uint8) for s in seqs]
    for both in (False, True):
        ms, lohi, st, offs = sm.match_stats_text(text, "fastq", both_strands=both)
        want = MS.expected(ref, codes, SPLIT | (BOTH if both else 0))
        assert np.array_equal(offs.cpu().numpy(), MS.csr(codes)[1])
        assert all(np.array_equal(x.cpu().numpy(), y) for x, y in zip((ms, lohi, st), want))
    ms, lohi, st, offs = sm.match_stats_text(text, "fastq", intervals=False, split_breaks=False)
    want = MS.expected(ref, codes, 0)
    assert lohi is None and np.array_equal(ms.cpu().numpy(), want[0]) and np.array_equal(st.cpu().numpy(), want[2])
    assert st.cpu().numpy().tolist() == [0, 1, 0, 1, 0]
