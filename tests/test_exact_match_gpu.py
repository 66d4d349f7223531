"""GPU: genie_exact_match (suffix-array intervals of CSR patterns of any length, one lane per pattern, on one strand or both)
against the brute force of tests/lookup_util.py through its restatement tests/exact_match_util.py, on every index of
test_lookups_gpu.index_specs(); byte for byte against genie_sa_interval on the same patterns padded into a matrix and
against the call without BOTH_STRANDS on the explicit interleaved batch; patterns longer than 8192 bases against
bytes.find; bad offsets; the Python layers.  Every comparison is on integers and exact.

As in test_lookups_gpu, a test first works out from the brute-force answers alone what it is about to ask and asserts that
the classes of patterns it exists for are not empty."""
import functools

import numpy as np
import pytest

import exact_match_calls as EC
import exact_match_util as EM
import lookup_util as U
from test_lookups_gpu import SPECS, _build, _spec_id

pytestmark = pytest.mark.gpu

FAMILY = U.family()
BOTH = EM.BOTH
N_FAMILY = 4096
N_RC = 1024
INVALID = -1


@pytest.fixture(scope="module")
def pkg():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import genie_smem_amd as g
    g._native.lib()
    return g


@functools.lru_cache(maxsize=None)
def _rows(name):
    return U.suffix_rows(FAMILY[name])


def _bad_at(p, at):
    p = p.copy()
    p[at] = 7
    return p


def family_plan(name, P, P2, seed):
    """-> (patterns, expected lohi / counts / status on one strand): lookup_util.patterns for this index -- every length
    0 .. P2 + 34, 63 / 64 / 65, 95 / 96 / 97, 150, 1000, patterns longer than the reference and running off its end -- then one
    pattern with a code > 3 at its last base and one at its first."""
    ref, rows = FAMILY[name], _rows(name)
    n = len(ref)
    pats = U.patterns(name, ref, P, P2, N_FAMILY, seed)
    base = next(p for p in pats if len(p) == 20)
    pats = pats + [_bad_at(base, 19), _bad_at(base, 0)]
    want = EM.expected(ref, pats, 0, rows)
    cnt, plen = want[1][:N_FAMILY], np.asarray([len(p) for p in pats[:N_FAMILY]])
    # the classes sa_plan asserts, from the brute-force answers alone
    assert (cnt == 0).any(), "no absent pattern"
    assert (cnt == 1).any(), "no pattern with one row"
    assert any(U.runs_off_end(ref, p) for p in pats), "no pattern that runs off the end of the reference"
    assert (plen > n).any() or n > 1000, "no pattern longer than the reference"
    if n + 1 > 32:
        assert (cnt > 32).any(), "no pattern with more than 32 rows"
    if name == "tandem1":
        assert ((plen > P) & (cnt > 2000)).any()
    assert set(U.pattern_lengths(P, P2)) <= set(plen.tolist())
    assert want[2][-2:].tolist() == [EM.READ_BAD_BASE] * 2 and not want[2][:-2].any() and (want[0][-2:] == -2).all()
    return pats, want


def _assert_same(got, want, pats, what):
    for g, w, field in zip(got, want, ("lohi", "counts", "status")):
        bad = np.nonzero((g.reshape(len(w), -1) != w.reshape(len(w), -1)).any(1))[0]
        assert g.shape == w.shape and not len(bad), (what, field, [(i, np.asarray(pats[i]).tolist()[:80], g[i].tolist(), w[i].tolist())
                                                                for i in bad[:3]])


# ------------------------------------------------------------------ the family, one strand
@pytest.mark.parametrize("spec", SPECS, ids=_spec_id)
def test_family_against_brute_force(pkg, spec):
    name, P, bits, fmt = spec
    ix, P2 = _build(pkg, name, P, bits, fmt)
    pats, want = family_plan(name, P, P2, SPECS.index(spec))
    ix.to("cuda")
    bases, offs = EM.csr(pats, lead=13, tail=29, fill=9)             # junk in front of off[0] and behind off[N]
    assert offs[0] > 0 and offs[-1] < bases.size
    _assert_same(EC.call(pkg._native.lib(), ix, 0, bases, offs), want, pats, spec)
    # byte for byte what genie_sa_interval writes for the same patterns padded into a matrix
    mat, lens = U.pack_rows(pats, fill=9)
    lohi = ix.exact_match(bases, offs)[0]
    assert lohi.cpu().numpy().tobytes() == ix.sa_interval(mat, lens).cpu().numpy().tobytes()


# ------------------------------------------------------------------ both strands
def strands_plan(name, P, P2, seed):
    """The family's patterns followed by the reverse complements of the first N_RC of them (the reverse complement of a cut
    of a random reference practically never occurs: without these, strand 1 would hold next to no hit), and the two bad
    patterns.  -> (patterns, expected with BOTH)."""
    ref, rows = FAMILY[name], _rows(name)
    n = len(ref)
    fam, _ = family_plan(name, P, P2, seed)
    pats = fam[:N_FAMILY] + [EM.rc(p) for p in fam[:N_RC]] + fam[N_FAMILY:]
    want = EM.expected(ref, pats, BOTH, rows)
    cnt1, plen = want[1][1::2], np.asarray([len(p) for p in pats])
    if n >= 300:                                                     # as sa_plan: a shorter reference has no such pattern
        assert ((plen > P + 32) & (cnt1 > 0)).any(), "strand 1 holds no present pattern longer than P + 32"
    if U.is_tandem(name):
        assert ((plen > P + 32) & (cnt1 > 100)).any(), "strand 1 holds no pattern of more than 100 rows"
    assert (cnt1 > 0).any() and (cnt1 == 0).any()
    # a code > 3 is bad on both strands
    assert want[2][-4:].tolist() == [EM.READ_BAD_BASE] * 4 and (want[0][-4:] == -2).all() and not want[1][-4:].any()
    return pats, want


@pytest.mark.parametrize("spec", SPECS, ids=_spec_id)
def test_both_strands(pkg, spec):
    name, P, bits, fmt = spec
    lib = pkg._native.lib()
    ix, P2 = _build(pkg, name, P, bits, fmt)
    pats, want = strands_plan(name, P, P2, SPECS.index(spec))
    ix.to("cuda")
    bases, offs = EM.csr(pats, lead=5, tail=3)
    got = EC.call(lib, ix, BOTH, bases, offs)
    _assert_same(got, want, EM.strand_patterns(pats, 2), spec)
    # byte for byte the call without the flag on the explicit interleaved batch
    one = EC.call(lib, ix, 0, *EM.csr(EM.strand_patterns(pats, 2), lead=1))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, one))
    if name == "noT":                                                # a pattern of A's: TTTT on strand 1, absent and no bad base
        lohi, cnt, st = EC.call(lib, ix, BOTH, np.zeros(4, np.uint8), [0, 4])
        assert lohi[0, 0] >= 0 and cnt[0] > 0 and lohi[1].tolist() == [-1, -1] and cnt[1] == 0 and st.tolist() == [0, 0]


# ------------------------------------------------------------------ at most 64 bases: every lane packs its own pattern
DIRECT = 64                  # kEmDirect: up to this max_len there is no pack stage


def short_plan(name, P, P2, seed):
    """The family's patterns of at most DIRECT bases, the reverse complements of the first N_RC of them and the two bad
    patterns -> (patterns, expected with BOTH).  Lengths 0, 1, 31 .. 33 and 63 / 64: both words, full and not."""
    ref, rows = FAMILY[name], _rows(name)
    fam, _ = family_plan(name, P, P2, seed)
    short = [p for p in fam[:N_FAMILY] if len(p) <= DIRECT]
    pats = short + [EM.rc(p) for p in short[:N_RC]] + fam[N_FAMILY:]
    want = EM.expected(ref, pats, BOTH, rows)
    plen = np.asarray([len(p) for p in pats])
    assert plen.max() == DIRECT and {0, 1, 31, 32, 33, 63, 64} <= set(plen.tolist()) and len(short) > 2000
    cnt0, cnt1 = want[1][0::2], want[1][1::2]
    if len(ref) >= 300:                                              # hits that need the second word, on either strand
        assert ((plen > 32) & (cnt0 > 0)).any() and ((plen > 32) & (cnt1 > 0)).any()
    assert (cnt0 == 0).any() and (cnt1 == 0).any() and want[2][-4:].tolist() == [EM.READ_BAD_BASE] * 4
    return pats, want


@pytest.mark.parametrize("spec", SPECS, ids=_spec_id)
def test_short_patterns_without_the_pack_stage(pkg, spec):
    name, P, bits, fmt = spec
    lib = pkg._native.lib()
    ix, P2 = _build(pkg, name, P, bits, fmt)
    pats, want = short_plan(name, P, P2, SPECS.index(spec))
    ix.to("cuda")
    bases, offs = EM.csr(pats, lead=11, tail=2)
    got = EC.call(lib, ix, BOTH, bases, offs)                         # max_len = 64
    _assert_same(got, want, EM.strand_patterns(pats, 2), spec)
    # a larger bound takes the same patterns through the packed stream: the same bytes
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, EC.call(lib, ix, BOTH, bases, offs, max_len=DIRECT + 1)))
    # one strand, on the interleaved batch and against genie_sa_interval
    both = EM.strand_patterns(pats, 2)
    one = EC.call(lib, ix, 0, *EM.csr(both, lead=1))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, one))
    mat, lens = U.pack_rows(both, fill=9)
    assert one[0].tobytes() == ix.sa_interval(mat, lens).cpu().numpy().tobytes()
    # one pattern of 65 bases more: the batch goes through the packed stream
    longer = pats + [np.concatenate([pats[int(np.argmax([len(p) for p in pats]))], [1]]).astype(np.uint8)]
    _assert_same(EC.call(lib, ix, BOTH, *EM.csr(longer)), EM.expected(FAMILY[name], longer, BOTH, _rows(name)),
                 EM.strand_patterns(longer, 2), (spec, "65"))


# ------------------------------------------------------------------ call geometries
GEOMETRY_SPECS = [SPECS[i] for i in (len(SPECS) - 2, SPECS.index(("tandem7", 7, 9, "wide")), SPECS.index(("tail_AAAAAAAA", 3, 0, "auto")))]


@pytest.mark.parametrize("spec", GEOMETRY_SPECS, ids=_spec_id)
def test_call_geometries(pkg, spec):
    name, P, bits, fmt = spec
    lib = pkg._native.lib()
    ref, rows = FAMILY[name], _rows(name)
    ix, P2 = _build(pkg, name, P, bits, fmt)
    fam, _ = family_plan(name, P, P2, SPECS.index(spec))
    ix.to("cuda")
    rng = np.random.default_rng(5)
    empty = np.zeros(0, np.uint8)
    batches = {}
    for n in (1, 63, 64, 65, 257):
        pick = rng.choice(N_FAMILY, n, replace=False)
        batches[f"N={n}"] = [fam[i] for i in pick]
    some = [fam[i] for i in rng.choice(N_FAMILY, 70, replace=False)]
    batches["empty runs"] = [empty] * 3 + some[:35] + [empty] * 66 + some[35:] + [empty] * 2
    batches["only empty"] = [empty] * 65
    batches["short, empty runs"] = [p for p in batches["empty runs"] if len(p) <= DIRECT]      # max_len <= 64: no pack stage
    batches["short N=65"] = [p[:DIRECT] for p in batches["N=65"]]
    batches["N=1 empty"] = [empty]
    for what, pats in batches.items():
        for flags in (0, BOTH):
            want = EM.expected(ref, pats, flags, rows)
            bases, offs = EM.csr(pats, lead=0 if what == "only empty" else 7)
            _assert_same(EC.call(lib, ix, flags, bases, offs), want, EM.strand_patterns(pats, 2 if flags else 1), (spec, what, flags))
    n = len(ref)
    for flags in (0, BOTH):
        strands = 2 if flags else 1
        # total_bases = 0 with N > 0: a null d_bases, empty patterns only
        lohi, cnt, st = EC.call(lib, ix, flags, empty, [0] * 6, total=0)
        assert (lohi == [0, n]).all() and (cnt == n + 1).all() and not st.any() and len(cnt) == 5 * strands
        # N = 0 writes nothing
        lohi, cnt, st = EC.call(lib, ix, flags, np.full(9, 2, np.uint8), [4])
        assert lohi.shape == (0, 2) and cnt.size == 0 and st.size == 0
        assert EC.call(lib, ix, flags, empty, [0])[0].shape == (0, 2)
        # d_counts and / or d_status NULL
        pats = batches["N=65"]
        want = EM.expected(ref, pats, flags, rows)
        bases, offs = EM.csr(pats, lead=3)
        for counts, status in ((False, True), (True, False), (False, False)):
            got = EC.call(lib, ix, flags, bases, offs, counts=counts, status=status)
            assert np.array_equal(got[0], want[0])
            assert (got[1] is None) == (not counts) and (counts is False or np.array_equal(got[1], want[1]))
            assert (got[2] is None) == (not status) and (status is False or np.array_equal(got[2], want[2]))


# ------------------------------------------------------------------ longer than 8192 bases
def _long_refs():
    rand = np.random.default_rng(401).integers(0, 4, 12_000).astype(np.uint8)
    tandem = np.tile(U._codes("GATTACA"), 20_000 // 7 + 1)[:20_000].copy()
    tandem[15_000] = (tandem[15_000] + 2) & 3
    return {"rand12000": rand, "tandem20000": tandem}


LONG_COUNTS = {"rand12000": [1, 1, 1, 1, 0], "tandem20000": [973, 973, 715, 1, 0]}      # worked out on the CPU beforehand


@pytest.mark.parametrize("name", ["rand12000", "tandem20000"])
def test_patterns_longer_than_8192(pkg, name):
    ref = _long_refs()[name]
    n = len(ref)
    rng = np.random.default_rng(n)
    cuts = []
    for L in (8192, 8193, 10_000, n, n + 1):
        cuts.append(np.concatenate([ref[:L], rng.integers(0, 4, max(L - n, 0)).astype(np.uint8)]))
    changed = []
    for c in cuts:
        c = c.copy()
        c[-1] = (c[-1] + 1 + rng.integers(0, 3)) & 3
        changed.append(c)
    pats = cuts + changed
    occ = [EM.occurrences(ref, p) for p in pats]
    assert [len(o) for o in occ[:5]] == LONG_COUNTS[name] and not any(occ[5:])
    assert [len(p) for p in cuts] == [8192, 8193, 10_000, n, n + 1]
    ix = pkg.GenieIndex.build(ref, 0).to("cuda")
    for both in (False, True):
        batch = pats + ([EM.rc(p) for p in pats] if both else [])
        strand = EM.strand_patterns(batch, 2 if both else 1)
        occ = [EM.occurrences(ref, p) for p in strand]
        if both:                                                     # strand 1 of rc(p) is p: hits on strand 1 as well
            assert sum(len(o) > 0 for o in occ[1::2]) >= 4
        lohi, cnt, st = ix.exact_match(*EM.csr(batch, lead=2), both_strands=both, counts=True)
        assert cnt.cpu().numpy().tolist() == [len(o) for o in occ] and not st.cpu().numpy().any()
        off, pos = ix.locate(lohi, sort=True)
        off, pos = off.cpu().numpy(), pos.cpu().numpy()
        assert off.tolist() == np.concatenate([[0], np.cumsum([len(o) for o in occ])]).tolist()
        assert pos.tolist() == [s + 1 for o in occ for s in o]


# ------------------------------------------------------------------ bad offsets
def test_bad_offsets_and_the_call_after(pkg):
    lib = pkg._native.lib()
    name = "rand4096"
    ref, rows = FAMILY[name], _rows(name)
    ix = pkg.GenieIndex.build(ref, 0, dir_bits=7).to("cuda")
    pats = [ref[:300].copy(), ref[500:900].copy()]
    bases, offs = EM.csr(pats)
    for flags in (0, BOTH):
        for bad in ([0, 400, 300], [0, 300, 701], [-1, 300, 700]):   # decreasing; beyond total_bases; below 0
            assert EC.call(lib, ix, flags, bases, bad, max_len=400, want_rc=INVALID) is None
        assert EC.call(lib, ix, flags, bases, offs, max_len=399, want_rc=INVALID) is None      # a pattern above max_len
        want = EM.expected(ref, pats, flags, rows)
        _assert_same(EC.call(lib, ix, flags, bases, offs), want, pats, "after bad offsets")


# ------------------------------------------------------------------ the Python layers
def _str(codes):
    return "".join("ACGTN"[min(int(c), 4)] for c in codes)


def _matcher(pkg, ref, fname):
    m = pkg.ExactMatch(fname)
    m.set_reference(_str(ref))
    return m


def test_exact_match_batch_on_a_ragged_list(pkg):
    name = "tandem7"
    ref, rows = FAMILY[name], _rows(name)
    m = _matcher(pkg, ref, "exact_match_ragged.fa")
    fam, _ = family_plan(name, 7, 8, 3)
    long = np.tile(ref[:7], 9000 // 7 + 1)[:9000]                    # 9000 bases: longer than GENIE_MAX_READ_LEN and than the reference
    pats = fam[:300:7] + [long, np.zeros(0, np.uint8), ref[:1400].copy(), ref.copy()]
    assert len(long) > pkg._native.MAX_READ_LEN and len({len(p) for p in pats}) > 20
    want = EM.expected(ref, pats, 0, rows)
    assert (want[1] > 100).any() and (want[1] == 0).any()
    got = m.exact_match_batch([_str(p) for p in pats])
    assert got.dtype == np.int32 and np.array_equal(got, want[0])
    assert m.exact_match_positions_batch([_str(p) for p in pats]) == [sorted(U.positions(rows, lo, hi)) for lo, hi in want[0].tolist()]
    assert m.exact_match_batch([]).shape == (0, 2) and m.exact_match_positions_batch([]) == []


def test_exact_match_text_in_three_formats(pkg):
    name = "rand4096"
    ref, rows = FAMILY[name], _rows(name)
    m = _matcher(pkg, ref, "exact_match_text.fa")
    flagged = np.concatenate([ref[100:130], [4], ref[131:150]]).astype(np.uint8)          # one pattern with an N
    pats = [ref[10:200].copy(), ref[100:150].copy(), flagged, ref[100:150].copy(), EM.rc(ref[3000:3100]), ref[4000:].copy(),
            np.asarray([0, 1, 2, 3] * 5, np.uint8)]
    seqs = [_str(p) for p in pats]
    assert "N" in seqs[2] and not any("N" in s for i, s in enumerate(seqs) if i != 2)
    texts = {"lines": "".join(s + "\n" for s in seqs),
             "fastq": "".join("@p%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for i, s in enumerate(seqs)),
             "fasta": "".join(">p%d\n%s" % (i, "".join(s[j:j + 60] + "\n" for j in range(0, len(s), 60))) for i, s in enumerate(seqs))}
    ix = m.index(0)
    for both in (False, True):
        want = EM.expected(ref, pats, BOTH if both else 0, rows)
        assert want[2].tolist() == ([0, 0, 0, 0, 1, 1] + [0] * 8 if both else [0, 0, 1, 0, 0, 0, 0])
        assert want[1][0] > 0 and (not both or want[1][9] > 0)        # rc(ref[3000:3100]) hits on strand 1
        arrays = [t.cpu().numpy() for t in ix.exact_match(*EM.csr(pats), both_strands=both, counts=True)]
        _assert_same(arrays, want, EM.strand_patterns(pats, 2 if both else 1), "arrays")
        for fmt, text in texts.items():
            lohi, cnt, st, offs = m.exact_match_text(text.encode(), fmt, both_strands=both)
            assert np.array_equal(offs.cpu().numpy(), EM.csr(pats)[1]), fmt
            assert all(np.array_equal(x.cpu().numpy(), y) for x, y in zip((lohi, cnt, st), arrays)), fmt


# ------------------------------------------------------------------ an image built on the device
def test_on_a_device_built_image(pkg):
    spec = ("rand4096", 7, 0, "auto")
    name, P, bits, fmt = spec
    _, P2 = _build(pkg, name, P, bits, fmt)
    pats, want = strands_plan(name, P, P2, SPECS.index(spec))
    ix = pkg.GenieIndex.build_on_device(FAMILY[name], 0, dir_bits=P, table_bits=bits, table_format=fmt)
    got = [t.cpu().numpy() for t in ix.exact_match(*EM.csr(pats, lead=3), both_strands=True, counts=True)]
    _assert_same(got, want, EM.strand_patterns(pats, 2), "device-built image")
