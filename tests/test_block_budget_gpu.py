"""GPU: every kernel that reads the compact match table, on an image whose 65535 overflow blocks are used up
(tests/budget_util.py; the image itself is pinned by test_block_budget_host.py).  A P2-mer with 7 .. 13 suffixes that got no
block looks like a full six-key entry whose rows decide, although none of its suffixes is cut short; the reads here start at
such entries -- and at entries that did get a block, as the control -- exact or with one substitution inside the entry's key,
at its edge and past it.

Every expectation comes from the CPU oracle or from the host-built image, none from the library under test, and every
comparison is exact (offsets, rows, statuses, intervals, positions).  Each test first asserts, from the host image, that
its batch lands where it is meant to: every targeted read starts on its class of entries, every other batch has at least
5 % of its positions on starved entries."""
import ctypes as C

import numpy as np
import pytest

import budget_util as B
import smem_util as S

pytestmark = pytest.mark.gpu

MODES = [("bwa", 1), ("bwa", 12), ("lut", 1), ("rmi", 1)]
FIXED = ["fromref150", "fromref255", "random150", "starved150", "block150", "starved255", "block255"]
SHORT = FIXED + ["ragged"]
MID = ["mid705", "mid1409"]
TARGETED = list(B.TARGETED)


@pytest.fixture(scope="module")
def pkg():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import genie_smem_amd as g
    g._native.lib()
    return g


@pytest.fixture(scope="module")
def cls(pkg):
    return B.classes(pkg)


@pytest.fixture(scope="module")
def handles(pkg, oracle_mod):
    """(host-built index with a natively trained [10] model on the device, the oracle with the same model)."""
    B.image(pkg)                                              # the image without a model, before one is trained
    ix = pkg.GenieIndex.build(B.REF, B.K, **B.KNOBS)
    coefs, icpts, _, _, _ = ix.train_rmi([10])
    orc = B.oracle(oracle_mod)
    orc.set_rmi([10], coefs, icpts)
    return ix.to("cuda"), orc


@pytest.fixture(scope="module")
def ix(handles):
    return handles[0]


@pytest.fixture(scope="module")
def orc(handles):
    return handles[1]


@pytest.fixture(scope="module")
def dev(pkg):
    return pkg.GenieIndex.build_on_device(B.REF, B.K, **B.KNOBS)


def _covered(pkg, cls, label, reads=None):
    """The coverage condition of a batch, from the host image."""
    reads = B.batches(pkg)[label] if reads is None else reads
    if label in B.TARGETED:
        assert B.starts_on(cls.starved if B.TARGETED[label] == "starved" else cls.block, reads, cls.P2), label
    else:
        assert B.positions_on(cls.starved, reads, cls.P2) >= 0.05 * B.positions(reads), label
    return reads


_WANT = {}


def _want(pkg, orc, label, mode, min_len):
    key = (label, mode, min_len if mode == "bwa" else 1)
    if key not in _WANT:
        _WANT[key] = B.expected_batch(orc, B.batches(pkg)[label], mode, key[2])
    return _WANT[key]


def _find(h, label, reads, mode, min_len):
    """find_smems on a batch: a fixed-length one as a matrix, the ragged one with junk behind every read, the reads of
    705 bases and more through the same entry point."""
    if len({len(r) for r in reads}) == 1:
        return h.find_smems(mode, np.stack(reads), None, min_len)
    mat, lens = S.matrix(reads, max(len(r) for r in reads) + 3)
    return h.find_smems(mode, mat, lens, min_len)


# ------------------------------------------------------------------ 1. the device builder
def _same_image(pkg, codes, k, knobs, seed_table, want):
    import torch
    built = pkg.GenieIndex.build_on_device(codes, k, seed_table=seed_table, **knobs)
    got = built.blob.cpu().numpy()
    tag = (len(codes), k, knobs, seed_table)
    assert got.size == want.size, (tag, got.size, want.size, B.sections(got)[0]["ov_entries"], B.sections(want)[0]["ov_entries"])
    diff = np.flatnonzero(got != want)
    assert not len(diff), (tag, "first difference at byte", int(diff[0]), "section", B.section_of(want, int(diff[0])))
    what = C.c_uint32(77)
    with torch.cuda.device(built.device):
        rc = pkg._native.lib().genie_index_validate(built._h, C.byref(what), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert (rc, what.value) == (0, 0), tag


@pytest.mark.parametrize("seed_table", [True, False])
def test_device_build_is_byte_identical(pkg, cls, seed_table):
    assert int(cls.starved.sum()) >= 20_000 and int(cls.block.sum()) == B.MAX_BLOCKS
    _same_image(pkg, B.REF, B.K, B.KNOBS, seed_table, B.image(pkg, seed_table))


@pytest.mark.parametrize("seed_table", [True, False])
def test_device_build_without_dir16(pkg, seed_table):
    """70 000 times A: sixteen neighbouring directory entries span more than 65535 rows, kFlagDir16 is clear."""
    codes = np.zeros(70_000, np.uint8)
    want = pkg.GenieIndex.build(codes, 8).serialize(seed_table).numpy()
    assert B.sections(want)[0]["flags"] & 1 == 0
    _same_image(pkg, codes, 8, {}, seed_table, want)


# ------------------------------------------------------------------ 2. find_smems
@pytest.mark.parametrize("label", SHORT + MID)
def test_find_smems_against_the_oracle(pkg, cls, ix, orc, label):
    reads = _covered(pkg, cls, label)
    for mode, min_len in MODES:
        B.compare(_find(ix, label, reads, mode, min_len), _want(pkg, orc, label, mode, min_len), reads, (label, mode, min_len))


def test_find_smems_on_the_device_built_image(pkg, cls, dev, orc):
    for label in SHORT + MID:
        reads = _covered(pkg, cls, label)
        for mode, min_len in MODES[:3]:                       # a device-built handle has no model
            B.compare(_find(dev, label, reads, mode, min_len), _want(pkg, orc, label, mode, min_len), reads,
                      ("device-built", label, mode, min_len))


# ------------------------------------------------------------------ 3. the other entry points
OTHER = ["fromref150"] + TARGETED


def test_both_strands(pkg, cls, ix, orc):
    from genie_smem_amd import packing
    for label in OTHER:
        reads = _covered(pkg, cls, label)
        both = [x for r in reads for x in (r, packing.reverse_complement(r))]
        for mode, min_len in MODES:
            B.compare(ix.find_smems_both(mode, np.stack(reads), None, min_len), B.expected_batch(orc, both, mode, min_len), both,
                      (label, "both", mode, min_len))


def test_packed_rows(pkg, cls, ix, orc):
    from genie_smem_amd import packing
    for label in OTHER:
        reads = _covered(pkg, cls, label)
        mat = np.stack(reads)
        packed = packing.pack_reads(mat)
        for mode, min_len in MODES:
            for rb in (8, 6):
                c8, s8, r8, esc = ix.find_smems_packed(mode, packed, mat.shape[1], None, min_len, row_bytes=rb)
                off, rows = packing.unpack_rows(c8.cpu().numpy(), r8.cpu().numpy(), esc.cpu().numpy(), row_bytes=rb)
                B.compare((off, rows, s8.cpu().numpy().astype(np.int32)), _want(pkg, orc, label, mode, min_len), reads,
                          (label, "packed", rb, mode, min_len))


def test_slots_and_compact(pkg, cls, ix, orc):
    for label in OTHER:
        reads = _covered(pkg, cls, label)
        for mode, min_len in MODES:
            counts, slots, st = ix.find_smems_slots(mode, np.stack(reads), None, min_len)
            off, rows = ix.compact(counts, slots)
            want = _want(pkg, orc, label, mode, min_len)
            assert counts.cpu().numpy().tolist() == np.diff(want[0]).tolist(), (label, mode, min_len)
            B.compare((off, rows[:int(off[-1])], st), want, reads, (label, "slots", mode, min_len))


def test_split_at_breaks(pkg, cls, ix, orc):
    """A break at offset P2 - 1 leaves a first segment shorter than a table key, one at P2 a segment of exactly the P2-mer."""
    for label in OTHER:
        cut = B.with_breaks(_covered(pkg, cls, label), cls.P2)
        if label in B.TARGETED:                               # the break at P2 keeps the P2-mer of position 0
            mask = cls.starved if B.TARGETED[label] == "starved" else cls.block
            assert B.starts_on(mask, cut[1::3], cls.P2)
        assert B.positions_on(cls.starved, cut, cls.P2) >= 0.05 * B.positions(cut), label
        for min_len in (1, 12):
            B.compare(ix.find_smems_split(np.stack(cut), None, min_len), B.expected_split(orc, cut, min_len), cut, (label, "split", min_len))


def test_long_reads(pkg, cls, ix, orc):
    reads = _covered(pkg, cls, "long9000")
    assert min(len(r) for r in reads) > pkg._native.MAX_READ_LEN
    for mode, min_len in MODES:
        B.compare(ix.find_smems_long(mode, *S.csr(reads), min_len), _want(pkg, orc, "long9000", mode, min_len), reads,
                  ("long", mode, min_len))


def test_long_reads_both_strands_and_breaks(pkg, cls, ix, orc):
    from genie_smem_amd import packing
    cut = B.with_breaks(_covered(pkg, cls, "mid705"), cls.P2)
    assert B.positions_on(cls.starved, cut, cls.P2) >= 0.05 * B.positions(cut)
    both = [x for r in cut for x in (r, packing.reverse_complement(r))]
    for min_len in (1, 12):
        got = ix.find_smems_long("bwa", *S.csr(cut), min_len, both_strands=True, split_breaks=True)
        B.compare(got, B.expected_split(orc, both, min_len), both, ("long_ex", min_len))


# ------------------------------------------------------------------ 4. matching statistics and their intervals
@pytest.mark.parametrize("label", OTHER)
def test_match_stats_intervals(pkg, cls, ix, orc, oracle_mod, label):
    """At every position i with length m: lohi is the oracle's interval of read[i : i + m], and the match cannot be
    extended -- it ends with the read, or read[i : i + m + 1] occurs nowhere."""
    reads = _covered(pkg, cls, label, B.batches(pkg)[label][:200 if label == "fromref150" else None])
    bases, offs = S.csr(reads)
    ms, lohi, st = (t.cpu().numpy() for t in ix.match_stats(bases, offs))
    assert not st.any() and (ms >= 1).all()
    lib, u8p = oracle_mod.lib(), C.POINTER(C.c_uint8)
    lo, hi, first = C.c_int32(), C.c_int32(), bases.ctypes.data

    def back_prop(at, m):
        return (-1, -1) if lib.orc_back_prop(orc._h, C.cast(first + at, u8p), m, C.byref(lo), C.byref(hi)) else (lo.value, hi.value)

    end = np.repeat(offs[1:], np.diff(offs))
    assert (np.arange(ms.size) + ms <= end).all()
    for at, (m, e, iv) in enumerate(zip(ms.tolist(), end.tolist(), lohi.tolist())):
        want = back_prop(at, m)
        longest = at + m == e or back_prop(at, m + 1) == (-1, -1)
        if tuple(iv) != want or not longest:
            r = int(np.searchsorted(offs, at, side="right")) - 1
            raise AssertionError((label, "read", r, reads[r].tolist()[:100], "position", at - int(offs[r]), "length", m, "got", iv,
                                  "want", want, "the longest match" if longest else "not the longest match"))


# ------------------------------------------------------------------ 5. plain intervals
PATTERN_LENGTHS = [B.P2 - 1, B.P2, B.P2 + 1, B.P2 + 7, B.P2 + 8, B.P2 + 9, B.P2 + 16, B.P2 + 17, 60]


def _patterns(cls):
    """Cuts of the reference of every length of PATTERN_LENGTHS at 60 starved and 60 block entries, each as cut and with its
    last base substituted."""
    rng = np.random.default_rng(7100)
    pats = []
    for mask in (cls.starved, cls.block):
        for s in B.class_starts(cls, mask, 60, 60, rng):
            for length in PATTERN_LENGTHS:
                p = B.REF[s:s + length].copy()
                pats += [p, B._substitute(p, length - 1, rng)]
        if mask is cls.starved:
            assert B.starts_on(mask, [p for p in pats[0::2] if len(p) >= cls.P2] + [p for p in pats[1::2] if len(p) > cls.P2], cls.P2)
    half = len(pats) // 2
    assert B.starts_on(cls.block, [p for p in pats[half::2] if len(p) >= cls.P2], cls.P2)
    return pats


def test_plain_intervals_and_locate(pkg, cls, ix, orc):
    from genie_smem_amd import packing
    pats = _patterns(cls)
    both = [x for p in pats for x in (p, packing.reverse_complement(p))]
    want2 = np.asarray([orc.back_prop(p) for p in both], np.int32)
    want1 = want2[0::2]
    assert (want1[0::2, 0] >= 0).all() and (want1[1::2, 0] < 0).any() and (want2[1::2, 0] < 0).any()

    def same(got, want, which, what):
        bad = np.flatnonzero((got != want).any(1))
        assert not len(bad), (what, "pattern", int(bad[0]), which[bad[0]].tolist(), "got", got[bad[0]].tolist(), "want", want[bad[0]].tolist())

    same(ix.sa_interval(*S.matrix(pats, fill=9)).cpu().numpy(), want1, pats, "sa_interval")
    same(ix.sa_interval(*S.matrix(both, fill=9)).cpu().numpy(), want2, both, "sa_interval, both strands")
    bases, offs = S.csr(pats)
    sa = orc.suffix_array
    for strands, want, which in ((False, want1, pats), (True, want2, both)):
        lohi, cnt, st = (t.cpu().numpy() for t in ix.exact_match(bases, offs, both_strands=strands, counts=True))
        same(lohi, want, which, ("exact_match", strands))
        assert not st.any() and np.array_equal(cnt, np.where(want[:, 0] >= 0, want[:, 1] - want[:, 0] + 1, 0))
        off, pos = (t.cpu().numpy() for t in ix.locate(lohi))
        assert np.array_equal(np.diff(off), cnt)
        for i, (lo, hi) in enumerate(want.tolist()):
            assert pos[off[i]:off[i + 1]].tolist() == (sa[lo:hi + 1].tolist() if lo >= 0 else []), ("locate", strands, i)


# ------------------------------------------------------------------ 6. launch options
def test_launch_options_change_nothing(pkg, cls, ix, orc):
    N = pkg._native
    settings = [{N.OPT_SEARCH_ALL: 1}, {N.OPT_GROUP_POSITIONS: 1}, {N.OPT_GROUP_POSITIONS: 1536}, {N.OPT_SCHEDULING: 15}]
    try:
        for setting in settings:
            for opt, value in setting.items():
                ix.set_option(opt, value)
            for label in TARGETED:
                reads = _covered(pkg, cls, label)
                for mode, min_len in MODES:
                    B.compare(_find(ix, label, reads, mode, min_len), _want(pkg, orc, label, mode, min_len), reads,
                              (tuple(setting.items()), label, mode, min_len))
            for opt in setting:
                ix.set_option(opt, 0)
    finally:
        for opt in (N.OPT_SEARCH_ALL, N.OPT_GROUP_POSITIONS, N.OPT_SCHEDULING):
            ix.set_option(opt, 0)
