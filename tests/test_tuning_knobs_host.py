"""CPU: the brute force of tests/smem_util.py (get_SMEMS stated as substring membership on sorted suffix strings) against
the C oracle, on every reference of lookup_util.family() and every read of smem_util.batches(): BWA mode with min_len 1
and 12, LUT mode, and RMI mode with a natively trained model, row for row and flag for flag; and the literal quadratic
form of the brute force against the linear one.  This validates the expectations of test_tuning_knobs_gpu.py without a
GPU and pins the oracle on tiny, tail and tandem references.  No read is left out of a comparison."""
import functools

import numpy as np
import pytest

import lookup_util as U
import smem_util as S

FAMILY = U.family()
GRID_P2 = (2, 3, 4, 5, 6, 8, 9, 10, 11, 12)                 # every table_bits test_tuning_knobs_gpu.py builds with


@pytest.fixture(scope="module")
def pkg():
    import genie_smem_amd as g
    g._native.build()
    g._native.lib()
    return g


def _groups(name):
    """(label, reads) of every batch of one reference."""
    b = S.batches(name)
    return ([(f"short{L}", r) for L, r in b["short"].items()] + [(f"mid{L}", r) for L, r in b["mid"].items()]
            + [("long", b["long"]), ("ragged", b["ragged"])])


def host_ks(n):
    """Key sizes for the LUT and RMI comparisons: 2, 8 and 13 where the reference holds a K-mer (K <= n), else n."""
    return sorted({min(k, n) for k in (2, 8, 13)})


def _oracle_status(rc, read):
    """The oracle's error -> the library's flag.  -2 is the reference's KeyError: for a code > 3, and also for a base that
    the reference lacks when a backward search meets it (count_dic[char]); -4 is the pivot standing on such a base."""
    if rc == -3:
        return S.READ_TOO_SHORT
    if rc == -2 and len(read) and int(read.max()) > 3:
        return S.READ_BAD_BASE
    assert rc in (-2, -4), rc
    return S.READ_ABSENT_BASE


def _against_oracle(o, ref, reads, mode, min_len, K, tag):
    mat, lens = S.matrix(reads)
    counts, out = o.find_smems_batch(mode, mat, min_len=min_len, lens=lens)
    flags = []
    for r, read in enumerate(reads):
        st, rows = S.expected(ref, read, mode, min_len, K)
        if counts[r] < 0:
            assert st == _oracle_status(int(counts[r]), read) != S.READ_OK, (tag, r, int(counts[r]), st)
        else:
            assert st == S.READ_OK and rows.tolist() == out[r, :counts[r]].tolist(), (tag, r, read.tolist()[:80])
        flags.append(st)
    return flags


@pytest.mark.parametrize("name", list(FAMILY))
def test_brute_force_equals_oracle_bwa(oracle_mod, name):
    ref = FAMILY[name]
    o = oracle_mod.Oracle(ref, 0)
    flags, long_rows = [], 0
    for label, reads in _groups(name):
        for min_len in (1, 12):
            flags += _against_oracle(o, ref, reads, "bwa", min_len, 0, (name, label, min_len))
        long_rows += sum(int((np.diff(S.expected(ref, r, "bwa")[1][:, :2]) >= 12).sum()) for r in reads)
    assert S.READ_BAD_BASE in flags and S.READ_OK in flags
    assert (S.READ_ABSENT_BASE in flags) == (len(np.unique(ref)) < 4)
    assert long_rows > 0 or len(ref) < 12                    # min_len 12 keeps some rows and drops others


@pytest.mark.parametrize("name", list(FAMILY))
def test_brute_force_equals_oracle_lut_rmi(pkg, oracle_mod, name):
    ref = FAMILY[name]
    for K in host_ks(len(ref)):
        o = oracle_mod.Oracle(ref, K)
        ix = pkg.GenieIndex.build(ref, K)
        coefs, icpts, _, _, _ = ix.train_rmi([10])
        o.set_rmi([10], coefs, icpts)
        for mode in ("lut", "rmi"):
            flags = []
            for label, reads in _groups(name):
                flags += _against_oracle(o, ref, reads, mode, 1, K, (name, label, mode, K))
            assert S.READ_BAD_BASE in flags and S.READ_OK in flags
            assert S.READ_TOO_SHORT in flags                # lengths K - 1 and 0 are in the batches


@pytest.mark.parametrize("name", list(FAMILY))
def test_quadratic_form_equals_linear_form(name):
    ref = FAMILY[name]
    seen = 0
    for label, reads in _groups(name):
        for read in reads:
            if len(read) > 255 or (len(read) and int(read.max()) > 3):
                continue                                     # the long reads have the linear form only; a code 7 has no rows
            for min_len in (1, 12):
                a, fa = S.smems_quadratic(ref, read, min_len)
                b, fb = S.smems(ref, read, min_len)
                assert fa == fb and a.tolist() == b.tolist(), (name, label, min_len, read.tolist())
                st, rows = S.expected(ref, read, "bwa", min_len)
                assert (st == S.READ_ABSENT_BASE) == fb and (fb or rows.tolist() == b.tolist())
            seen += 1
    assert seen >= 150


@pytest.mark.parametrize("name", [n for n in FAMILY if U.is_tandem(n)])
def test_long_repeats_against_the_definition_of_an_smem(name):
    """The 9000-base reads that repeat a tandem unit throughout ("long_extra") cost the literal oracle a minute each, so
    their expected rows are held against the definition instead: the SMEMs of a read are its matches that can be extended
    on neither side -- (s, fwd[s]) wherever fwd rises -- and the row of pivot i is the longest SMEM that covers i, the one
    that ends first on a tie; the first pivot is 0, the next one the row's end, the last row ends the read."""
    ref, reads = FAMILY[name], S.batches(name)["long_extra"]
    sufs, rows_of = U._sorted_suffixes(ref), U.suffix_rows(ref)
    assert len(reads) >= 2 and all(len(r) == S.LONG_LENGTH for r in reads)
    for read in reads:
        st, rows = S.expected(ref, read, "bwa")
        assert st == S.READ_OK and len(rows)
        q, L = U._bytes(read), len(read)
        fwd = S.matching_stats(ref, read)
        rises = np.flatnonzero(np.diff(np.concatenate([[0], fwd])) > 0)
        maximal = [(int(s), int(fwd[s])) for s in rises]
        for s, e in maximal[:50] + maximal[-50:]:            # maximal as strings, not only by fwd[]
            assert S._occurs(sufs, q[s:e]) and (e == L or not S._occurs(sufs, q[s:e + 1]))
            assert s == 0 or not S._occurs(sufs, q[s - 1:e])
        pivot, starts, ends = 0, rises, fwd[rises]
        for s, e, lo, hi in rows.tolist():
            cover = np.flatnonzero((starts <= pivot) & (ends > pivot))
            longest = cover[ends[cover] - starts[cover] == (ends[cover] - starts[cover]).max()]
            best = longest[np.argmin(ends[longest])]
            assert (int(starts[best]), int(ends[best])) == (s, e) and (lo, hi) == U.interval(ref, rows_of, read[s:e]), (name, pivot)
            pivot = e
        assert pivot == L
        assert S.expected(ref, read, "bwa", 12)[1].tolist() == [r for r in rows.tolist() if r[1] - r[0] >= 12]


def test_matching_stats_definition():
    """fwd[] against its definition, directly, on reads short enough to try every prefix."""
    for name in ("rand5", "tail_AAAAAAAA", "tandem3", "noT"):
        ref = FAMILY[name]
        r = U._bytes(ref)
        for read in S.batches(name)["short"][33] + S.batches(name)["short"][7]:
            q = U._bytes(read)
            want = [max(e for e in range(a, len(q) + 1) if q[a:e] in r) for a in range(len(q))]
            assert S.matching_stats(ref, read).tolist() == want, (name, read.tolist())


@functools.lru_cache(maxsize=None)
def _profile(name):
    """Per read of every batch that has rows: (length, longest row, last pivot, widest interval)."""
    ref, out = FAMILY[name], []
    for label, reads in _groups(name):
        for read in reads:
            st, rows = S.expected(ref, read, "bwa")
            if st == S.READ_OK and len(rows):
                pivot = int(rows[-2, 1]) if len(rows) > 1 else 0
                out.append((len(read), int((rows[:, 1] - rows[:, 0]).max()), pivot, int((rows[:, 3] - rows[:, 2]).max())))
    return np.asarray(out)


def test_batches_hold_the_classes_the_knobs_decide():
    """What table_bits (P2) decides in the match-statistics kernels, from the brute-force answers alone: matches longer
    than P2 + 16 (past every shortcut of the slow path) and shorter than P2 (absent P2-mers) for every P2 of the grid; a
    last pivot inside the final P2 - 1 bases, where the zero padding is looked up; on tandem1 intervals wider than 255
    rows (the 6-byte rows' escape; no interval of a reference of 3000 bases reaches the 8-byte rows' 65535)."""
    for name in ("tail_AAAAAAAA", "tandem7", "rand4096", "noT"):
        p = _profile(name)
        L, longest, pivot = p[:, 0], p[:, 1], p[:, 2]
        assert (longest > max(GRID_P2) + 16).any() and (longest < min(GRID_P2)).any(), name
        for P2 in GRID_P2:
            assert ((longest > P2 + 8) & (longest <= P2 + 16)).any(), (name, P2)
            assert ((pivot >= L - (P2 - 1)) & (pivot < L) & (L >= P2)).any(), (name, P2)
        assert (pivot == L - 1).any() and ((pivot < L - 1) & (pivot >= L - 11)).any(), name
    assert (_profile("tandem1")[:, 3] > 255).any() and (_profile("tandem1")[:, 3] <= 3000).all()
    ends_in_run = [r for r in S.batches("tail_AAAAAAAA")["short"][32] if U._bytes(r) == U._bytes(FAMILY["tail_AAAAAAAA"][268:300])]
    assert ends_in_run                                       # stops where the reference's final run of A begins
    assert {len(r) for r in S.batches("rand37")["ragged"]} >= {0, 1, 17, 255}
    for name in FAMILY:
        b = S.batches(name)
        assert set(b["short"]) == set(range(1, 18)) | {31, 32, 33, 64, 150, 255} and set(b["mid"]) == {256, 705, 1409}
        assert all(len(r) == 9000 for r in b["long"]) and 11 <= len(b["long"]) <= 16
        assert all(int(g[-1].max()) == S.BAD_CODE for g in list(b["short"].values()) + list(b["mid"].values()) + [b["long"]])
