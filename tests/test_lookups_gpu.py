"""GPU: genie_sa_interval, genie_seed_lookup and genie_locate against the brute force of tests/lookup_util.py (sorted
suffix strings; pinned by test_lookups_host.py) on a family of edge references of at most 4096 bases: tiny ones, every
tail that the prefix directory has to correct for, tandem repeats, a reference without T.  Every comparison is on integers
or float64 bit patterns and exact.

Each test first works out, from the brute-force answers alone, what it is about to ask (a `plan`: inputs and expected
outputs) and asserts that the classes of inputs it exists for are not empty, then runs the plan's calls on the device."""
import functools

import numpy as np
import pytest

import lookup_util as U
from test_host_index import _parse

pytestmark = pytest.mark.gpu

FAMILY = U.family()


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


# ------------------------------------------------------------------ the indices
EXPLICIT_BITS = {3: 6, 7: 9}          # table_bits (P2) given by hand, per dir_bits; automatic is P + 1 .. 5 at these sizes


def index_specs():
    """(reference, dir_bits, table_bits, table form).  Every reference with dir_bits 3 and 7 and automatic tables (compact
    form); with explicit table_bits, tandem references at both dir_bits and the others at one (alternating), in the wide
    form on tandem and tail references: both forms there, 57 indices in all."""
    specs = []
    for i, name in enumerate(FAMILY):
        specs += [(name, 3, 0, "auto"), (name, 7, 0, "auto")]
        fmt = "wide" if U.is_tandem(name) or U.is_tail(name) else "auto"
        ps = (3, 7) if U.is_tandem(name) else ((3,) if i % 2 == 0 else (7,))
        specs += [(name, P, EXPLICIT_BITS[P], fmt) for P in ps]
    return specs


SPECS = index_specs()
assert len(SPECS) < 60


def _build(pkg, name, P, bits, fmt, K=0):
    ix = pkg.GenieIndex.build(FAMILY[name], K, dir_bits=P, table_bits=bits, table_format=fmt)
    h = _parse(ix.serialize().numpy())
    assert h["P"] == P == ix.info()["dir_bits"] and h["n"] == len(FAMILY[name])
    assert h["P2"] == (bits or h["P2"]) and h["P2"] > P
    assert bool(h["flags"] & 2) == (fmt != "wide")                                  # kFlagCompactTable
    return ix, h["P2"]


# ------------------------------------------------------------------ sa_interval
N_MAIN = 4097
BAD = (-2, -2)


def sa_plan(name, P, P2, seed):
    """-> list of calls (pats [N, stride] uint8, lens or None, expected int32 [N, 2]) and the number of patterns.
    Call geometries: N = 4097 with a lens array and a stride wider than every length (the bytes behind a pattern are junk,
    one row holds a code > 3); N = 1 and N = 5; fixed_len without lens for several lengths; one batch at fixed_len 8192."""
    ref, rows = FAMILY[name], _rows(name)
    n = len(ref)
    pats = U.patterns(name, ref, P, P2, N_MAIN - 1, seed)
    want = [U.interval(ref, rows, p) for p in pats]
    cnt = np.asarray([hi - lo + 1 if lo >= 0 else 0 for lo, hi in want])
    plen = np.asarray([len(p) for p in pats])

    # what this index has to be asked, from the brute-force answers alone
    assert (cnt == 0).any(), "no absent pattern"
    assert (cnt == 1).any(), "no pattern with one row"
    assert any(U.runs_off_end(ref, p) for p in pats), "no pattern that runs off the end of the reference"
    if n + 1 > 32:                                           # a reference of fewer rows has no such pattern
        assert (cnt > 32).any(), "no pattern with more than 32 rows"
    if P2 > P + 1:                                           # shorter than P2, longer than P: bucket bisection from the directory
        mid = (plen > P) & (plen < P2)
        assert (cnt[mid] > 0).any() or n <= P
        if not (cnt[mid] == 0).any():                        # none absent: only where every (P + 1)-mer occurs
            every = ((np.arange(4 ** (P + 1))[:, None] >> (2 * np.arange(P, -1, -1))) & 3).astype(np.uint8)
            assert all(U.interval(ref, rows, k)[0] >= 0 for k in every)
    if n >= 300:
        inkey = (plen >= P2) & (plen <= P + 32)              # decided inside the first row's inline key ...
        first = np.asarray([U.interval(ref, rows, p[:P2])[0] if len(p) >= P2 else -1 for p in pats])
        lo = np.asarray([w[0] for w in want])
        assert (inkey & (cnt > 0) & (lo == first)).any() and (inkey & (cnt == 0) & (first >= 0)).any()
        if n >= 3000 or P2 <= 6:                             # (300 random bases: no two suffixes share 8 bases, in expectation)
            assert (inkey & (cnt > 0) & (lo > first)).any()
        short = (plen >= P2) & (first >= 0) & (rows[np.maximum(first, 0)] > n - (P + 32))      # ... or a kHeadShort head
        assert short.any()
        assert ((plen > P + 32) & (cnt > 0)).any(), "no present pattern longer than P + 32 (cmp_suffix)"
    if U.is_tandem(name):
        assert ((plen > P + 32) & (cnt > 1)).any(), "no repeated pattern longer than P + 32"
        assert ((plen > P + 32) & (cnt > 100)).any()
        if name == "tandem1":                                # many equal keys, a gallop over thousands of rows
            assert ((plen > P) & (cnt > 2000)).any()

    calls = []
    stride = int(plen.max()) + 5
    mat, lens = U.pack_rows(pats + [np.asarray([0, 1, 7, 2], np.uint8)], stride, fill=9)
    calls.append((mat, lens, np.asarray(want + [BAD], np.int32)))
    pick = [int(np.argmax((cnt > 0) * plen)), 0, int(np.argmax(cnt)), int(np.argmax(cnt == 0)), N_MAIN - 1]
    calls.append((mat[pick[:1]], lens[pick[:1]], calls[0][2][pick[:1]]))
    calls.append((mat[pick], lens[pick], calls[0][2][pick]))
    for L in sorted({1, P, P + 1, P2, P + 33, 97}):
        sel = np.nonzero(plen == L)[0]
        assert len(sel)
        calls.append((np.ascontiguousarray(mat[sel, :L]), None, calls[0][2][sel]))
    rng = np.random.default_rng(seed + 1)
    long = [np.concatenate([ref, rng.integers(0, 4, 8192 - n).astype(np.uint8)]),
            np.tile(ref, 8192 // n + 1)[:8192], rng.integers(0, 4, 8192).astype(np.uint8),
            np.tile(ref[:7], 8192 // min(n, 7) + 1)[:8192], np.full(8192, ref[-1], np.uint8)]
    assert all(len(p) == 8192 > n for p in long) and ((plen > n).any() or n > 1000)      # patterns longer than the reference
    calls.append((np.asarray(long, np.uint8), None, np.asarray([U.interval(ref, rows, p) for p in long], np.int32)))
    return calls, sum(len(c[0]) for c in calls)


def _spec_id(s):
    return f"{s[0]}-P{s[1]}-bits{s[2]}-{s[3]}"


@pytest.mark.parametrize("spec", SPECS, ids=_spec_id)
def test_sa_interval_against_brute_force(pkg, spec):
    name, P, bits, fmt = spec
    ix, P2 = _build(pkg, name, P, bits, fmt)
    calls, _ = sa_plan(name, P, P2, SPECS.index(spec))
    ix.to("cuda")
    for c, (mat, lens, want) in enumerate(calls):
        got = ix.sa_interval(mat, lens).cpu().numpy()
        bad = np.nonzero((got != want).any(1))[0]
        assert not len(bad), (spec, c, [(mat[i, :(lens[i] if lens is not None else mat.shape[1])].tolist()[:80],
                                         got[i].tolist(), want[i].tolist()) for i in bad[:3]])


# ------------------------------------------------------------------ seed_lookup
TRAINED = ([10], [10, 100], [4, 16, 64])


def bad_models(n, K):
    """Caller-supplied coefficients that predict badly: all zero; a slope so large that every prediction exceeds n; a
    negative slope.  (experts, coefs, icpts) as GenieIndex.set_rmi takes them."""
    z = [np.zeros(1), np.zeros(10)]
    return [([10], z, z),
            ([10], [np.full(1, 1e6), np.full(10, 1e6)], [np.full(1, n + 5.0), np.full(10, n + 5.0)]),
            ([10], [np.full(1, -10.0 / 4 ** K), np.full(10, -(n + 1.0) / 4 ** K)], [np.full(1, 10.0), np.full(10, float(n))])]


@functools.lru_cache(maxsize=None)
def seed_plan(name, K):
    """-> (kmers uint8 [N, K], kmer_interval of each int32 [N, 2], present mask)."""
    ref, rows = FAMILY[name], _rows(name)
    kmers = U.kmers_for(ref, K, 1000 + K)
    want = np.asarray([U.kmer_interval(ref, rows, k) for k in kmers], np.int32)
    return kmers, want, want[:, 1] >= want[:, 0]


def _lookup_chunks(ix, mode, kmers, want_pred=False):
    """The batch in calls of 255, 256, 257 K-mers and the rest."""
    cuts = np.minimum(np.cumsum([0, 255, 256, 257, len(kmers)]), len(kmers))
    out, pred = [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        if b > a:
            r = ix.seed_lookup(mode, kmers[a:b], want_pred=want_pred)
            out.append((r[0] if want_pred else r).cpu().numpy())
            if want_pred:
                pred.append(r[1].cpu().numpy())
    return np.concatenate(out), (np.concatenate(pred) if want_pred else None)


SEED_CASES = [(name, K) for name in FAMILY for K in U.SEED_KS if K <= len(FAMILY[name])]
SHORT_CASES = [(name, K) for name in FAMILY for K in U.SEED_KS if K > len(FAMILY[name])]


@pytest.mark.parametrize("name,K", SEED_CASES)
def test_seed_lookup_against_brute_force(pkg, name, K):
    ref = FAMILY[name]
    n = len(ref)
    kmers, want, present = seed_plan(name, K)
    assert present.any()
    assert (~present).any() or (K <= 8 and present[:4 ** K].all())     # all 4^K were asked: the reference holds every K-mer
    codes = np.asarray([U.kmer_code(k) for k in kmers], np.int64)
    lut_want = np.where(present[:, None], want, -1)
    models = [(ex, None, None) for ex in TRAINED] + bad_models(n, K)
    for m, (experts, coefs, icpts) in enumerate(models):
        ix = pkg.GenieIndex.build(ref, K, dir_bits=3)
        if coefs is None:
            coefs, icpts, leaf_err, _, _ = ix.train_rmi(experts)          # the coefficients genie_index_rmi_models exports
            assert len(leaf_err) == experts[-1]
        else:
            ix.set_rmi(experts, coefs, icpts)
        ix.to("cuda")
        if m == 0:
            got, _ = _lookup_chunks(ix, "lut", kmers)
            bad = np.nonzero((got != lut_want).any(1))[0]
            assert not len(bad), (name, K, "lut", [(kmers[i].tolist(), got[i].tolist(), lut_want[i].tolist()) for i in bad[:3]])
        got, pred = _lookup_chunks(ix, "rmi", kmers, want_pred=True)
        bad = np.nonzero((got != want).any(1))[0]
        assert not len(bad), (name, K, experts, m, [(kmers[i].tolist(), got[i].tolist(), want[i].tolist()) for i in bad[:3]])
        sizes, scales = [len(c) for c in coefs], list(experts) + [1]
        ref_pred = U.rmi_predict(sizes, scales, np.concatenate(coefs), np.concatenate(icpts), codes)
        assert (pred.view(np.uint64) == ref_pred.view(np.uint64)).all(), (name, K, experts, m)
        if m >= len(TRAINED):                                             # the bad models do predict badly
            by_code = ref_pred[np.argsort(codes, kind="stable")]
            assert [(ref_pred == 0).all(), (ref_pred > n).all(),
                    (np.diff(by_code) <= 0).all() and by_code[0] > by_code[-1]][m - len(TRAINED)]


@pytest.mark.parametrize("name,K", SHORT_CASES)
def test_seed_lookup_reference_shorter_than_k(pkg, name, K):
    """A reference of fewer than K bases holds no K-mer.  Pinned: the index builds; LUT mode reports every K-mer absent,
    (-1, -1); native training is refused on the host (GENIE_E_INVALID, nothing launched); with caller-supplied coefficients
    RMI mode reports every K-mer absent the reference's way, lower > upper, lower = the row it would be inserted at."""
    ref, rows = FAMILY[name], _rows(name)
    kmers = U.kmers_for(ref, K, 5)[-2000:]
    want = np.asarray([U.kmer_interval(ref, rows, k) for k in kmers], np.int32)
    assert (want[:, 1] == want[:, 0] - 1).all()
    ix = pkg.GenieIndex.build(ref, K, dir_bits=3)
    assert ix.info()["lut_keys"] == 0
    with pytest.raises(pkg._native.GenieError) as err:
        ix.train_rmi([10])
    assert err.value.status == -1                                             # GENIE_E_INVALID
    experts, coefs, icpts = bad_models(len(ref), K)[2]
    ix.set_rmi(experts, coefs, icpts)
    ix.to("cuda")
    assert (ix.seed_lookup("lut", kmers).cpu().numpy() == -1).all()
    got = ix.seed_lookup("rmi", kmers).cpu().numpy()
    assert (got == want).all(), (name, K, kmers[np.nonzero((got != want).any(1))[0][:3]].tolist())


# ------------------------------------------------------------------ locate
LOCATE_REFS = ["rand1", "rand5", "rand37", "tail_TTTTTTTT", "tandem1", "tandem7", "noT", "rand4096"]
ROW_COUNTS = [0, 1, 2, 31, 32, 33, 64, 65]


@functools.lru_cache(maxsize=None)
def locate_plan(name):
    """-> int32 [S, 2] intervals, S >= 257: row ranges of every count of ROW_COUNTS that fits (at the first row, at the
    last row and in between), the whole array (0, n), the absent conventions (-1, -1), (-2, -2) and lo > hi, intervals of
    patterns from the brute force, and on a tandem reference 80 consecutive intervals of more than 32 rows each."""
    ref, rows = FAMILY[name], _rows(name)
    n = len(ref)
    iv = [(0, n), (-1, -1), (-2, -2), (3, 2), (n, 0), (1, 0)]
    for c in ROW_COUNTS[1:]:
        if c <= n + 1:
            iv += [(0, c - 1), (n + 1 - c, n), ((n + 1 - c) // 2, (n + 1 - c) // 2 + c - 1)]
    iv.append((n // 2, n // 2 - 1))                                           # count 0 as lo = hi + 1 (an absent K-mer)
    if U.is_tandem(name):
        wide = [U.interval(ref, rows, ref[i:i + 50 + i]) for i in range(80)]
        assert all(hi - lo + 1 > 32 for lo, hi in wide)
        iv += wide
    rng = np.random.default_rng(len(name) + n)
    for p in U.patterns(name, ref, 3, 5, 300, 77):
        iv.append(U.interval(ref, rows, p[:int(rng.integers(0, 12))]))
    while len(iv) < 257:
        iv += iv[:257 - len(iv)]
    return np.asarray(iv, np.int32)


def _check_locate(ix, name, iv, width, sort):
    rows = _rows(name)
    want = [U.positions(rows, int(lo), int(hi)) for lo, hi in iv]
    if sort:
        want = [sorted(w) for w in want]
    arg = iv
    if width == 4:                                                            # find_smems rows: junk in columns 0 - 1
        arg = np.concatenate([np.full((len(iv), 2), -77, np.int32), iv], axis=1)
        arg[::2, 0], arg[1::2, 1] = 2**31 - 1, 5
    off, pos = ix.locate(arg.reshape(-1, width), sort=sort)
    off, pos = off.cpu().numpy(), pos.cpu().numpy()
    assert off.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).astype(np.int64).tolist(), (name, width)
    assert pos.tolist() == [x for w in want for x in w], (name, width, sort)
    return len(iv), len(pos)


@pytest.mark.parametrize("name", LOCATE_REFS)
def test_locate_against_brute_force(pkg, name):
    iv = locate_plan(name)
    n = len(FAMILY[name])
    counts = np.where((iv[:, 0] >= 0) & (iv[:, 1] >= iv[:, 0]), iv[:, 1] - iv[:, 0] + 1, 0)
    assert set(c for c in ROW_COUNTS if c <= n + 1) <= set(counts.tolist()) and n + 1 in counts
    if U.is_tandem(name):                                                     # a wave in which all 64 lanes hold a wide interval
        run = np.convolve((counts > 32).astype(int), np.ones(64, int), "valid")
        assert (run == 64).any()
    ix = pkg.GenieIndex.build(FAMILY[name], 0, dir_bits=3).to("cuda")
    for S in (0, 1, 255, 256, 257, len(iv)):
        for width in (2, 4):
            _check_locate(ix, name, iv[:S], width, sort=False)
    _check_locate(ix, name, iv, 2, sort=True)
    _check_locate(ix, name, iv[::-1].copy(), 4, sort=True)
    if U.is_tandem(name):                                                     # the wide run at the front of a block, S = 64
        start = int(np.argmax(run == 64))
        _check_locate(ix, name, iv[start:start + 64], 2, sort=False)


# ------------------------------------------------------------------ end to end through the drop-in
@pytest.mark.parametrize("name", ["tail_ACGTTTA", "tandem3"])
def test_dropin_exact_match_against_brute_force(pkg, name):
    ref, rows = FAMILY[name], _rows(name)
    n = len(ref)
    m = pkg.ExactMatch(name + ".fa")
    m.set_reference("".join("ACGT"[c] for c in ref))
    rng = np.random.default_rng(3)
    chosen = []
    for L in range(1, 13):                                  # the directory answers up to 7 bases
        s = int(rng.integers(0, n - L))
        miss = ref[s:s + L].copy()
        miss[-1] = (miss[-1] + 1 + rng.integers(0, 3)) & 3
        chosen += [ref[s:s + L], miss]
    chosen += [ref[n - 3:], ref[n - 7:], ref[n - 8:], ref[:150], ref[100:141]]
    chosen += [np.concatenate([ref[n - j:], [b]]).astype(np.uint8) for j in (2, 6, 7, 40) for b in (0, 3)]   # off the end
    assert sum(len(p) <= 7 for p in chosen) >= 10 and sum(len(p) > 7 for p in chosen) >= 10
    hits = 0
    for p in chosen:
        q = "".join("ACGT"[c] for c in p)
        lo, hi = U.interval(ref, rows, p)
        got = m.exact_match_back_prop(q)
        assert got == (-1 if lo < 0 else (lo, hi)), q
        if lo >= 0:
            hits += 1
            assert m.get_positions(lo, hi) == U.positions(rows, lo, hi), q
            assert m.exact_match(q) == sorted(U.positions(rows, lo, hi)), q
    assert 0 < hits < len(chosen)
    batch = m.exact_match_positions_batch(["".join("ACGT"[c] for c in p) for p in chosen])
    assert batch == [sorted(U.positions(rows, *U.interval(ref, rows, p))) for p in chosen]
