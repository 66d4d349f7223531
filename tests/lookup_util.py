"""Brute-force reference for the lookup calls (genie_sa_interval, genie_seed_lookup, genie_locate): the suffix array by
sorting the suffix strings themselves, intervals by bisecting them, the RMI level walk in NumPy float64.  Plain Python and
NumPy; nothing here comes from the library under test.  Also the family of edge references the lookup tests run on and
the patterns they ask for.  References are at most 4096 bases (the sorted suffixes are kept as strings)."""
import bisect

import numpy as np

MAX_N = 4096
_SUFFIXES = {}          # reference bytes -> its suffixes as byte strings, sorted ('$' = end of string: a prefix sorts first)


def _bytes(a):
    return np.ascontiguousarray(a, np.uint8).tobytes()


def _sorted_suffixes(codes):
    key = _bytes(codes)
    if key not in _SUFFIXES:
        assert len(key) <= MAX_N
        _SUFFIXES[key] = sorted(key[s:] for s in range(len(key) + 1))
    return _SUFFIXES[key]


def suffix_rows(codes):
    """The n + 1 suffix starts (0-based) in sorted order; the empty suffix ('$', start n) comes first."""
    n = len(_bytes(codes))
    return np.asarray([n - len(s) for s in _sorted_suffixes(codes)], np.int64)


def _bounds(codes, pat):
    """[first, end) of the rows whose suffix starts with pat; first = where pat would be inserted."""
    sufs, p = _sorted_suffixes(codes), _bytes(pat)
    first = bisect.bisect_left(sufs, p)
    return first, bisect.bisect_left(sufs, p + b"\x04", first)     # every base code is below 4


def interval(codes, rows, pat):
    """Inclusive (lo, hi) of the rows whose suffix starts with pat; (0, n) for the empty pattern, (-1, -1) if none does."""
    assert len(rows) == len(_bytes(codes)) + 1
    first, end = _bounds(codes, pat)
    return (first, end - 1) if end > first else (-1, -1)


def kmer_interval(codes, rows, kmer):
    """interval() for a K-mer that occurs; (first, first - 1) for one that does not, first = the row it would be inserted at
    (a suffix that is a proper prefix of the K-mer sorts before it)."""
    assert len(rows) == len(_bytes(codes)) + 1
    first, end = _bounds(codes, kmer)
    return first, end - 1


def positions(rows, lo, hi):
    """1-based starts of rows lo .. hi in row order; none for lo < 0 or hi < lo."""
    if lo < 0 or hi < lo:
        return []
    return [int(s) + 1 for s in rows[lo:hi + 1]]


def rmi_predict(sizes, scales, coef, icpt, code):
    """The RMI level walk in float64: per level p = coef * x + icpt, rounded after the multiply and after the add; the
    next expert is min(scale - 1, max(0, int(p))).  coef / icpt hold all levels back to back (sizes[l] models each).
    `code` is one K-mer code or an array of them (finite coefficients only)."""
    coef, icpt = np.asarray(coef, np.float64), np.asarray(icpt, np.float64)
    x = np.atleast_1d(np.asarray(code)).astype(np.float64)
    p, idx, off = np.zeros_like(x), np.zeros(x.shape, np.int64), 0
    for size, scale in zip(sizes, scales):
        prod = coef[off + idx] * x                                   # one rounding
        p = prod + icpt[off + idx]                                   # and another
        idx = np.trunc(np.clip(p, 0.0, float(int(scale) - 1))).astype(np.int64)
        off += int(size)
    return float(p[0]) if np.ndim(code) == 0 else p


# ------------------------------------------------------------------ the reference family
TAILS = ["", "A", "AAAAAAAA", "TTTTTTTT", "CAAAAAA", "GTTTTTT", "ACGTTTA", "TTTTTTA", "C"]      # test_prefix_directory_brute_force
TANDEM_UNITS = {1: "G", 3: "ACT", 7: "GATTACA"}
TANDEM_LEN, TANDEM_BREAK = 3000, 1500


def _codes(s):
    return np.asarray(["ACGT".index(c) for c in s], np.uint8)


def family():
    """name -> uint8 codes of every reference of the family, in a fixed order."""
    out = {}
    for n in (1, 2, 5, 37):
        out[f"rand{n}"] = np.random.default_rng(100 + n).integers(0, 4, n).astype(np.uint8)
    for i, tail in enumerate(TAILS):
        body = np.random.default_rng(200 + i).integers(0, 4, 300).astype(np.uint8)
        out["tail_" + (tail or "none")] = np.concatenate([body, _codes(tail)]).astype(np.uint8)
    for u, unit in TANDEM_UNITS.items():
        ref = np.tile(_codes(unit), TANDEM_LEN // u + 1)[:TANDEM_LEN].copy()
        ref[TANDEM_BREAK] = (ref[TANDEM_BREAK] + 2) & 3              # one substituted base in the middle
        out[f"tandem{u}"] = ref
    out["noT"] = np.random.default_rng(300).integers(0, 3, 3000).astype(np.uint8)
    out["rand4096"] = np.random.default_rng(301).integers(0, 4, 4096).astype(np.uint8)
    return out


def is_tandem(name):
    return name.startswith("tandem")


def is_tail(name):
    return name.startswith("tail_")


# ------------------------------------------------------------------ patterns for sa_interval
WORD_LENGTHS = [63, 64, 65, 95, 96, 97, 150, 1000]


def pattern_lengths(P, P2):
    """Every length from 0 to P2 + 34 (so P, P + 1, P2 - 1, P2, P2 + 1, P + 32 and P + 33 by construction), the word
    boundaries of the 2-bit packing, 150 and 1000."""
    return sorted(set(range(0, P2 + 35)) | set(WORD_LENGTHS))


def patterns(name, ref, P, P2, total, seed):
    """`total` patterns (uint8 arrays, codes 0..3) for one index on reference `ref`: for every length of pattern_lengths
    one of each kind that exists at that length -- cut from the reference; cut with the last / first base changed; the
    reference's tail; the tail plus one base; random; on a tandem reference whole multiples of the unit, starting before
    the substituted base -- then cuts and changed cuts of random lengths until there are `total`.  A length beyond n
    gives the whole reference (or a cut of it) followed by random bases: a pattern longer than n."""
    rng = np.random.default_rng(seed)
    n = len(ref)
    out = []

    def cut(L):
        if L <= n:
            s = int(rng.integers(0, n - L + 1))
            return ref[s:s + L].copy()
        s = int(rng.integers(0, n))
        return np.concatenate([ref[s:], rng.integers(0, 4, L - (n - s)).astype(np.uint8)])

    def changed(p, at):
        p = p.copy()
        p[at] = (p[at] + 1 + rng.integers(0, 3)) & 3
        return p

    for L in pattern_lengths(P, P2):
        out.append(cut(L))
        out.append(rng.integers(0, 4, L).astype(np.uint8))
        if L >= 1:
            c = cut(L)
            out.append(changed(c, L - 1))
            out.append(changed(c, 0))
            if L - 1 <= n:
                for b in range(4):                                   # the tail plus one base: runs off the reference
                    out.append(np.concatenate([ref[n - (L - 1):], [b]]).astype(np.uint8))
        if L <= n:
            out.append(ref[n - L:].copy())
        if is_tandem(name):
            u = int(name[len("tandem"):])
            m = max(u, L // u * u)                                   # a whole multiple of the unit, about L long
            if m <= TANDEM_BREAK:
                s = int(rng.integers(0, (TANDEM_BREAK - m) // u + 1)) * u
                out.append(ref[s:s + m].copy())
                out.append(ref[:m].copy())
    lens = pattern_lengths(P, P2)
    while len(out) < total:
        L = int(lens[rng.integers(0, len(lens))]) if rng.integers(0, 2) else int(rng.integers(1, 200))
        c = cut(L)
        out.append(c if rng.integers(0, 3) or L == 0 else changed(c, int(rng.integers(0, L))))
    return out[:total]


def runs_off_end(ref, pat):
    """The pattern is a non-empty tail of the reference followed by one more base."""
    L, n = len(pat), len(ref)
    return 2 <= L <= n + 1 and _bytes(pat[:L - 1]) == _bytes(ref[n - (L - 1):])


def pack_rows(pats, stride=None, fill=0):
    """Patterns -> (uint8 [N, stride] matrix, int32 lengths); stride defaults to the longest length (at least 1)."""
    lens = np.asarray([len(p) for p in pats], np.int32)
    width = max(int(lens.max()) if len(pats) else 0, 1) if stride is None else stride
    mat = np.full((len(pats), width), fill, np.uint8)
    for i, p in enumerate(pats):
        mat[i, :len(p)] = p
    return mat, lens


# ------------------------------------------------------------------ K-mers for seed_lookup
SEED_KS = [1, 2, 3, 8, 12, 16]


def kmers_for(ref, K, seed):
    """uint8 [N, K]: all 4^K K-mers for K <= 8, else every K-mer of the reference and 2000 random ones; then, for every
    j < K, the last j bases of the reference padded to K with each base (they meet suffixes shorter than K)."""
    n = len(ref)
    if K <= 8:
        codes = np.arange(4 ** K, dtype=np.int64)
        body = ((codes[:, None] >> (2 * (K - 1 - np.arange(K)))) & 3).astype(np.uint8)
    else:
        own = np.lib.stride_tricks.sliding_window_view(ref, K) if n >= K else np.zeros((0, K), np.uint8)
        body = np.concatenate([own, np.random.default_rng(seed).integers(0, 4, (2000, K)).astype(np.uint8)])
    tails = []
    for j in range(0, min(K - 1, n) + 1):
        for b in range(4):
            tails.append(np.concatenate([ref[n - j:], np.full(K - j, b, np.uint8)]))
    return np.ascontiguousarray(np.concatenate([body, np.asarray(tails, np.uint8).reshape(-1, K)]), np.uint8)


def kmer_code(kmer):
    c = 0
    for b in kmer:
        c = (c << 2) | int(b)
    return c
