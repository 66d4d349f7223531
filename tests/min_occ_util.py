"""The specification of genie_match_stats_min_occ and genie_find_smems_min_occ restated in Python by brute force, on
references of at most 4096 bases.  Nothing here comes from the library under test.

occ(w) is the number of positions of the reference at which w starts.  ms_k, the matching statistic under a minimum
occurrence count k, is restated twice, independently:

  naive         ms_k_naive: for every position the occurrences of its first base, narrowed base by base (a comparison of
                the reference with the read, nothing else) until fewer than k are left;
  by rows       ms_k_by_rows: fact 5 of the header on a suffix array built in NumPy by prefix doubling and the LCPs of its
                neighbouring rows: where the interval [lo, hi] of the full match has fewer than k rows,
                ms_k = max over a in [max(1, hi-k+1), min(lo, R-k)] of min(ms, lcp(SA[a], SA[a+k-1])).  Also counts what
                it met (for the guard against a vacuous suite).

A base RARE AT K occurs fewer than k times.  Without SPLIT_BREAKS a strand-read that holds one is flagged
GENIE_READ_ABSENT_BASE (no SMEM rows; its statistics stand); with it the base is a break.  `shortened` (d_totals) counts the
positions with ms_k < ms, ms being the matching statistic under the same breaks.  lohi is lookup_util.interval of the ms_k
bases; the SMEM rows are smem_util.smems(reference, run, min_len, fwd=fwd_k).  Also the cases the host and GPU tests share
and the raw calls of step_calls.py bound to this pair of entry points."""
import numpy as np

import contig_util as CU
import lookup_util as U
import match_stats_util as MS
import smem_util as SM
import step_calls as SC

BOTH, SPLIT, FLAGS = CU.BOTH, CU.SPLIT, CU.FLAGS
KS = (1, 2, 3, 11, 32, 33, 65, 1000)
_NAIVE, _SA, _WIN, _ONE = {}, {}, {}, {}


# ------------------------------------------------------------------ ms_k, twice
def ms_k_naive(ref, run, k):
    """ms_k of a break-free run by counting substrings."""
    ref, run = np.asarray(ref, np.uint8), np.asarray(run, np.uint8)
    key = (U._bytes(ref), U._bytes(run), int(k))
    if key in _NAIVE:
        return _NAIVE[key]
    n, L = len(ref), len(run)
    out = np.zeros(L, np.int64)
    starts = [np.flatnonzero(ref == b) for b in range(4)]
    for p in range(L):
        cand = starts[int(run[p])] if run[p] < 4 else np.zeros(0, np.int64)
        l = 0
        while len(cand) >= k:
            l += 1
            if p + l >= L:
                break
            cand = cand[cand + l < n]
            cand = cand[ref[cand + l] == run[p + l]]
        out[p] = l
    _NAIVE[key] = out
    return out


def suffix_array(ref):
    """(rows int64 [n + 1] of suffix starts, '$' first; lcp int64 [n + 1], lcp[j] = LCP of rows j - 1 and j, lcp[0] = 0) by
    prefix doubling in NumPy."""
    ref = np.asarray(ref, np.uint8)
    key = U._bytes(ref)
    if key in _SA:
        return _SA[key]
    n = len(ref)
    rank = np.concatenate([ref.astype(np.int64) + 1, [0]])
    h = 1
    while True:
        nxt = np.concatenate([rank[h:], np.zeros(min(h, n + 1), np.int64)])[:n + 1]
        order = np.lexsort((nxt, rank))
        changed = np.concatenate([[0], ((rank[order][1:] != rank[order][:-1]) | (nxt[order][1:] != nxt[order][:-1])).astype(np.int64)])
        new = np.empty(n + 1, np.int64)
        new[order] = np.cumsum(changed)
        rank = new
        if rank.max() == n:
            break
        h *= 2
    rows = np.argsort(rank).astype(np.int64)
    lcp = np.zeros(n + 1, np.int64)
    for j in range(1, n + 1):
        a, b = ref[rows[j - 1]:], ref[rows[j]:]
        m = min(len(a), len(b))
        d = np.flatnonzero(a[:m] != b[:m])
        lcp[j] = d[0] if len(d) else m
    _SA[key] = (rows, lcp)
    return rows, lcp


def _window_lcp(ref, k):
    """W[a] = lcp(SA[a], SA[a + k - 1]) for a in [0, R - k]; for k == 1 the suffix's own length."""
    key = (U._bytes(ref), int(k))
    if key not in _WIN:
        rows, lcp = suffix_array(ref)
        R = len(rows)
        if k == 1:
            w = len(ref) - rows
        elif k > R:
            w = np.zeros(0, np.int64)
        else:
            w = np.lib.stride_tricks.sliding_window_view(lcp[1:], k - 1).min(axis=1)       # over lcp[a+1 .. a+k-1]
            assert len(w) == R - k + 1
        _WIN[key] = w
    return _WIN[key]


def ms_k_by_rows(ref, run, k, seen=None):
    """The same by facts 3 and 5.  seen (a dict) counts: run starts, failed run starts, positions of failed runs that keep ms
    (their own interval has k rows), positions shortened to a length > 0, positions shortened to 0."""
    ref, run = np.asarray(ref, np.uint8), np.asarray(run, np.uint8)
    rows, _ = suffix_array(ref)
    assert np.array_equal(rows, U.suffix_rows(ref))
    R, L = len(rows), len(run)
    fwd = SM.matching_stats(ref, run)
    ms = fwd - np.arange(L, dtype=np.int64)
    out = ms.copy()
    W = _window_lcp(ref, k)
    seen = seen if seen is not None else {}

    def bump(name):
        seen[name] = seen.get(name, 0) + 1

    p0 = 0
    while p0 < L:
        p1 = p0 + 1
        while p1 < L and fwd[p1] == fwd[p0]:
            p1 += 1
        bump("starts")
        if ms[p0] > 0:
            lo, hi = U.interval(ref, rows, run[p0:p0 + ms[p0]])
            if hi - lo + 1 < k:
                bump("failed")
                for p in range(p0, p1):
                    if ms[p] == 0:
                        continue
                    lo, hi = U.interval(ref, rows, run[p:p + ms[p]])
                    if hi - lo + 1 >= k:
                        bump("kept")
                        continue
                    a0, a1 = max(1, hi - k + 1), min(lo, R - k)
                    best = int(W[a0:a1 + 1].max()) if a1 >= a0 else 0
                    out[p] = min(int(ms[p]), best)
                    bump("shortened" if out[p] > 0 else "rare")
        p0 = p1
    return out


# ------------------------------------------------------------------ what the library has to answer
def usable(ref, k):
    """The base codes that occur at least k times."""
    return np.flatnonzero(np.bincount(np.asarray(ref, np.uint8), minlength=4)[:4] >= k).astype(np.uint8)


def _runs(read, ref, split, k):
    """The break-free runs [a, b) of a strand-read that is not flagged GENIE_READ_BAD_BASE."""
    if not split:
        return [(0, len(read))] if len(read) else []
    good = (read < 4) & np.isin(read, usable(ref, k))
    edges = np.flatnonzero(np.diff(np.concatenate([[0], good.astype(np.int8), [0]])))
    return list(zip(edges[::2].tolist(), edges[1::2].tolist()))


def expected_one(ref, read, split, k, ms_k=ms_k_naive):
    """(ms_k int32 [L], lohi int32 [L, 2], status, positions shortened) of one strand-read."""
    ref, read = np.asarray(ref, np.uint8), np.asarray(read, np.uint8)
    key = (U._bytes(ref), U._bytes(read), bool(split), int(k), ms_k.__name__)
    if key in _ONE:
        return _ONE[key]
    L, rows = len(read), U.suffix_rows(ref)
    ms, lohi = np.zeros(L, np.int32), np.full((L, 2), -1, np.int32)
    if not split and (read > 3).any():
        res = (np.full(L, -1, np.int32), lohi, MS.READ_BAD_BASE, 0)
    else:
        short = 0
        for a, b in _runs(read, ref, split, k):
            ms[a:b] = ms_k(ref, read[a:b], k)
            short += int((ms[a:b] < SM.matching_stats(ref, read[a:b]) - np.arange(b - a)).sum())
        for p, l in enumerate(ms.tolist()):
            if l > 0:
                lohi[p] = U.interval(ref, rows, read[p:p + l])
                assert lohi[p, 1] - lohi[p, 0] + 1 >= k
        rare = (not split) and bool((ms == 0).any())
        res = (ms, lohi, MS.READ_ABSENT_BASE if rare else MS.READ_OK, short)
    _ONE[key] = res
    return res


def expected_ms(ref, reads, flags, k, lead=0, tail=0, ms_k=ms_k_naive):
    """What genie_match_stats_min_occ returns -> (ms [S total], lohi [S total, 2], status [S N], shortened)."""
    strands, split = (2 if flags & BOTH else 1), bool(flags & SPLIT)
    res = [expected_one(ref, r, split, k, ms_k) for r in MS.strand_reads(reads, strands)]
    pad = lambda n: (np.zeros(strands * n, np.int32), np.full((strands * n, 2), -1, np.int32))      # noqa: E731
    ms = np.concatenate([pad(lead)[0]] + [r[0] for r in res] + [pad(tail)[0]]).astype(np.int32)
    lohi = np.concatenate([pad(lead)[1]] + [r[1] for r in res] + [pad(tail)[1]]).astype(np.int32).reshape(-1, 2)
    return ms, lohi, np.asarray([r[2] for r in res], np.int32), sum(r[3] for r in res)


def smems_one(ref, read, split, k, mode="bwa", min_len=1, K=0):
    """(rows int32 [R, 4], status, positions shortened) of one strand-read: the traversal of smem_util.smems over fwd_k, per
    break-free run with SPLIT_BREAKS.  A flagged strand-read has no rows and its positions are not counted."""
    ref, read = np.asarray(ref, np.uint8), np.asarray(read, np.uint8)
    if split:
        ms, _, _, short = expected_one(ref, read, True, k)
        out = [SM.NO_ROWS]
        for a, b in _runs(read, ref, True, k):
            rows, flagged = SM.smems(ref, read[a:b], min_len, fwd=ms[a:b].astype(np.int64) + np.arange(b - a))
            assert not flagged
            out.append(rows + np.asarray([a, a, 0, 0], np.int32))
        return np.concatenate(out), SM.READ_OK, short
    if len(read) and int(read.max()) > 3:
        return SM.NO_ROWS, SM.READ_BAD_BASE, 0
    if mode != "bwa":
        if len(read) < K:
            return SM.NO_ROWS, SM.READ_TOO_SHORT, 0
        min_len = 1
    ms, _, status, short = expected_one(ref, read, False, k)
    if status != MS.READ_OK:
        return SM.NO_ROWS, SM.READ_ABSENT_BASE, 0
    rows, flagged = SM.smems(ref, read, min_len, fwd=ms.astype(np.int64) + np.arange(len(read)))
    assert not flagged
    return rows, SM.READ_OK, short


def expected_smems(ref, reads, flags, k, mode="bwa", min_len=1, K=0):
    """What genie_find_smems_min_occ returns -> (offsets int64 [S N + 1], rows int32 [R, 4], status int32 [S N], shortened)."""
    strands, split = (2 if flags & BOTH else 1), bool(flags & SPLIT)
    res = [smems_one(ref, r, split, k, mode, min_len, K) for r in MS.strand_reads(reads, strands)]
    offs = np.zeros(len(res) + 1, np.int64)
    offs[1:] = np.cumsum([len(x[0]) for x in res])
    rows = np.concatenate([SM.NO_ROWS] + [x[0] for x in res]).astype(np.int32).reshape(-1, 4)
    return offs, rows, np.asarray([x[1] for x in res], np.int32), sum(x[2] for x in res)


# ------------------------------------------------------------------ the shared cases
class Case:
    def __init__(self, ref, reads, dir_bits=7):
        self.ref, self.reads, self.dir_bits = np.asarray(ref, np.uint8), reads, dir_bits
        assert len(self.ref) <= U.MAX_N


def _iid_ref():
    """3000 i.i.d. bases in which [2000, 2060) repeats [500, 560): a read over [480, 560) starts a run that occurs once and
    whose positions from 20 on occur twice at full length."""
    ref = U.family()["rand4096"][:3000].copy()
    ref[2000:2060] = ref[500:560]
    ref[1999], ref[2060] = CU._other(ref[499]), CU._other(ref[560])
    return ref


def _junk(rng, n, behind):
    j = rng.integers(0, 4, n).astype(np.uint8)
    j[-1] = CU._other(behind)                                     # no match runs from the junk into what follows it
    return j


def _iid_case():
    """Window reads (255 .. 513 bases), the repeat read, run starts at positions 255 and 256, one run of 720 positions (three
    windows) that fails at every k >= 2, reads with break codes, an empty read."""
    ref = _iid_ref()
    rng = np.random.default_rng(11)
    at255 = np.concatenate([_junk(rng, 255, ref[899]), ref[900:1200]]).astype(np.uint8)
    at256 = np.concatenate([_junk(rng, 256, ref[1299]), ref[1300:1530]]).astype(np.uint8)
    broken = ref[100:400].copy()
    broken[[0, 150, 255, 256, 299]] = 7
    return Case(ref, MS.window_reads(ref) + [ref[480:560].copy(), at255, at256, ref[1000:1720].copy(), broken, np.zeros(0, np.uint8),
                                             ref[2990:3000].copy()])


def _tandem_case(name):
    """Reads of 3 to 130 bases of a tandem reference around its substituted base: intervals of hundreds of rows, so every k
    of KS but 1000 (and, for the unit G, that one too) leaves some matches whole and cuts others."""
    ref = U.family()[name]
    b = U.TANDEM_BREAK
    reads = [ref[100:190].copy(), ref[b - 60:b].copy(), ref[b - 65:b + 15].copy(), ref[b - 10:b + 60].copy(), ref[2500:2630].copy(),
             ref[300:303].copy(), ref[len(ref) - 40:].copy()]
    return Case(ref, reads)


def _once_case():
    """Twelve bases in which T occurs once and G three times: T is rare at 2, G at 11; reads with T in front, inside, last,
    twice in a row, a read of T alone, one without it."""
    ref = U._codes("ACGACGACCACT")
    reads = [U._codes(s) for s in ("ACGACT", "TACGAC", "ACGTTACG", "T", "ACGACC", "CCACTA", "")]
    broken = U._codes("ACGACCACGT")
    broken[3] = 7
    return Case(ref, reads + [broken], dir_bits=2)


def _passes_case():
    """With SPLIT_BREAKS more units than one pass holds: a break on every second position, then reads with a few breaks."""
    ref = _iid_ref()
    dense = ref[100:1700].copy()
    dense[1::2] = 7
    some = []
    for s in (300, 480, 900, 2500):
        r = ref[s:s + 90].copy()
        r[30] = 7
        some.append(r)
    return Case(ref, [dense] + some + [ref[700:1100].copy()])


def _short_case():
    """Reads shorter than K = 12 beside longer ones, for the LUT and RMI modes."""
    ref = _iid_ref()
    return Case(ref, [ref[5:9].copy(), ref[480:560].copy(), ref[400:411].copy(), ref[2000:2070].copy(), np.zeros(0, np.uint8),
                      ref[150:162].copy(), ref[1000:1200].copy()])


def cases():
    """name -> Case: every shape the GPU tests run, checked on the host first (tests/test_min_occ_host.py)."""
    out = {"iid": _iid_case, "once": _once_case, "passes": _passes_case, "short": _short_case}
    out.update({n: (lambda n=n: _tandem_case(n)) for n in U.family() if U.is_tandem(n)})
    return out


_MAKERS, _CASES = None, {}


def case(name):
    global _MAKERS
    if _MAKERS is None:
        _MAKERS = cases()
    if name not in _CASES:
        _CASES[name] = _MAKERS[name]()
    return _CASES[name]


# ------------------------------------------------------------------ the raw calls (step_calls.py, bound to this pair)
def _bound(call):
    """call(lib, ix, flags, k, bases, offs, ...) of step_calls' function of that name, the last result the positions shortened."""
    return lambda lib, ix, flags, k, *args, **kw: call(SC.Pair("min_occ", extra=(k,)), lib, ix, flags, *args, **kw)


ms_call, smem_call, sized_smem_call = _bound(SC.ms_call), _bound(SC.smem_call), _bound(SC.sized_smem_call)


def guarded_calls(lib, ix, a, s, flags, k, reads, cap):
    return SC.guarded_calls(SC.Pair("min_occ", extra=(k,)), lib, ix, a, s, flags, reads, cap)
