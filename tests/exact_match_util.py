"""The specification of genie_exact_match restated in Python on the brute force of tests/lookup_util.py (intervals by
bisecting the sorted suffix strings), for references of at most 4096 bases.  Nothing here comes from the library under
test.

S = 2 with both strands, else 1; strand-pattern S i + s is pattern i (s = 0) or its reverse complement (s = 1: reversed,
code c -> 3 - c, a code > 3 stays what it is).  For strand-pattern q:
  lohi[q]    lookup_util.interval of it: the inclusive rows, (-1, -1) if it occurs nowhere (a base the reference lacks is
             nothing special), (0, n) for the empty pattern; (-2, -2) if it holds a code > 3
  counts[q]  hi - lo + 1; 0 where absent or bad, n + 1 for the empty pattern
  status[q]  READ_BAD_BASE for (-2, -2), else READ_OK"""
import numpy as np

import lookup_util as U

BOTH, SPLIT = 1, 2
READ_OK, READ_BAD_BASE = 0, 1
BAD = (-2, -2)


def rc(pat):
    out = np.asarray(pat, np.uint8)[::-1].copy()
    out[out < 4] ^= 3
    return out


def strand_patterns(pats, strands):
    """[p0, rc(p0), p1, rc(p1), ...] for two strands, the patterns themselves for one."""
    out = []
    for p in pats:
        out.append(np.asarray(p, np.uint8))
        if strands == 2:
            out.append(rc(p))
    return out


def expected_one(ref, rows, pat):
    """((lo, hi), count, status) of one strand-pattern."""
    pat = np.asarray(pat, np.uint8)
    if (pat > 3).any():
        return BAD, 0, READ_BAD_BASE
    lo, hi = U.interval(ref, rows, pat)
    return (lo, hi), (hi - lo + 1 if lo >= 0 else 0), READ_OK


def expected(ref, pats, flags=0, rows=None):
    """-> (lohi int32 [S N, 2], counts int32 [S N], status int32 [S N])."""
    rows = U.suffix_rows(ref) if rows is None else rows
    res = [expected_one(ref, rows, p) for p in strand_patterns(pats, 2 if flags & BOTH else 1)]
    return (np.asarray([r[0] for r in res], np.int32).reshape(-1, 2), np.asarray([r[1] for r in res], np.int32),
            np.asarray([r[2] for r in res], np.int32))


def csr(pats, lead=0, tail=0, fill=9):
    """Patterns -> (uint8 bases, int64 [N + 1] offsets) with `lead` / `tail` bytes of `fill` around them."""
    off = np.zeros(len(pats) + 1, np.int64)
    off[1:] = np.cumsum([len(p) for p in pats])
    parts = [np.full(lead, fill, np.uint8)] + [np.asarray(p, np.uint8) for p in pats] + [np.full(tail, fill, np.uint8)]
    return np.concatenate(parts).astype(np.uint8), off + lead


def occurrences(ref, pat):
    """0-based starts of every (overlapping) occurrence of pat in ref, by bytes.find: for references beyond the brute force."""
    r, p = U._bytes(ref), U._bytes(pat)
    out, at = [], r.find(p)
    while at >= 0:
        out.append(at)
        at = r.find(p, at + 1)
    return out
