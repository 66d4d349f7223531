"""Brute-force reference for the SMEM calls (genie_find_smems* in every mode): matching statistics and the get_SMEMS
traversal stated in terms of substring membership, on the sorted suffix strings of tests/lookup_util.py.  Plain Python and
NumPy; nothing here comes from the library under test or from the C oracle (test_tuning_knobs_host.py pins both against
this).  Also the read batches the tuning-knob tests run on every reference of lookup_util.family(): they and their
expected rows depend on the reference alone -- not on dir_bits, table_bits, the table form, K or any launch option -- so
they are made once per process.

The traversal (SMEM.get_SMEMS): pivot i = 0; while i < L, fend = the largest e with read[i:e] in the reference (fend == i:
the base occurs nowhere, the read is flagged); for every e in i + 1 .. fend, s(e) = the smallest s <= i with read[s:e] in
the reference; the row is the (s, e) of the largest e - s, the smaller e on a tie; it is emitted if e - s >= min_len, and
the next pivot is e.  Rows are (start, end, lo, hi) with [lo, hi] = lookup_util.interval of read[start:end]."""
import bisect
import functools

import numpy as np

import lookup_util as U

READ_OK, READ_BAD_BASE, READ_TOO_SHORT, READ_ABSENT_BASE = 0, 1, 2, 3
NO_ROWS = np.zeros((0, 4), np.int32)


def _occurs(sufs, p):
    k = bisect.bisect_left(sufs, p)
    return k < len(sufs) and sufs[k].startswith(p)


def matching_stats(ref, read):
    """fwd[a] = the end of the longest prefix of read[a:] that occurs in ref (fwd[a] == a: read[a] occurs nowhere).
    fwd is non-decreasing: a match that starts at a, shortened by its first base, starts at a + 1."""
    sufs, q = U._sorted_suffixes(ref), U._bytes(read)
    L = len(q)
    fwd = np.zeros(L, np.int64)
    e = 0
    for a in range(L):
        e = max(e, a)
        while e < L and _occurs(sufs, q[a:e + 1]):
            e += 1
        fwd[a] = e
    return fwd


def _row(ref, rows, read, s, e):
    lo, hi = U.interval(ref, rows, read[s:e])
    assert 0 <= lo <= hi
    return (s, e, lo, hi)


def smems_quadratic(ref, read, min_len):
    """The traversal as the module docstring states it, with `bytes in bytes`.  -> (rows int32 [S, 4], flagged)."""
    r, q = U._bytes(ref), U._bytes(read)
    rows, L = U.suffix_rows(ref), len(q)
    out, i = [], 0
    while i < L:
        fend = i
        while fend < L and q[i:fend + 1] in r:
            fend += 1
        if fend == i:
            return NO_ROWS, True
        best = None
        for e in range(i + 1, fend + 1):
            s = i
            while s > 0 and q[s - 1:e] in r:
                s -= 1
            if best is None or e - s > best[1] - best[0]:
                best = (s, e)
        if best[1] - best[0] >= min_len:
            out.append(_row(ref, rows, read, *best))
        i = best[1]
    return np.asarray(out, np.int32).reshape(-1, 4), False


def smems(ref, read, min_len, fwd=None):
    """The same rows from fwd[] in time linear in the read (plus the windows looked at): s(e) is the smallest s with
    fwd[s] >= e, and it is monotone in e, so the best (s, e) of pivot i is the first maximum of fwd[s] - s over
    s0 <= s <= i, s0 = the first s with fwd[s] > i, with e = fwd[s].  -> (rows int32 [S, 4], flagged)."""
    if fwd is None:
        fwd = matching_stats(ref, read)
    rows, L = U.suffix_rows(ref), len(fwd)
    at = np.arange(L, dtype=np.int64)
    out, i = [], 0
    while i < L:
        if fwd[i] == i:
            return NO_ROWS, True
        s0 = int(np.searchsorted(fwd, i, side="right"))
        s = s0 + int(np.argmax(fwd[s0:i + 1] - at[s0:i + 1]))
        e = int(fwd[s])
        if e - s >= min_len:
            out.append(_row(ref, rows, read, s, e))
        i = e
    return np.asarray(out, np.int32).reshape(-1, 4), False


# ------------------------------------------------------------------ what the library has to answer
_BWA1 = {}          # (reference bytes, read bytes) -> (rows with min_len 1, flagged)


def bwa_rows(ref, read):
    """smems(ref, read, 1), remembered.  min_len m keeps the rows of at least m bases: the pivots do not depend on it."""
    key = (U._bytes(ref), U._bytes(read))
    if key not in _BWA1:
        _BWA1[key] = smems(ref, read, 1)
    return _BWA1[key]


def expected(ref, read, mode, min_len=1, K=0):
    """(status, rows) of one read.  bwa: the traversal with min_len.  lut / rmi: the bwa rows with min_len 1 for a read
    of at least K bases (the equivalence test_mode_equivalence.py establishes), GENIE_READ_TOO_SHORT below.  A code > 3
    flags the read GENIE_READ_BAD_BASE first; a base that the reference lacks, GENIE_READ_ABSENT_BASE last."""
    read = np.asarray(read, np.uint8)
    if len(read) and int(read.max()) > 3:
        return READ_BAD_BASE, NO_ROWS
    if mode != "bwa":
        if len(read) < K:
            return READ_TOO_SHORT, NO_ROWS
        min_len = 1
    rows, flagged = bwa_rows(ref, read)
    if flagged:
        return READ_ABSENT_BASE, NO_ROWS
    return READ_OK, rows[rows[:, 1] - rows[:, 0] >= min_len]


def expected_split(ref, read, min_len=1):
    """Rows of genie_find_smems_split: a break is a code > 3 or a base the reference lacks; the rows of every run between
    breaks, in read order, with start / end in the whole read.  The status is always GENIE_READ_OK."""
    read = np.asarray(read, np.uint8)
    ok = np.isin(read, np.unique(ref))
    edges = np.flatnonzero(np.diff(np.concatenate([[0], ok.astype(np.int8), [0]])))
    out = [NO_ROWS]
    for a, b in zip(edges[::2], edges[1::2]):
        st, rows = expected(ref, read[a:b], "bwa", min_len)
        assert st == READ_OK
        out.append(rows + np.asarray([a, a, 0, 0], np.int32))
    return READ_OK, np.concatenate(out)


def expected_batch(ref, reads, mode, min_len=1, K=0, split=False):
    """reads: a list of uint8 arrays -> (offsets int64 [N + 1], rows int32 [S, 4], status int32 [N]) as the CSR entry
    points return them."""
    res = [expected_split(ref, r, min_len) if split else expected(ref, r, mode, min_len, K) for r in reads]
    off = np.zeros(len(res) + 1, np.int64)
    off[1:] = np.cumsum([len(rows) for _, rows in res])
    return off, np.concatenate([NO_ROWS] + [rows for _, rows in res]), np.asarray([st for st, _ in res], np.int32)


# ------------------------------------------------------------------ the read batches
TAIL_TS = (1, 5, 6, 7, 8, 11, 12, 13)
FULL_LENGTHS = (31, 32, 33, 64, 150, 255)                    # every kind; the lengths below get one tail and one repeat
SHORT_LENGTHS = tuple(range(1, 18)) + FULL_LENGTHS           # 1 .. 17 holds K - 1, K and K + 1 for every K up to 16
MID_LENGTHS = (256, 705, 1409)
LONG_LENGTH = 9000
# On a tandem reference the 9000-base reads that repeat the unit for more than 1520 bases (the unit tile, one base repeated)
# are in the "long" batch cut down to that -- past the longest match the reference allows, TANDEM_BREAK = 1500 bases -- and
# go on with random bases; the reads as they were are the "long_extra" batch.  The literal oracle extends backwards from
# every forward match of every pivot and needs a minute per mode for 9000 bases of one unit, so "long_extra" is pinned on
# the host by the definition of an SMEM alone (test_tuning_knobs_host.py), and both batches run on the device.
TANDEM_LONG_REPEAT = U.TANDEM_BREAK + 20
BAD_CODE = 7


def _reads_of_length(name, ref, L, rng, full):
    """One read of L bases of every kind that exists at that length on this reference (module docstring of
    test_tuning_knobs_gpu.py lists them); bases are drawn from those the reference holds.  The last two reads are the
    designated flagged ones: a base the reference lacks (where it lacks one), then a code 7."""
    n, present = len(ref), np.unique(ref)

    def rnd(m):
        return present[rng.integers(0, len(present), m)].astype(np.uint8)

    def cut(s):                                              # ref[s : s + L]; random bases where the reference has ended
        p = ref[s:s + L]
        return np.concatenate([p, rnd(L - len(p))]).astype(np.uint8)

    def anywhere():
        return int(rng.integers(0, max(n - L, 0) + 1))

    out = [rnd(L)]
    buf = []
    while sum(len(b) for b in buf) < L:                      # reference pieces of 1 .. 30 bases
        p = int(rng.integers(0, n))
        buf.append(ref[p:p + int(rng.integers(1, 31))])
    out.append(np.concatenate(buf)[:L].astype(np.uint8))
    out += [cut(anywhere()), cut(0), cut(max(n - L, 0))]
    if len(present) > 1:                                     # one substitution
        c, at = cut(anywhere()), int(rng.integers(0, L))
        others = present[present != c[at]]
        c[at] = others[rng.integers(0, len(others))]
        out.append(c)
    for t in (TAIL_TS if full else (TAIL_TS[L % len(TAIL_TS)],)):
        if t < L and t <= n:                                 # the last t bases of the reference, then random ones
            out.append(np.concatenate([ref[n - t:], rnd(L - t)]).astype(np.uint8))
    for b in (present if full else present[:1]):             # one base repeated (present[0] is A wherever A occurs)
        out.append(np.full(L, b, np.uint8))
    ends = [p for p in range(L, n) if ref[p] == 0]           # the read ends at p and the reference goes on with A
    if ends:
        run = lambda p: next(j for j in range(n - p + 1) if p + j == n or ref[p + j] != 0)      # noqa: E731
        p = max(ends, key=run)
        out += [ref[p - L:p].copy(), ref[p + run(p) // 2 - L:p + run(p) // 2].copy()]
    if U.is_tandem(name):
        u = int(name[len("tandem"):])
        brk = U.TANDEM_BREAK
        for s in ((brk - L // 2) // u * u, brk - L + 1, brk - L):       # across, up to and short of the substituted base
            if 0 <= s and s + L <= n:
                out.append(ref[s:s + L].copy())
        out.append(np.tile(U._codes(U.TANDEM_UNITS[u]), L // u + 1)[:L])
    lacks = np.setdiff1d(np.arange(4, dtype=np.uint8), present)
    if len(lacks):
        c = rnd(L)
        c[(0, L - 1, L // 2)[L % 3]] = lacks[-1]
        out.append(c)
    c = cut(anywhere())
    c[int(rng.integers(0, L))] = BAD_CODE
    out.append(c)
    assert all(len(r) == L and r.dtype == np.uint8 for r in out)
    return out


@functools.lru_cache(maxsize=None)
def batches(name):
    """The batches of one reference: {"short": {L: [reads]}, "mid": {L: [reads]}, "long": [reads of 9000 bases],
    "long_extra": [more of them, on tandem references], "ragged": [reads of mixed lengths, 0 among them]} -- lists of
    uint8 arrays."""
    ref = U.family()[name]
    rng = np.random.default_rng(sum(name.encode()) + len(ref))

    def dozen(L):
        reads = []
        if L > 255:                                          # two more reads, random and stitched, at the longer lengths
            reads += _reads_of_length(name, ref, L, rng, False)[:2]
        return reads + _reads_of_length(name, ref, L, rng, L in FULL_LENGTHS)

    out = {"short": {L: dozen(L) for L in SHORT_LENGTHS}, "mid": {L: dozen(L) for L in MID_LENGTHS},
           "long": dozen(LONG_LENGTH), "long_extra": []}
    if U.is_tandem(name):
        u, present = int(name[len("tandem"):]), np.unique(ref)
        for i, r in enumerate(out["long"]):
            same = np.concatenate([[0], (r[u:] == r[:-u]).astype(np.int64), [0]])
            gaps = np.flatnonzero(same == 0)
            if int(np.diff(gaps).max()) - 1 + u > TANDEM_LONG_REPEAT:           # the longest stretch of period u
                out["long_extra"].append(r)
                fill = present[rng.integers(0, len(present), LONG_LENGTH - TANDEM_LONG_REPEAT)].astype(np.uint8)
                out["long"][i] = np.concatenate([r[:TANDEM_LONG_REPEAT], fill])
    ragged = [np.zeros(0, np.uint8)]
    for L in SHORT_LENGTHS:
        ragged += out["short"][L][-3:] + out["short"][L][1:3]
    ragged += [np.zeros(0, np.uint8), out["short"][255][0], np.zeros(0, np.uint8)]
    out["ragged"] = ragged
    return out


def matrix(reads, stride=None, fill=9):
    """Reads -> (uint8 [N, stride] with `fill` behind every read, int32 lengths)."""
    return U.pack_rows(reads, stride, fill)


def csr(reads):
    """Reads -> (uint8 bases back to back, int64 [N + 1] offsets) as genie_find_smems_long takes them."""
    off = np.zeros(len(reads) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in reads])
    return (np.concatenate(reads).astype(np.uint8) if len(reads) else np.zeros(0, np.uint8)), off
