"""The specification of genie_match_stats_contigs and genie_find_smems_contigs restated in Python by brute force, on
references of at most 4096 bases.  Nothing here comes from the library under test.

ms_c, the contig-exact matching statistic, is restated twice, independently:

  per contig    the elementwise maximum over the contigs of smem_util.matching_stats(contig, run) on every break-free run
                of a strand-read, as match_stats_util.expected_one cuts the runs; empty contigs contribute nothing;
  by rows       facts 3 and 4 of the header on the suffix rows of the concatenation: the run starts of the concatenation's
                fwd[] are tested for an occurrence with room; where none has it, every position of the run is resolved by
                bisection over the length.  Also counts what the bisection met (for the guard against a vacuous suite).

lohi is lookup_util.interval of the ms_c bases on the concatenation; the SMEM rows are smem_util.smems(concatenation, run,
min_len, fwd=fwd_c).  Also the cases the host and GPU tests share and the raw calls of step_calls.py bound to this
pair of entry points."""
import numpy as np

import contig_util as CU
import lookup_util as U
import match_stats_util as MS
import smem_util as SM
import step_calls as SC

BOTH, SPLIT, FLAGS = CU.BOTH, CU.SPLIT, CU.FLAGS
_PER = {}            # (contig bytes, run bytes) -> fwd of the run against that contig
_ONE = {}            # (reference bytes, table bytes, strand-read bytes, split) -> expected_one


# ------------------------------------------------------------------ ms_c, twice
def ms_c_per_contig(ref, off, run):
    """ms_c of a break-free run: the maximum over the contigs of its matching statistics against each alone."""
    ref, off, run = np.asarray(ref, np.uint8), np.asarray(off, np.int64), np.asarray(run, np.uint8)
    at = np.arange(len(run), dtype=np.int64)
    best = np.zeros(len(run), np.int64)
    for c in range(len(off) - 1):
        a, b = int(off[c]), int(off[c + 1])
        if b == a:
            continue
        key = (U._bytes(ref[a:b]), U._bytes(run))
        if key not in _PER:
            _PER[key] = SM.matching_stats(ref[a:b], run) - at
        best = np.maximum(best, _PER[key])
    return best


def _best_room(ref, off, rows, pat):
    """The largest room among the occurrences of pat in the concatenation (0: none)."""
    lo, hi = U.interval(ref, rows, pat)
    if lo < 0:
        return 0
    t = rows[lo:hi + 1]
    t = t[t < len(ref)]
    return int((off[CU.contig_of(off, t) + 1] - t).max()) if t.size else 0


def ms_c_by_rows(ref, off, run, seen=None):
    """The same by facts 3 and 4.  seen (a dict) counts: run starts, flagged runs, positions of flagged runs that keep ms
    (resolved through another occurrence at full length), positions clipped."""
    ref, off, run = np.asarray(ref, np.uint8), np.asarray(off, np.int64), np.asarray(run, np.uint8)
    rows, L = U.suffix_rows(ref), len(run)
    fwd = SM.matching_stats(ref, run)
    ms = fwd - np.arange(L, dtype=np.int64)
    out = ms.copy()
    seen = seen if seen is not None else {}
    p0 = 0
    while p0 < L:
        p1 = p0 + 1
        while p1 < L and fwd[p1] == fwd[p0]:
            p1 += 1
        seen["starts"] = seen.get("starts", 0) + 1
        if ms[p0] > 0:
            room0 = _best_room(ref, off, rows, run[p0:p0 + ms[p0]])
            if room0 < ms[p0]:
                seen["flagged"] = seen.get("flagged", 0) + 1
                for p in range(p0, p1):
                    if ms[p] == 0:
                        continue
                    lo, hi = max(1, room0 - (p - p0)), int(ms[p]) + 1       # pred(lo) holds, pred(hi) does not
                    first = True
                    while hi - lo > 1:
                        mid = hi - 1 if first else (lo + hi) // 2
                        first = False
                        room = _best_room(ref, off, rows, run[p:p + mid])
                        if room >= mid:
                            lo = mid
                        else:
                            hi, lo = mid, max(lo, room)
                    out[p] = lo
                    seen["kept" if lo == ms[p] else "clipped"] = seen.get("kept" if lo == ms[p] else "clipped", 0) + 1
        p0 = p1
    return out


# ------------------------------------------------------------------ what the library has to answer
def _runs(read, ref, split):
    """The break-free runs [a, b) of a strand-read that is not flagged GENIE_READ_BAD_BASE."""
    if not split:
        return [(0, len(read))] if len(read) else []
    good = (read < 4) & np.isin(read, np.unique(ref))
    edges = np.flatnonzero(np.diff(np.concatenate([[0], good.astype(np.int8), [0]])))
    return list(zip(edges[::2].tolist(), edges[1::2].tolist()))


def expected_one(ref, off, read, split, ms_c=ms_c_per_contig):
    """(ms_c int32 [L], lohi int32 [L, 2], status, positions clipped) of one strand-read."""
    ref, off, read = np.asarray(ref, np.uint8), np.asarray(off, np.int64), np.asarray(read, np.uint8)
    key = (U._bytes(ref), off.tobytes(), U._bytes(read), bool(split), ms_c.__name__)
    if key in _ONE:
        return _ONE[key]
    ms0, _, status = MS.expected_one(ref, read, split)
    L, rows = len(read), U.suffix_rows(ref)
    ms, lohi = np.zeros(L, np.int32), np.full((L, 2), -1, np.int32)
    if status == MS.READ_BAD_BASE:
        res = (ms0.copy(), lohi, status, 0)
    else:
        for a, b in _runs(read, ref, split):
            ms[a:b] = ms_c(ref, off, read[a:b])
        for p, l in enumerate(ms.tolist()):
            if l > 0:
                lohi[p] = U.interval(ref, rows, read[p:p + l])
        res = (ms, lohi, status, int((ms < ms0).sum()))
    _ONE[key] = res
    return res


def expected_ms(ref, off, reads, flags, lead=0, tail=0, ms_c=ms_c_per_contig):
    """What genie_match_stats_contigs returns -> (ms [S total], lohi [S total, 2], status [S N], clipped)."""
    strands, split = (2 if flags & BOTH else 1), bool(flags & SPLIT)
    res = [expected_one(ref, off, r, split, ms_c) for r in MS.strand_reads(reads, strands)]
    pad = lambda n: (np.zeros(strands * n, np.int32), np.full((strands * n, 2), -1, np.int32))      # noqa: E731
    ms = np.concatenate([pad(lead)[0]] + [r[0] for r in res] + [pad(tail)[0]]).astype(np.int32)
    lohi = np.concatenate([pad(lead)[1]] + [r[1] for r in res] + [pad(tail)[1]]).astype(np.int32).reshape(-1, 2)
    return ms, lohi, np.asarray([r[2] for r in res], np.int32), sum(r[3] for r in res)


def smems_one(ref, off, read, split, mode="bwa", min_len=1, K=0):
    """(rows int32 [R, 4], status, positions clipped) of one strand-read: the traversal of smem_util.smems over fwd_c, per
    break-free run with SPLIT_BREAKS.  Statuses as smem_util.expected; a flagged strand-read has no rows and its positions
    are not counted."""
    ref, read = np.asarray(ref, np.uint8), np.asarray(read, np.uint8)
    if split:
        ms, _, _, clipped = expected_one(ref, off, read, True)
        out = [SM.NO_ROWS]
        for a, b in _runs(read, ref, True):
            rows, flagged = SM.smems(ref, read[a:b], min_len, fwd=ms[a:b].astype(np.int64) + np.arange(b - a))
            assert not flagged
            out.append(rows + np.asarray([a, a, 0, 0], np.int32))
        return np.concatenate(out), SM.READ_OK, clipped
    if len(read) and int(read.max()) > 3:
        return SM.NO_ROWS, SM.READ_BAD_BASE, 0
    if mode != "bwa":
        if len(read) < K:
            return SM.NO_ROWS, SM.READ_TOO_SHORT, 0
        min_len = 1
    ms, _, status, clipped = expected_one(ref, off, read, False)
    if status != MS.READ_OK:
        return SM.NO_ROWS, SM.READ_ABSENT_BASE, 0
    rows, flagged = SM.smems(ref, read, min_len, fwd=ms.astype(np.int64) + np.arange(len(read)))
    assert not flagged
    return rows, SM.READ_OK, clipped


def expected_smems(ref, off, reads, flags, mode="bwa", min_len=1, K=0):
    """What genie_find_smems_contigs returns -> (offsets int64 [S N + 1], rows int32 [R, 4], status int32 [S N], clipped)."""
    strands, split = (2 if flags & BOTH else 1), bool(flags & SPLIT)
    res = [smems_one(ref, off, r, split, mode, min_len, K) for r in MS.strand_reads(reads, strands)]
    offs = np.zeros(len(res) + 1, np.int64)
    offs[1:] = np.cumsum([len(x[0]) for x in res])
    rows = np.concatenate([SM.NO_ROWS] + [x[0] for x in res]).astype(np.int32).reshape(-1, 4)
    return offs, rows, np.asarray([x[1] for x in res], np.int32), sum(x[2] for x in res)


def concat_smems(ref, reads, flags, min_len=1):
    """smem_util.expected_batch of the strand-reads on the concatenation (BWA mode)."""
    strands, split = (2 if flags & BOTH else 1), bool(flags & SPLIT)
    return SM.expected_batch(ref, MS.strand_reads(reads, strands), "bwa", min_len, split=split)


# ------------------------------------------------------------------ the shared cases
class Case:
    def __init__(self, ref, off, reads, dir_bits=7):
        self.ref, self.off, self.reads, self.dir_bits = np.asarray(ref, np.uint8), np.asarray(off, np.int64), reads, dir_bits
        assert self.off[0] == 0 and self.off[-1] == len(self.ref) <= U.MAX_N and (np.diff(self.off) >= 0).all()

    @property
    def n_contigs(self):
        return len(self.off) - 1


JUNCTION_LENS = [0, 0, 1, 137, 0, 0, 61, 1, 300, 45, 260, 0, 90, 700, 33, 2, 120, 75, 0]      # 1825 bases in 19 contigs
JUNCTION_BACK = 60          # bases of a junction read in front of the boundary


def _junction_base():
    off = CU._offsets(JUNCTION_LENS)
    return U.family()["rand4096"][500:500 + int(off[-1])].copy(), off


def junction_reads(ref, off):
    """A read across every boundary of the concatenation, 1 to 40 bases into the neighbour (what is there of it), and the
    depths of the reads."""
    cuts = [int(b) for b in np.unique(off) if 0 < b < len(ref)]
    reads, depth = [], []
    for i, b in enumerate(cuts):
        d = 1 + (7 * i) % 40
        reads.append(ref[max(b - JUNCTION_BACK, 0):b + d].copy())
        depth.append(d)
    return reads, depth


def _junction_case(kind):
    """plain: the junction reads, a read longer than every contig, contigs of 0 and 1 base, two empty contigs in a row, an
    empty contig first and last.  copy: one more contig that holds every junction read whole, so that the full match has a
    second occurrence that does not bridge.  short: that contig holds each read without its first 20 bases instead (the
    positions from 20 on keep ms through it: a flagged run resolved at full length), every second one also without its last
    base: a shorter copy that still crosses the boundary (the bisection ends strictly between the room and ms)."""
    ref, off = _junction_base()
    reads, _ = junction_reads(ref, off)
    if kind == "plain":
        return Case(ref, off, reads + [ref[600:1500].copy(), np.zeros(0, np.uint8)])
    pieces = reads if kind == "copy" else [r[20:len(r) - (i & 1)] for i, r in enumerate(reads) if len(r) > 24]
    sep = np.asarray([0], np.uint8)
    extra = np.concatenate([np.concatenate([p, sep]) for p in pieces]).astype(np.uint8)
    return Case(np.concatenate([ref, extra]), np.concatenate([off, [off[-1] + len(extra)]]), reads)


TANDEM_FROM, TANDEM_TO = U.TANDEM_BREAK - 600, U.TANDEM_BREAK + 600
TANDEM_LONG = (540, 640)        # the one long contig: 60 bases of pure repeat, the substituted base, 39 more


def _tandem_case(name):
    """1200 bases of a tandem reference around its substituted base, cut into contigs of 3 to 50 bases except one of 120
    that holds 60 bases of pure repeat, the substitution and 39 more.  A 90-base read of pure repeat has hundreds of
    occurrences, all bridging; the 60 bases in front of the substituted base have as many, and the only one with room is the
    long contig's -- the LAST row of the interval where the substituted base is larger than the repeat's base there."""
    ref = U.family()[name][TANDEM_FROM:TANDEM_TO].copy()
    rng = np.random.default_rng(len(name))
    cuts, at = [0], 0
    while at < len(ref):
        step = int(rng.integers(3, 51))
        nxt = at + step
        if at < TANDEM_LONG[0] < nxt:
            nxt = TANDEM_LONG[0]
        elif at == TANDEM_LONG[0]:
            nxt = TANDEM_LONG[1]
        at = min(nxt, len(ref))
        cuts.append(at)
    off = np.asarray(cuts, np.int64)
    reads = [ref[100:190].copy(), ref[540:600].copy(), ref[535:615].copy(), ref[590:660].copy(), ref[1000:1130].copy(),
             ref[300:303].copy()]
    return Case(ref, off, reads)


def _window_case():
    """Reads of 255 .. 513 bases; a flagged run that starts at the last position of a window, one that starts at the first
    position of one, and one that spans three windows (700 bases in front of a boundary, 20 behind)."""
    lens = [900, 400, 800, 300, 1000]
    off = CU._offsets(lens)
    ref = U.family()["rand4096"][200:200 + int(off[-1])].copy()
    b1, b2, b3 = int(off[1]), int(off[2]), int(off[3])
    rng = np.random.default_rng(7)

    def junk(n, behind):
        j = rng.integers(0, 4, n).astype(np.uint8)
        j[-1] = CU._other(behind)                                 # no match runs from the junk into what follows it
        return j

    last = np.concatenate([junk(255, ref[b2 - 301]), ref[b2 - 300:b2 + 20]]).astype(np.uint8)
    first = np.concatenate([junk(256, ref[b3 - 201]), ref[b3 - 200:b3 + 30]]).astype(np.uint8)
    three = ref[b1 - 700:b1 + 20].copy()
    return Case(ref, off, MS.window_reads(ref) + [last, first, three])


def _passes_case():
    """With SPLIT_BREAKS more units than one pass holds: a break on every second position, then junction reads with breaks."""
    ref, off = _junction_base()
    reads, _ = junction_reads(ref, off)
    dense = ref[100:2000 - 300].copy()
    dense[1::2] = 7
    broken = []
    for r in reads[:8]:
        r = r.copy()
        r[len(r) // 3] = 7
        broken.append(r)
    return Case(ref, off, [dense] + broken + [ref[700:1100].copy()])


def _short_case():
    """Reads shorter than K = 12 beside longer ones, for the LUT and RMI modes."""
    ref, off = _junction_base()
    reads, _ = junction_reads(ref, off)
    return Case(ref, off, [ref[5:9].copy(), reads[3], ref[400:411].copy(), reads[6], np.zeros(0, np.uint8), ref[150:162].copy(), reads[9]])


def _from_contigs(name):
    c = CU.case(name)
    return Case(c.ref, c.off, c.reads, c.dir_bits)



def cases():
    """name -> Case: every shape the GPU tests run, checked on the host first (tests/test_contig_stats_host.py)."""
    out = {"ctg_" + n: (lambda n=n: _from_contigs(n)) for n in CU.cases()}                 # every one of them
    out.update({"junction": lambda: _junction_case("plain"), "junction_copy": lambda: _junction_case("copy"),
                "junction_short": lambda: _junction_case("short"), "windows": _window_case, "passes": _passes_case,
                "short": _short_case})
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


def bad_tables(c):
    """Eight tables that genie_contigs_validate refuses."""
    n, off, nc = len(c.ref), c.off, c.n_contigs
    first, order, last = off.copy(), off.copy(), off.copy()
    first[0] = 1
    order[len(off) // 2] = order[min(len(off) // 2 + 1, nc)] + 1
    last[-1] = n + 1
    return {"first": first, "order": order, "last": last, "huge": np.full(nc + 1, 2**62, np.int64), "negative": -off - 1,
            "noise": np.random.default_rng(nc).integers(-2**40, 2**40, nc + 1), "reversed": off[::-1].copy() + 1,
            "zeros": np.zeros(nc + 1, np.int64)}


# ------------------------------------------------------------------ the raw calls (step_calls.py, bound to this pair)
def _bound(call):
    """call(lib, ix, off, flags, bases, offs, ...) of step_calls' function of that name, the last result the clipped positions."""
    return lambda lib, ix, off, flags, *args, **kw: call(SC.Pair("contigs", table=off), lib, ix, flags, *args, **kw)


ms_call, smem_call, sized_smem_call = _bound(SC.ms_call), _bound(SC.smem_call), _bound(SC.sized_smem_call)


def guarded_calls(lib, ix, a, s, off, flags, reads, cap):
    return SC.guarded_calls(SC.Pair("contigs", table=off), lib, ix, a, s, flags, reads, cap)
