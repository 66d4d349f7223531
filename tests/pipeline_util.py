"""The paired pipeline end to end on the CPU: SMEM.map_pairs and SMEM.sam_text restated as the composition of the stage brute
forces of tests/*_util.py, from the reads to the SAM bytes with no device result in between; a simulator of noisy read pairs
with a truth table; and check_sam, a checker of SAM text that parses the bytes itself and shares no code with either side.

  simulator      reference() -> a 4096-base three-contig reference with an exact 300-base duplication and a tandem repeat;
                 library(seed) and hard(seed) -> Batch: reads as CSR codes, names, qualities and one Truth row per mate.
  host pipeline  host_pipeline(...) -> HostRun: every intermediate of map_pairs in the order its docstring names them;
                 host_map_pairs(...) -> the tuple SMEM.map_pairs returns, as numpy arrays; host_sam_text(...) -> sam_text's.
  checker        check_sam(text, line_offsets, T, table, contig_names, reads, names, align_params).

Stage order (SMEM.map_pairs): MEMs (contig_util / mems_util) -> chains (chain_util) -> alignment (align_util) -> selection
(select_util) -> [insert-size statistics (isize_util) -> index.insert_size_options] -> pairing (pair_util) -> with rescue:
windows (window_util.plan); where one is planned, window MEMs (window_util.expected) and the four again on the union rows;
no window planned, so the first pass stands -> CIGARs (cigar_util) of the standing selection."""
import re
from collections import namedtuple

import numpy as np

import align_util as AU
import chain_util as CH
import cigar_util as CG
import contig_util as CU
import isize_util as IU
import mems_util as MM
import pair_util as PU
import sam_text_util as ST
import select_util as SU
import window_util as WU

ORIENT = {"fr": 1, "rf": 2, "same": 4, "any": 7}                     # _native.PAIR_ORIENT
RESCUE_MIN_LEN, RESCUE_MIN_ANCHOR = 12, 40                           # map_pairs' rescue_options defaults
SELECT_LANE_MAX, PAIR_LANE_MAX = SU.LANE_MAX, PU.LANE_MAX            # GENIE_SELECT_LANE_MAX, GENIE_PAIR_LANE_MAX
ALL_TAGS = ST.NM | ST.AS | ST.MD | ST.MC | ST.MQ


# ------------------------------------------------------------------ the composed host pipeline
class HostRun:
    """Every intermediate of one host run.  first / second: dicts of the stages of the first pass and of the pass over the
    union rows (None when no window was planned) with mems (offsets, rows, status, skipped), chains, aln, select, pair;
    stats, est: the insert-size statistics and the InsertSize used; windows, planned: window_util.plan's; window_mems:
    window_util.expected's four; cigars: cigar_util.expected's dict; result: what map_pairs returns."""


def _orient(v):
    return ORIENT[v] if isinstance(v, str) else int(v)


def _pair_params(popts):
    opts = dict(popts)
    if "orient" in opts:
        opts["orient"] = _orient(opts["orient"])
    return PU.DEFAULTS._replace(**opts)


def _reads_list(bases, read_offsets):
    return [np.asarray(bases[read_offsets[i]:read_offsets[i + 1]], np.uint8) for i in range(len(read_offsets) - 1)]


def _chain_batch(bases, read_offsets, S, offsets, rows, chains):
    return {"S": S, "bases": bases, "read_offsets": read_offsets, "offsets": offsets, "rows": rows, "anchor_chain": chains["anchor_chain"],
            "anchor_pred": chains["anchor_pred"], "chain_offsets": chains["offsets"], "chains": chains["chains"]}


def _four(T, table, bases, read_offsets, S, offsets, rows, cp, ap, sp, pp):
    """chain, align, select, pair over MEM rows -> the stage dict."""
    st = {}
    st["chains"] = CH.expected(offsets, rows, cp, table)
    st["batch"] = _chain_batch(bases, read_offsets, S, offsets, rows, st["chains"])
    st["aln"], st["aln_totals"], _ = AU.expected(st["batch"], ap, T, table)
    sb = {"read_offsets": read_offsets, "S": S, "chain_offsets": st["chains"]["offsets"], "chains": st["chains"]["chains"],
          "aln": st["aln"]}
    st["select_batch"] = sb
    st["select"] = SU.expected(sb, sp, table)
    st["pair_batch"] = {"sel_offsets": st["select"]["offsets"], "records": st["select"]["records"], "klass": st["select"]["klass"]}
    st["pair"] = PU.expected(st["pair_batch"], pp) if pp is not None else None
    return st


def host_pipeline(T, table, reads_csr, minimum_length, *, both_strands=True, split_breaks=False, max_occ=0, chain_options=None,
                  align_options=None, select_options=None, pair_options=None, rescue=False, rescue_options=None, insert_size=None):
    """SMEM.map_pairs on the CPU -> HostRun.  T: the reference's codes; table: the contig offsets int64[nc + 1] or None;
    reads_csr: (bases uint8, read_offsets int64[N + 1]), interleaved mates; the options as map_pairs takes them (chain_options
    a dict here).  insert_size: None, "estimate", a dict of insert_size_stats' options or an index.InsertSize."""
    from genie_smem_amd.index import InsertSize, insert_size_options
    T = np.asarray(T, np.uint8)
    bases, read_offsets = np.asarray(reads_csr[0], np.uint8), np.asarray(reads_csr[1], np.int64)
    table = None if table is None else np.asarray(table, np.int64)
    S = 2 if both_strands else 1
    flags = (MM.BOTH if both_strands else 0) | (MM.SPLIT if split_breaks else 0)
    reads = _reads_list(bases, read_offsets)
    cp = CH.DEFAULTS._replace(**(chain_options or {}))
    ap = AU.DEFAULTS._replace(**(align_options or {}))
    sp = SU.DEFAULTS._replace(**(select_options or {}))
    run = HostRun()
    run.S, run.align_params = S, ap
    if table is not None:
        mems = CU.expected(T, table, reads, flags, minimum_length, max_occ)
    else:
        mems = MM.expected(T, reads, flags, minimum_length, max_occ)
    first = _four(T, table, bases, read_offsets, S, mems[0], mems[1], cp, ap, sp, None)
    first["mems"] = mems
    popts, ropts, used = dict(pair_options or {}), dict(rescue_options or {}), ()
    run.stats = run.est = None
    if insert_size is not None:
        if isinstance(insert_size, InsertSize):
            est = insert_size
        elif insert_size == "estimate" or isinstance(insert_size, dict):
            ip = IU.DEFAULTS._replace(**(insert_size if isinstance(insert_size, dict) else {}))
            run.stats = IU.expected(first["pair_batch"], ip)
            est = insert_size_options(run.stats["stats"], popts)
        else:
            raise ValueError("insert_size")
        popts.update(orient=est.orient, isize_min=est.isize_min, isize_max=est.isize_max, isize_mean=est.isize_mean)
        run.est, used = est, (est,)
    pp = _pair_params(popts)
    run.pair_params = pp
    first["pair"] = PU.expected(first["pair_batch"], pp)
    run.first, run.second, run.windows, run.window_mems = first, None, None, None
    last, extra = first, ()
    if rescue:
        if not both_strands:
            raise ValueError("rescue needs both_strands")
        min_len, min_anchor = int(ropts.pop("min_len", RESCUE_MIN_LEN)), int(ropts.pop("min_anchor_score", RESCUE_MIN_ANCHOR))
        orient = _orient(ropts.pop("orient") if "orient" in ropts else popts.get("orient", "fr"))
        isize_max = int(ropts.pop("isize_max") if "isize_max" in ropts else popts.get("isize_max", 1000))
        if ropts:
            raise TypeError(f"unknown rescue option {sorted(ropts)[0]!r}")
        sel = first["select"]
        run.windows, run.planned = WU.plan(len(T), table, read_offsets, sel["offsets"], sel["records"], first["pair"]["pairs"], orient,
                                           isize_max, min_anchor)
        status, totals = np.zeros(run.windows.shape[0], np.int32), np.zeros(3, np.int64)
        if run.planned[0] > 0:
            run.window_mems = WU.expected(T, reads, S, run.windows, min_len, mems[0], mems[1])
            offsets, rows, status, totals = run.window_mems
            run.second = _four(T, table, bases, read_offsets, S, offsets, rows, cp, ap, sp, pp)
            run.second["mems"] = (offsets, rows)
            last = run.second
        extra = ((run.windows, status, totals),)
    run.last = last
    run.cigars = CG.expected(last["batch"], ap, T, last["aln"], table, last["select"]["sel"])
    run.result = (last["select"]["records"], last["select"]["offsets"], run.cigars["offsets"], run.cigars["cigar"], run.cigars["info"],
                  last["pair"]["pairs"], last["pair"]["sam"]) + extra + used
    return run


def host_map_pairs(T, table, reads_csr, minimum_length, **options):
    """What SMEM.map_pairs returns, as numpy arrays: (records, sel_offsets, cigar_offsets, cigar uint32, info, pairs, sam), then
    (windows, status, totals) with rescue, then the InsertSize with insert_size."""
    return host_pipeline(T, table, reads_csr, minimum_length, **options).result


def host_sam_text(result, T, table, reads_csr, names, contig_names, quals=None, tags=ST.NM | ST.AS, seq=True):
    """What SMEM.sam_text returns for a result of host_map_pairs (or of the device, as numpy arrays) -> (text uint8,
    line_offsets int64, totals int64[3]).  names, contig_names: lists of bytes; quals: uint8 parallel to the bases, or None."""
    b = {"bases": np.asarray(reads_csr[0], np.uint8), "read_offsets": np.asarray(reads_csr[1], np.int64),
         "quals": None if quals is None else np.asarray(quals, np.uint8), "sel_offsets": result[1], "records": result[0], "sam": result[6],
         "info": result[4], "cigar_offsets": result[2], "cigar": np.asarray(result[3]).astype(np.int64) & 0xFFFFFFFF,
         "names": [bytes(x) for x in names], "contig_names": [bytes(x) for x in contig_names],
         "contig_offsets": None if table is None else np.asarray(table, np.int64)}
    out = ST.expected(b, np.asarray(T, np.uint8), tags, 0 if seq else ST.NO_SEQ)
    return out["text"], out["line_offsets"], out["totals"]


# ------------------------------------------------------------------ the simulator
N_REF = 4096
TABLE = np.asarray([0, 3300, 3800, N_REF], np.int64)                 # contigs a (3300 bases), b (500), c (296)
CONTIG_NAMES = [b"a", b"b", b"c"]
DUP = ((400, 700), (2000, 2300))                                     # a[2000:2300] is an exact copy of a[400:700]
TANDEM_UNIT, TANDEM = 17, (1000, 1340)                               # a[1000:1340]: a 17-base unit, 20 times
REPEATS = DUP + (TANDEM,)
MIN_LEN = 19
EVERY = 13                                                           # a diverged mate: one substitution every 13 bases

Truth = namedtuple("Truth", "contig start end strand label recoverable rescuable")
# one row per mate: the template piece T[TABLE[contig] + start : TABLE[contig] + end) (contig -1: none), the strand the read
# is on, the scenario, whether the first pass must find it (recoverable) and whether it is a diverged mate that only rescue
# finds (rescuable: True inside a window, False when unreachable, None for any other mate)


class Batch:
    """bases, read_offsets (CSR codes, interleaved mates), names (one per read, the pair's), quals uint8 parallel to bases,
    truth (one Truth per read), options (what both sides pass to map_pairs)."""

    def reads(self):
        return _reads_list(self.bases, self.read_offsets)

    def strings(self):
        return ["".join("ACGTN"[c] for c in q) for q in self.reads()]

    def pairs_of(self, label):
        return sorted({r // 2 for r, t in enumerate(self.truth) if t.label == label})


def reference(seed=7):
    """-> T uint8[4096]: random bases, then the duplication and the tandem repeat planted in contig a."""
    rng = np.random.default_rng(seed)
    T = rng.integers(0, 4, N_REF).astype(np.uint8)
    T[DUP[1][0]:DUP[1][1]] = T[DUP[0][0]:DUP[0][1]]
    unit = rng.integers(0, 4, TANDEM_UNIT).astype(np.uint8)
    T[TANDEM[0]:TANDEM[1]] = np.resize(unit, TANDEM[1] - TANDEM[0])
    return T


def longest_run(kept):
    """The longest run of True."""
    best = run = 0
    for k in kept:
        run = run + 1 if k else 0
        best = max(best, run)
    return best


def mutate(rng, piece, subs=0.03, ins=0.01, dele=0.01):
    """A copy of the template with substitutions, insertions and deletions -> (read, the longest run of bases copied unchanged
    between two edits: an exact match of the template by construction)."""
    out, kept = [], []
    for c in np.asarray(piece, np.uint8).tolist():
        u = rng.random()
        if u < dele:
            kept.append(False)                                      # the base is gone: the run ends here
            continue
        if u < dele + ins:
            out += [int(rng.integers(0, 4)), c]                      # a base in front of this one: the run ends, the base stays
            kept += [False, True]
        elif u < dele + ins + subs:
            out.append((c + int(rng.integers(1, 4))) % 4)
            kept.append(False)
        else:
            out.append(c)
            kept.append(True)
    return np.asarray(out, np.uint8), longest_run(kept)


def diverge(piece):
    """A substitution at every 13th base: no exact run above 12 bases."""
    q = np.asarray(piece, np.uint8).copy()
    q[EVERY - 1::EVERY] = (q[EVERY - 1::EVERY] + 1) % 4
    return q


def in_repeat(contig, start, end):
    return contig == 0 and any(start < hi and lo < end for lo, hi in REPEATS)


def _finish(batch, reads, names, truth, rng):
    batch.read_offsets = np.zeros(len(reads) + 1, np.int64)
    batch.read_offsets[1:] = np.cumsum([len(q) for q in reads])
    batch.bases = np.concatenate([np.asarray(q, np.uint8) for q in reads] + [np.zeros(0, np.uint8)]).astype(np.uint8)
    batch.quals = rng.integers(35, 74, batch.bases.size).astype(np.uint8)
    batch.names, batch.truth = names, truth
    assert len(reads) == len(truth) == len(names) and len(reads) % 2 == 0
    return batch


def library(T, seed=11, pairs=48):
    """FR pairs of 100 to 150 base mates with inserts of 250 to 500, mate 0 forward in every other pair, 3 % substitutions and
    1 % each of insertions and deletions; every fifth second mate diverged instead (found by rescue alone)."""
    rng = np.random.default_rng(seed)
    reads, names, truth = [], [], []
    k = 0
    while k < pairs:
        ins = int(rng.integers(250, 501))
        room = np.maximum(np.diff(TABLE) - ins + 1, 0)               # the fragment's start, uniform over every place it fits
        at = int(rng.integers(0, room.sum()))
        c = int(np.searchsorted(np.cumsum(room), at, side="right"))
        f = at - int(np.cumsum(room)[c] - room[c])
        L = [int(rng.integers(100, 151)) for _ in range(2)]
        left, right = (f, f + L[0]), (f + ins - L[1], f + ins)
        if (in_repeat(c, *left) or in_repeat(c, *right)) and rng.random() < 0.9:
            continue                                                 # most fragments that touch a planted repeat are not kept
        swap = k % 2                                                 # mate 0 is the forward one in half of the pairs
        spans = [right, left] if swap else [left, right]
        strands = [1, 0] if swap else [0, 1]
        for m in (0, 1):
            lo, hi = spans[m]
            piece = T[TABLE[c] + lo:TABLE[c] + hi]
            diverged = m == 1 and k % 5 == 4
            if diverged:
                q, run = diverge(piece), EVERY - 1
            else:
                q, run = mutate(rng, piece)
            reads.append(AU.revcomp(q) if strands[m] else q)
            unique = not in_repeat(c, lo, hi)
            truth.append(Truth(c, lo, hi, strands[m], "diverged" if diverged else "library", unique and run >= MIN_LEN,
                               True if diverged else None))
            names.append(f"lib{k}".encode())
        k += 1
    b = Batch()
    b.options = dict(minimum_length=MIN_LEN, split_breaks=False, chain_options=dict(min_score=MIN_LEN))
    b.insert_range = (250, 500)
    return _finish(b, reads, names, truth, rng)


def hard(T, seed=23):
    """Every scenario at least twice, once with the affected mate on each strand.  The affected mate is mate 1 unless said."""
    rng = np.random.default_rng(seed)
    reads, names, truth = [], [], []
    rand = lambda n: rng.integers(0, 4, n).astype(np.uint8)      # noqa: E731

    def piece(c, lo, hi):
        return T[TABLE[c] + lo:TABLE[c] + hi].copy()

    def add(label, mates):
        """mates: two of (read as sequenced on the template's strand, strand, contig, start, end, recoverable, rescuable)."""
        for q, strand, c, lo, hi, rec, res in mates:
            reads.append(AU.revcomp(q) if strand else np.asarray(q, np.uint8))
            truth.append(Truth(c, lo, hi, strand, label, rec, res))
            names.append(f"{label}.{(len(reads) - 1) // 2}".encode())

    def exact(c, lo, hi, strand, rec=True):
        return (piece(c, lo, hi), strand, c, lo, hi, rec and not in_repeat(c, lo, hi), None)

    def fr(label, c, left, right, affected, lq=None, rq=None):
        """An FR pair on contig c: left = (lo, hi) forward, right = (lo, hi) reverse; the affected side ("left" or "right") is
        mate 1, so it is on strand 1 with "right" and on strand 0 with "left"; lq / rq replace the sequences."""
        lm = (piece(c, *left) if lq is None else lq, 0, c, left[0], left[1], not in_repeat(c, *left), None)
        rm = (piece(c, *right) if rq is None else rq, 1, c, right[0], right[1], not in_repeat(c, *right), None)
        add(label, [lm, rm] if affected == "right" else [rm, lm])

    # a mate inside the duplication with a unique partner: the copy at a[400:700] with a partner on either side
    fr("dup", 0, (150, 290), (520, 660), "right")
    fr("dup", 0, (450, 590), (760, 900), "left")
    # both mates inside the tandem repeat
    fr("tandem", 0, (1034, 1134), (1190, 1290), "right")
    fr("tandem", 0, (1040, 1140), (1200, 1300), "left")
    # a mate whose template runs off its contig's end into random bases: a's end (reverse mate), b's start (forward mate)
    fr("overhang", 0, (2900, 3040), (3190, 3300), "right", rq=np.concatenate([piece(0, 3190, 3300), rand(40)]))
    fr("overhang", 1, (0, 110), (250, 390), "left", lq=np.concatenate([rand(40), piece(1, 0, 110)]))
    # a mate whose template is the reference across the boundary of a and b, 60 bases of each: one record per contig at most
    across = T[TABLE[1] - 60:TABLE[1] + 60].copy()
    add("boundary", [exact(0, 2950, 3090, 0), (across, 1, 0, 3240, 3300, False, None)])
    add("boundary", [exact(1, 80, 220, 1), (across, 0, 0, 3240, 3300, False, None)])
    # a chimeric mate: 80 bases of a, then 70 of c (of b) -> a supplementary record
    fr("chimeric", 0, (2400, 2540), (2700, 2780), "right", rq=np.concatenate([piece(0, 2700, 2780), piece(2, 100, 170)]))
    fr("chimeric", 0, (1500, 1580), (1800, 1940), "left", lq=np.concatenate([piece(1, 300, 370), piece(0, 1500, 1580)]))
    # an 8-base deletion and an 8-base insertion
    fr("deletion", 0, (2350, 2490), (2600, 2748), "right", rq=np.concatenate([piece(0, 2600, 2670), piece(0, 2678, 2748)]))
    fr("deletion", 0, (1400, 1548), (1700, 1840), "left", lq=np.concatenate([piece(0, 1400, 1470), piece(0, 1478, 1548)]))
    fr("insertion", 0, (2800, 2940), (3050, 3190), "right", rq=np.concatenate([piece(0, 3050, 3120), rand(8), piece(0, 3120, 3190)]))
    fr("insertion", 0, (1350, 1490), (1600, 1740), "left", lq=np.concatenate([piece(0, 1350, 1420), rand(8), piece(0, 1420, 1490)]))
    # a run of N (code 4): split_breaks
    for flip, (left, right) in enumerate((((2500, 2640), (2760, 2900)), ((1560, 1700), (1820, 1960)))):
        q = piece(0, *(right if flip == 0 else left))
        q[60:70] = 4
        fr("n_run", 0, left, right, "right" if flip == 0 else "left", **({"rq": q} if flip == 0 else {"lq": q}))
    # an insert shorter than the read: both mates read 90 bases of template and then 30 of adapter
    for flip, f in enumerate((2310, 710)):
        lq, rq = np.concatenate([piece(0, f, f + 90), rand(30)]), np.concatenate([AU.revcomp(rand(30)), piece(0, f, f + 90)])
        fr("short_insert", 0, (f, f + 90), (f, f + 90), "right" if flip == 0 else "left", lq=lq, rq=rq)
    # two mates that start at the same position (the TLEN sign rule), the reverse one the longer
    fr("same_start", 0, (2420, 2520), (2420, 2550), "right")
    fr("same_start", 0, (800, 900), (800, 930), "left")
    # an RF pair: the left mate reverse, the right mate forward
    for flip, (left, right) in enumerate((((2330, 2450), (2650, 2770)), ((1360, 1480), (1660, 1780)))):
        lm, rm = exact(0, *left, 1), exact(0, *right, 0)
        add("rf", [lm, rm] if flip == 0 else [rm, lm])
    # a same-strand pair: both forward, both reverse
    add("same_strand", [exact(0, 2340, 2460, 0), exact(0, 2640, 2760, 0)])
    add("same_strand", [exact(0, 1380, 1500, 1), exact(0, 1680, 1800, 1)])
    # a pair on two contigs
    add("two_contigs", [exact(0, 3000, 3120, 0), exact(1, 100, 220, 1)])
    add("two_contigs", [exact(2, 50, 170, 1), exact(0, 100, 220, 0)])
    # a pair 3 kb apart on one contig
    add("far", [exact(0, 50, 170, 0), exact(0, 3150, 3270, 1)])
    add("far", [exact(0, 3160, 3280, 1), exact(0, 60, 180, 0)])
    # a random mate, two random mates
    add("random_mate", [exact(0, 2850, 2970, 0), (rand(120), 1, -1, 0, 0, False, None)])
    add("random_mate", [exact(1, 200, 320, 1), (rand(120), 0, -1, 0, 0, False, None)])
    add("random_both", [(rand(110), 0, -1, 0, 0, False, None), (rand(130), 1, -1, 0, 0, False, None)])
    add("random_both", [(rand(130), 1, -1, 0, 0, False, None), (rand(110), 0, -1, 0, 0, False, None)])
    # a mate shorter than minimum_length, a mate of length 0
    add("short_mate", [exact(0, 2560, 2680, 0), (piece(0, 2800, 2800 + MIN_LEN - 1), 1, 0, 2800, 2800 + MIN_LEN - 1, False, None)])
    add("short_mate", [exact(0, 1900, 1990, 1), (piece(0, 1700, 1700 + MIN_LEN - 1), 0, 0, 1700, 1700 + MIN_LEN - 1, False, None)])
    add("empty_mate", [exact(0, 2570, 2690, 0), (rand(0), 1, -1, 0, 0, False, None)])
    add("empty_mate", [(rand(0), 0, -1, 0, 0, False, None), exact(0, 1450, 1570, 1)])
    # diverged mates: two that rescue reaches, then one whose only copy lies outside the window and one across the boundary
    add("diverged", [exact(0, 2320, 2440, 0), (diverge(piece(0, 2600, 2750)), 1, 0, 2600, 2750, False, True)])
    add("diverged", [exact(0, 1850, 1970, 1), (diverge(piece(0, 1500, 1650)), 0, 0, 1500, 1650, False, True)])
    add("unreachable", [exact(0, 100, 220, 0), (diverge(piece(0, 1400, 1550)), 1, 0, 1400, 1550, False, False)])
    add("unreachable", [exact(0, 3100, 3220, 1), (diverge(piece(0, 1800, 1950)), 0, 0, 1800, 1950, False, False)])
    add("unreachable", [exact(0, 3150, 3290, 0), (diverge(piece(1, 60, 210)), 1, 1, 60, 210, False, False)])
    add("unreachable", [exact(1, 20, 160, 1), (diverge(piece(0, 3100, 3250)), 0, 0, 3100, 3250, False, False)])
    b = Batch()
    b.options = dict(minimum_length=MIN_LEN, split_breaks=True, chain_options=dict(min_score=MIN_LEN),
                     select_options=dict(max_secondary=12))          # 13 x 13 record combinations for a pair inside the tandem repeat
    return _finish(b, reads, names, truth, rng)


# ------------------------------------------------------------------ the SAM checker: its own parser, none of the brute forces
TAG_NM, TAG_AS, TAG_MD, TAG_MC, TAG_MQ = 1, 2, 4, 8, 16
_CIGAR = re.compile(rb"(\d+)([IDS=X])")
_MD = re.compile(rb"(\d+)|\^([ACGT]+)|([ACGT])")
_LETTERS = b"ACGTN"
_TURN = bytes.maketrans(b"ACGTN", b"TGCAN")


class SamLine:
    """One parsed line: the eleven columns and the tags as a dict of bytes."""

    def __init__(self, number, raw):
        assert raw.endswith(b"\n") and raw.count(b"\n") == 1, (number, "a line ends with its only newline")
        cols = raw[:-1].split(b"\t")
        assert len(cols) >= 11, (number, "eleven columns")
        self.number, self.name, self.flag, self.rname = number, cols[0], int(cols[1]), cols[2]
        self.pos, self.mapq = int(cols[3]), int(cols[4])
        self.cigar, self.rnext, self.pnext, self.tlen, self.seq, self.qual = cols[5], cols[6], int(cols[7]), int(cols[8]), cols[9], cols[10]
        self.tags = {}
        for c in cols[11:]:
            key, kind, value = c.split(b":", 2)
            assert key not in self.tags and (kind == b"i") == (key in (b"NM", b"AS", b"MQ")) and kind in (b"i", b"Z"), (number, c)
            self.tags[key] = value
        self.order = [c[:2] for c in cols[11:]]
        self.ops = [(int(n), op) for n, op in _CIGAR.findall(self.cigar)] if self.cigar != b"*" else []
        assert self.cigar == b"*" or b"".join(b"%d%s" % o for o in self.ops) == self.cigar, (number, "CIGAR syntax", self.cigar)
        self.mapped = not self.flag & 4
        self.mine = not self.flag & 0x900

    def count(self, letters):
        return sum(n for n, op in self.ops if op in letters)


def _need(ok, line, what, *more):
    if not ok:
        raise AssertionError((f"line {line.number}", what, line.name, line.flag, line.rname, line.pos, line.cigar) + more)


def _check_mapped(ln, r, T, table, cnames, reads, p, tags, seq, quals):
    read = bytes(_LETTERS[min(int(c), 4)] for c in reads[r])
    turned = bool(ln.flag & 0x10)
    q = read.translate(_TURN)[::-1] if turned else read
    _need(ln.ops and all(n > 0 for n, _ in ln.ops), ln, "a mapped line has ops of positive length")
    _need(all(op != b"S" or k in (0, len(ln.ops) - 1) for k, (_, op) in enumerate(ln.ops)), ln, "S only at the ends")
    _need(ln.count(b"IS=X") == len(read), ln, "I, S, = and X add up to the SEQ length", len(read))
    if seq:
        _need(ln.seq == q, ln, "SEQ is the read on the strand of 0x10")
        if quals is not None:
            _need(ln.qual == (quals[r][::-1] if turned else quals[r]), ln, "QUAL follows SEQ")
        else:
            _need(ln.qual == b"*", ln, "QUAL")
    else:
        _need(ln.seq == b"*" and ln.qual == b"*", ln, "no SEQ, no QUAL")
    _need(ln.rname in cnames, ln, "RNAME is a contig")
    c = cnames.index(ln.rname)
    clo, chi = (0, len(T)) if table is None else (int(table[c]), int(table[c + 1]))
    span = ln.count(b"D=X")
    _need(ln.pos >= 1 and ln.pos - 1 + span <= chi - clo, ln, "the alignment lies inside its contig", chi - clo)
    ref = bytes(_LETTERS[int(v)] for v in T[clo + ln.pos - 1:clo + ln.pos - 1 + span])
    _need(0 <= ln.mapq <= 60, ln, "MAPQ in [0, 60]")
    _need(not (ln.flag & 0x100 and ln.flag & 0x800), ln, "0x100 and 0x800 never both")
    want = [k for k, bit in ((b"NM", TAG_NM), (b"AS", TAG_AS), (b"MD", TAG_MD)) if tags & bit]
    _need([k for k in ln.order if k in (b"NM", b"AS", b"MD")] == want, ln, "NM, AS and MD as asked for, in this order", ln.order)
    # the walk: SEQ, CIGAR and MD rebuild the reference.  MD becomes one entry per reference base the alignment covers
    entries = None
    if tags & TAG_MD:
        toks = [(int(n) if n else None, d, s) for n, d, s in _MD.findall(ln.tags[b"MD"])]
        _need(b"".join(b"%d" % n if n is not None else (b"^" + d if d else s) for n, d, s in toks) == ln.tags[b"MD"], ln, "MD syntax")
        _need(len(toks) % 2 == 1 and all((tok[0] is not None) == (k % 2 == 0) for k, tok in enumerate(toks)), ln,
              "MD is count, item, count, ..., count", ln.tags[b"MD"])
        entries = []
        for k, (n, d, s) in enumerate(toks):
            entries += [("=", None, k)] * n if n is not None else [("D", bytes([v]), k, len(d)) for v in d] if d else [("X", s, k)]
        _need(len(entries) == span, ln, "MD covers as many reference bases as the CIGAR", len(entries), span)
    built, at, t, score = [], 0, 0, 0
    for n, op in ln.ops:
        if op == b"S":
            at += n
        elif op == b"I":
            at, score = at + n, score - p.gap_open - p.gap_extend * n
        elif op == b"=":
            _need(q[at:at + n] == ref[t:t + n] and b"N" not in q[at:at + n], ln, "= bases equal the reference", at, t)
            _need(entries is None or all(e[0] == "=" for e in entries[t:t + n]), ln, "MD counts where the CIGAR has =", t)
            built.append(q[at:at + n])
            at, t, score = at + n, t + n, score + p.match * n
        elif op == b"X":
            _need(len(ref[t:t + n]) == n and all(q[at + i] != ref[t + i] or q[at + i] == 78 for i in range(n)), ln, "X bases differ", at, t)
            _need(entries is None or all(e[0] == "X" for e in entries[t:t + n]), ln, "MD has a letter where the CIGAR has X", t)
            built.append(ref[t:t + n] if entries is None else b"".join(e[1] for e in entries[t:t + n]))
            at, t, score = at + n, t + n, score - p.mismatch * n
        else:
            _need(op == b"D", ln, "an op of I, D, S, = or X")
            _need(entries is None or all(e[0] == "D" and e[2] == entries[t][2] and e[3] == n for e in entries[t:t + n]), ln,
                  "MD has ^ and as many letters where the CIGAR has D", t)
            built.append(ref[t:t + n] if entries is None else b"".join(e[1] for e in entries[t:t + n]))
            t, score = t + n, score - p.gap_open - p.gap_extend * n
    _need(b"".join(built) == ref and t == span and at == len(read), ln, "SEQ, CIGAR and MD rebuild the reference", b"".join(built), ref)
    if tags & TAG_NM:
        _need(int(ln.tags[b"NM"]) == ln.count(b"XID"), ln, "NM is the sum of X, I and D", ln.tags[b"NM"])
    if tags & TAG_AS:
        score += p.end_bonus * ((ln.ops[0][1] != b"S") + (ln.ops[-1][1] != b"S"))
        _need(int(ln.tags[b"AS"]) == score, ln, "AS is the score of the CIGAR", ln.tags[b"AS"], score)
    return c, ln.pos - 1, ln.pos - 1 + span


def check_sam(text, line_offsets, T, table, contig_names, reads, names, align_params, tags=TAG_NM | TAG_AS | TAG_MD | TAG_MC | TAG_MQ,
              seq=True, quals=None):
    """The SAM text of a paired batch against the reads, the reference and the scoring alone -> the number of lines checked.
    text: bytes or uint8; line_offsets: one entry more than there are lines; T: the reference's codes; table: the contig
    offsets or None; contig_names, names: lists of bytes or str, one name per contig and per read (the names of two pairs in
    a row differ); reads: the code arrays in read orientation; align_params: match, mismatch, gap_open, gap_extend, end_bonus;
    tags: the mask the text was written with; quals: per read bytes, or None.  Raises AssertionError naming the line."""
    raw = bytes(np.asarray(text, np.uint8)) if not isinstance(text, (bytes, bytearray)) else bytes(text)
    lo = [int(v) for v in line_offsets]
    enc = lambda x: x.encode() if isinstance(x, str) else bytes(x)      # noqa: E731
    cnames, names = [enc(x) for x in contig_names], [enc(x) for x in names]
    quals = None if quals is None else [enc(x) for x in quals]
    assert lo[0] == 0 and lo[-1] == len(raw) and all(a < b for a, b in zip(lo, lo[1:])), "the line offsets cover the text"
    lines = [SamLine(k, raw[a:b]) for k, (a, b) in enumerate(zip(lo, lo[1:]))]
    N = len(reads)
    assert N % 2 == 0 and len(names) == N
    # lines to reads: in read order, a read's lines share its name and its parity bit
    by_read, r = [[] for _ in range(N)], 0
    for ln in lines:
        _need(ln.flag & 1 and bool(ln.flag & 0x40) != bool(ln.flag & 0x80), ln, "paired, and exactly one of 0x40 and 0x80")
        parity = 1 if ln.flag & 0x80 else 0
        while r < N and (by_read[r] and (names[r] != ln.name or parity != r % 2)):
            r += 1
        _need(r < N and names[r] == ln.name and parity == r % 2, ln, "QNAME is the pair's name and 0x40 / 0x80 the read's parity", r)
        by_read[r].append(ln)
    assert all(by_read), ("a read without a line", [i for i in range(N) if not by_read[i]][:4])
    place = {}
    for r in range(N):
        mapped = [ln for ln in by_read[r] if ln.mapped]
        for ln in mapped:
            place[ln.number] = _check_mapped(ln, r, T, table, cnames, reads, align_params, tags, seq, quals)
        if mapped:
            _need(len(mapped) == len(by_read[r]), by_read[r][0], "a mapped read has no unmapped line")
            _need(sum(ln.mine for ln in mapped) == 1, mapped[0], "exactly one line with neither 0x100 nor 0x800")
        else:
            _need(len(by_read[r]) == 1, by_read[r][0], "an unmapped read has one line")
    for k in range(N // 2):
        mine = [next((ln for ln in by_read[2 * k + m] if ln.mapped and ln.mine), None) for m in (0, 1)]
        for m in (0, 1):
            other = mine[1 - m]
            for ln in by_read[2 * k + m]:
                _need(bool(ln.flag & 8) == (other is None), ln, "0x8 is the other mate's 0x4")
                _need(bool(ln.flag & 0x20) == bool(other is not None and other.flag & 0x10), ln, "0x20 is the other mate's 0x10")
                if other is not None:
                    _need(bool(ln.flag & 2) == bool(other.flag & 2), ln, "the proper bit is the same on both mates")
                    has_mc, has_mq = bool(tags & TAG_MC), bool(tags & TAG_MQ)
                    _need((ln.tags.get(b"MC") == other.cigar) if has_mc else b"MC" not in ln.tags, ln, "MC is the other mate's CIGAR")
                    _need((int(ln.tags.get(b"MQ", -1)) == other.mapq) if has_mq else b"MQ" not in ln.tags, ln,
                          "MQ is the other mate's MAPQ")
                else:
                    _need(not ln.flag & 2 and b"MC" not in ln.tags and b"MQ" not in ln.tags, ln, "no proper bit, MC or MQ without a mate")
                if ln.mapped:
                    if other is None:
                        _need(ln.rnext == b"*" and ln.pnext == 0 and ln.tlen == 0, ln, "RNEXT, PNEXT and TLEN without a mapped mate")
                        continue
                    named = ln.rname if ln.rnext == b"=" else ln.rnext
                    _need(named == other.rname and (ln.rnext == b"=") == (ln.rname == other.rname), ln, "RNEXT names the other mate's RNAME")
                    _need(ln.pnext == other.pos, ln, "PNEXT is the other mate's POS", other.pos)
                    (c0, b0, e0), (c1, b1, e1) = place[ln.number], place[other.number]
                    if c0 != c1:
                        _need(ln.tlen == 0, ln, "TLEN is 0 across contigs")
                    else:
                        first = b0 < b1 or (b0 == b1 and m == 0)
                        span = max(e0, e1) - min(b0, b1)
                        _need(ln.tlen == (span if first else -span), ln, "TLEN spans both mates, positive on the leftmost", span)
                    if ln.mine:
                        _need(ln.tlen == -other.tlen, ln, "TLEN is the negation of the other mate's", other.tlen)
                else:
                    _need(ln.flag & 4 and ln.mapq == 0 and ln.cigar == b"*" and ln.tlen == 0, ln,
                          "an unmapped line: 0x4, MAPQ 0, no CIGAR, TLEN 0")
                    _need(not {b"NM", b"AS", b"MD"} & set(ln.tags), ln, "an unmapped line carries no NM, AS or MD")
                    read = bytes(_LETTERS[min(int(c), 4)] for c in reads[2 * k + m])
                    _need(ln.seq == (read if seq else b"*"), ln, "an unmapped line has SEQ in read orientation")
                    if other is None:
                        _need((ln.rname, ln.pos, ln.rnext, ln.pnext) == (b"*", 0, b"*", 0), ln, "without a mapped mate: * and 0")
                    else:
                        _need((ln.rname, ln.pos, ln.rnext, ln.pnext) == (other.rname, other.pos, b"=", other.pos), ln,
                              "placed at its mapped mate")
    return len(lines)


# ------------------------------------------------------------------ what the host and the GPU tests share, computed once
OPTION_SETS = {"plain": dict(rescue=False), "rescue": dict(rescue=True), "estimate": dict(rescue=True, insert_size="estimate"),
               # every orientation allowed, a narrower pairing window than rescue's, a stricter anchor and a longer window seed
               "any": dict(rescue=True, pair_options=dict(orient="any", isize_max=700, isize_mean=350, pen_unpaired=30),
                           rescue_options=dict(isize_max=900, min_anchor_score=100, min_len=11))}
_MADE = {}


def made(key, make):
    if key not in _MADE:
        _MADE[key] = make()
    return _MADE[key]


def batch(name):
    """"library" or "hard" on reference() -> (T, Batch), made once."""
    T = made("T", reference)
    return T, made(name, lambda: {"library": library, "hard": hard}[name](T))


def map_options(b, option_set):
    """The keyword options of host_pipeline for a batch and an option set; SMEM.map_pairs takes chain_options flat."""
    opts = {k: v for k, v in b.options.items() if k != "minimum_length"}
    opts.update(OPTION_SETS[option_set])
    return opts


def host_run(name, option_set, table=True):
    """The HostRun of a batch under an option set, with or without the contig table, computed once and not to be changed."""
    T, b = batch(name)
    return made((name, option_set, table), lambda: host_pipeline(T, TABLE if table else None, (b.bases, b.read_offsets),
                                                                 b.options["minimum_length"], **map_options(b, option_set)))
