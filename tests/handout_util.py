"""Large batches of hard reads for the tests of the persistent kernels (test_group_handout_gpu.py), and their expected
results without a brute-force run per batch element: a batch is an ORDER over a small POOL of distinct reads -- every read
of smem_util.batches(name) of one length class -- so the brute force of tests/smem_util.py runs once per pool read and
the batch's (offsets, rows, status) are gathered from those with np.repeat.  Plain Python and NumPy; nothing here comes
from the library under test (packing.reverse_complement is a layout conversion, pinned by test_both_strands_host.py).
test_group_handout_host.py pins the gather against smem_util.expected_batch on the explicit list of reads."""
import functools

import numpy as np

import lookup_util as U
import smem_util as S

READ_OVERFLOW = 4                   # GENIE_READ_OVERFLOW (slot form: more rows than the slot capacity)
JUNK = 9                            # the byte behind every read of a pool matrix
RUN_LENGTHS = (1, 7, 64, 300)
RUN_KINDS = ("slow", "flagged", "empty", "one", "longest", "random")
TAIL_READS = 37
ORDERS = ("shuffled", "runs", "long_then_short", "tail")


@functools.lru_cache(maxsize=None)
def pool(name, kind):
    """(reads, matrix uint8 [n, longest + 3] with JUNK behind every read, lens int32 [n]) of one reference.  "short": every
    read of smem_util.batches(name)["short"] (1 .. 17, 31, 32, 33, 64, 150 and 255 bases) and one empty read; "mid": every
    read of ["mid"] (256, 705 and 1409 bases)."""
    assert kind in ("short", "mid")
    reads = [r for group in S.batches(name)[kind].values() for r in group]
    if kind == "short":
        reads.append(np.zeros(0, np.uint8))
    mat, lens = U.pack_rows(reads, max(len(r) for r in reads) + 3, JUNK)
    return reads, mat, lens


def flagged(read):
    """The read holds a code > 3 (GENIE_READ_BAD_BASE; the 2-bit packing cannot carry it)."""
    return bool(len(read)) and int(np.max(read)) > 3


def _period(read):
    """The smallest u <= 7 with read[u:] == read[:-u]; 0 if there is none (or the read is shorter than 16 bases)."""
    if len(read) >= 16:
        for u in range(1, 8):
            if np.array_equal(read[u:], read[:-u]):
                return u
    return 0


def kinds(reads):
    """Pool index of the read every run kind of orders()["runs"] repeats ("random" has none; a kind the pool lacks is left
    out).  "slow": the longest slow path -- among the longest reads the one that repeats a unit of at most 7 bases, the
    longest unit there is and the last such read (the tandem reference's unit tile; one base repeated elsewhere).  "flagged": the longest read with
    a code > 3.  "empty".  "one": the first of the shortest reads that are not empty.  "longest": the first of the longest
    reads that is neither of the above."""
    lens = np.asarray([len(r) for r in reads])
    top = int(lens.max())
    bad = np.asarray([flagged(r) for r in reads])
    per = np.asarray([_period(r) if len(r) == top and not flagged(r) else 0 for r in reads])
    assert per.max() > 0
    out = {"slow": int(np.flatnonzero(per == per.max())[-1])}
    if bad.any():
        out["flagged"] = int(np.flatnonzero(bad & (lens == lens[bad].max()))[0])
    if (lens == 0).any():
        out["empty"] = int(np.flatnonzero(lens == 0)[0])
    low = int(lens[lens > 0].min())
    out["one"] = int(np.flatnonzero((lens == low) & ~bad)[0])
    out["longest"] = int(np.flatnonzero((lens == top) & ~bad & (per == 0))[0])
    return out


def orders(reads, N, seed):
    """name -> pick (int64 [N], indexes into `reads`): the batch is [reads[i] for i in pick].  N is odd, so that it is no
    multiple of a group, a tile or a block.
    "shuffled": uniform random.
    "runs": runs of ONE read repeated.  The kind of read cycles through RUN_KINDS (kinds(); "random" draws a read per
        run); the run lengths cycle through RUN_LENGTHS, starting one further with every cycle of the kinds, so that every
        kind meets every run length: a wave's consecutive groups are all hard, then all flagged, then all empty or tiny.
    "long_then_short": the pool by descending length interleaved with the pool by ascending length -- a long read directly
        followed by a short one -- the ascending side moved on by one read with every repetition, so that in the end every
        read has followed every other read.
    "tail": "shuffled" with the last TAIL_READS reads replaced by one flagged read, one empty read (the shortest, where
        the pool has no such read) and TAIL_READS - 2 of the longest reads: the partial last group, the last claims of the
        hand-out."""
    assert N % 2 == 1 and N > 4 * TAIL_READS
    n = len(reads)
    rng = np.random.default_rng(seed)
    out = {"shuffled": rng.integers(0, n, N)}
    kind = kinds(reads)
    names = [k for k in RUN_KINDS if k == "random" or k in kind]
    others = np.setdiff1d(np.arange(n), list(kind.values()))      # a "random" run never lengthens its neighbours
    runs, total, i = [], 0, 0
    while total < N:
        k, cycle = names[i % len(names)], i // len(names)
        length = RUN_LENGTHS[(i % len(names) + cycle) % len(RUN_LENGTHS)]
        runs.append(np.full(length, kind[k] if k != "random" else int(others[rng.integers(0, len(others))]), np.int64))
        total += length
        i += 1
    out["runs"] = np.concatenate(runs)[:N]
    lens = np.asarray([len(r) for r in reads])
    down, up = np.argsort(-lens, kind="stable"), np.argsort(lens, kind="stable")
    reps = -(-N // (2 * n))
    pairs = np.empty((reps, n, 2), np.int64)
    pairs[:, :, 0] = down[None, :]
    pairs[:, :, 1] = up[(np.arange(n)[None, :] + np.arange(reps)[:, None]) % n]
    out["long_then_short"] = pairs.reshape(-1)[:N]
    tail = rng.integers(0, n, N)
    tail[N - TAIL_READS:] = kind["longest"]
    tail[N - TAIL_READS] = kind.get("flagged", kind["one"])
    tail[N - TAIL_READS + 1] = kind.get("empty", kind["one"])
    out["tail"] = tail
    assert set(out) == set(ORDERS) and all(p.shape == (N,) and p.dtype == np.int64 for p in out.values())
    return out


# ------------------------------------------------------------------ expectations
def per_read(name, reads, mode, min_len=1, K=0, split=False):
    """[(status, rows)] of every read: smem_util.expected / expected_split, one brute-force run per read."""
    ref = U.family()[name]
    return [S.expected_split(ref, r, min_len) if split else S.expected(ref, r, mode, min_len, K) for r in reads]


def both_strands(reads):
    """[r0, rc(r0), r1, rc(r1), ...]: the strand-reads of genie_find_smems_both."""
    from genie_smem_amd import packing
    return [x for r in reads for x in (r, packing.reverse_complement(r))]


def both_pick(pick):
    """The order over both_strands(reads) of the strand-reads of the batch `pick`: 2i, 2i + 1 for every i of pick."""
    pick = np.asarray(pick, np.int64)
    return np.stack([2 * pick, 2 * pick + 1], axis=1).reshape(-1)


def _table(per):
    """The expectations of the pool as one CSR: (first row of every read int64 [n + 1], rows int32 [S, 4], status int32 [n])."""
    first = np.zeros(len(per) + 1, np.int64)
    first[1:] = np.cumsum([len(rows) for _, rows in per])
    rows = np.concatenate([S.NO_ROWS] + [np.asarray(rows, np.int32).reshape(-1, 4) for _, rows in per])
    return first, rows, np.asarray([st for st, _ in per], np.int32)


def gather_index(per, pick):
    """(offsets int64 [N + 1], src int64 [S], status int32 [N]) of the batch [reads[i] for i in pick]: row j of the batch is
    row src[j] of the pool's rows, _table(per)[1]."""
    first, _, status = _table(per)
    pick = np.asarray(pick, np.int64)
    counts = (first[1:] - first[:-1])[pick]
    offsets = np.zeros(len(pick) + 1, np.int64)
    np.cumsum(counts, out=offsets[1:])
    # row j of batch element b is pool row first[pick[b]] + (j - offsets[b])
    src = np.repeat(first[pick] - offsets[:-1], counts) + np.arange(int(offsets[-1]), dtype=np.int64)
    return offsets, src, status[pick]


def gather_expected(per, pick):
    """(offsets int64 [N + 1], rows int32 [S, 4], status int32 [N]) of the batch [reads[i] for i in pick], `per` being the
    (status, rows) of every pool read."""
    offsets, src, status = gather_index(per, pick)
    return offsets, _table(per)[1][src], status


def count_rows(per, pick):
    """The number of rows of the batch."""
    return int(np.asarray([len(rows) for _, rows in per], np.int64)[np.asarray(pick, np.int64)].sum())


def gather_slots(per, pick, cap):
    """The slot form (genie_find_smems): (counts int32 [N], slots int32 [N, cap, 4], filled bool [N, cap], status int32 [N]).
    counts holds every row the read has; only the first min(count, cap) slots are filled (`filled`; the others are not
    part of the result, zero here), and a read with more rows than `cap` has status READ_OVERFLOW."""
    first, rows, status = _table(per)
    n = len(per)
    counts = (first[1:] - first[:-1]).astype(np.int32)
    slots = np.zeros((n, cap, 4), np.int32)
    for i in range(n):
        k = min(int(counts[i]), cap)
        slots[i, :k] = rows[first[i]:first[i] + k]
    status = np.where(counts > cap, READ_OVERFLOW, status).astype(np.int32)
    pick = np.asarray(pick, np.int64)
    filled = np.arange(cap)[None, :] < np.minimum(counts, cap)[pick][:, None]
    return counts[pick], slots[pick], filled, status[pick]
