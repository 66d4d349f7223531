"""The brute force of genie_insert_size_stats (include/genie_smem.h) in plain Python -- collect the samples, sort them, apply
the formulas -- with the raw ctypes call, the call on the guarded buffers of tests/guarded.py, and a generator of record batches
with a planted (type, span, mapq) per pair.  The record, the combination type and the span are pair_util's: the definition
says "exactly as genie_pair_alignments defines it".

A batch is a dict: sel_offsets int64[N+1] (N even: reads 2k and 2k + 1 are mates) and records int32[T, 12], as
genie_select_alignments writes them."""
import ctypes as C
from collections import namedtuple

import numpy as np

from pair_util import FR, NO_TYPE, RF, SAME, Rec, clamp, combo_type, span

Params = namedtuple("IsizeParams", "min_mapq max_span min_samples")
DEFAULTS = Params(20, 10000, 25)                         # GenieIndex.insert_size_stats' defaults
LDS_BINS, WINDOW_MAX = 4096, 65536                       # GENIE_ISIZE_LDS_BINS, GENIE_WINDOW_MAX
OUTLIER_IQR, WINDOW_IQR, WINDOW_STD = 2, 3, 4            # GENIE_ISIZE_OUTLIER_IQR, GENIE_ISIZE_WINDOW_IQR, GENIE_ISIZE_WINDOW_STD
INVALID, NO_DEVICE, CAPACITY, TOO_LONG = -1, -4, -10, -6
COLS = "n ok q25 q50 q75 lo_b hi_b n_in mean std isize_min isize_max".split()


def type_row(v, p, n_most):
    """The 12 columns of one type from its samples v (any order)."""
    v = sorted(v)
    n = len(v)
    row = [n] + [0] * 11
    if n == 0:
        return row
    q25, q50, q75 = v[min(n - 1, (n + 1) // 4)], v[n // 2], v[min(n - 1, (3 * n + 1) // 4)]
    row[2:5] = [q25, q50, q75]
    if n < p.min_samples or 20 * n < n_most:
        return row
    iqr = q75 - q25
    lo_b, hi_b = max(1, q25 - OUTLIER_IQR * iqr), q75 + OUTLIER_IQR * iqr
    inside = [s for s in v if lo_b <= s <= hi_b]
    n_in, S = len(inside), sum(inside)
    mean = (2 * S + n_in) // (2 * n_in)
    SS = sum((s - mean) ** 2 for s in inside)
    std = 0
    while std * std * n_in < SS:
        std += 1
    lo = max(0, min(q25 - WINDOW_IQR * iqr, mean - WINDOW_STD * std))
    hi = min(p.max_span, max(q75 + WINDOW_IQR * iqr, mean + WINDOW_STD * std))
    return [n, 1, q25, q50, q75, lo_b, hi_b, n_in, mean, std, lo, hi]


def stats_of(samples, p):
    """samples: (t, s) of the pairs that have one -> int64[3, 12]."""
    per = [[s for t, s in samples if t == u] for u in range(3)]
    n_most = max(len(v) for v in per)
    return np.asarray([type_row(per[u], p, n_most) for u in range(3)], np.int64)


def expected(b, p, n_records=None):
    """Every output of the call: {"stats": int64[3, 12], "samples": int32[P, 2], "totals": int64[4]}."""
    so, rec = b["sel_offsets"], b["records"]
    N = so.size - 1
    assert N % 2 == 0
    n_records = rec.shape[0] if n_records is None else n_records
    R = clamp(int(so[N]), 0, n_records)
    samples = np.zeros((N // 2, 2), np.int32)
    totals = np.zeros(4, np.int64)
    for k in range(N // 2):
        heads = []
        for r in (2 * k, 2 * k + 1):
            lo = clamp(int(so[r]), 0, R)
            if clamp(int(so[r + 1]), lo, R) > lo:
                heads.append(Rec(lo, rec[lo]))
        samples[k] = (-1, 0)
        if len(heads) < 2:
            continue
        totals[0] += 1
        x, y = heads
        t = combo_type(x, y)
        if t is None or t == NO_TYPE or not 1 <= span(x, y) <= p.max_span:
            totals[3] += 1
        elif x.q < p.min_mapq or y.q < p.min_mapq:
            totals[2] += 1
        else:
            totals[1] += 1
            samples[k] = (t, span(x, y))
    return {"stats": stats_of([tuple(r) for r in samples.tolist() if r[0] >= 0], p), "samples": samples, "totals": totals}


def agrees(got, want):
    for k in ("stats", "samples", "totals"):
        if k in got:
            assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (k, got[k].shape, want[k].shape, got[k].dtype)
            bad = np.argwhere(got[k] != want[k])
            assert bad.size == 0, (k, bad[:4].tolist(), got[k][bad[0][0]].tolist(), want[k][bad[0][0]].tolist())


# ------------------------------------------------------------------ batches
def planted_pair(t, s, mapq=60, length=100, contig=0, at=1000, mapq1=None):
    """The two heads (strand, contig, offset, r_span, mapq) of a pair of type t and span s; mate 0 first.  t: FR, RF, SAME,
    NO_TYPE (mate 1 strictly inside mate 0; s is then mate 0's length), "contigs" (two contigs), or None: no sample is meant and
    s is ignored (both mates far apart on one contig, FR).  A span shorter than the mates shortens them."""
    mapq1 = mapq if mapq1 is None else mapq1
    if t == NO_TYPE:
        return (0, contig, at + 1, s, mapq), (1, contig, at + 2, max(s - 2, 0), mapq1)
    if t == "contigs":
        return (0, contig, at + 1, length, mapq), (1, contig + 1, at + 1 + s - length, length, mapq1)
    ln = min(length, s)
    left, right = (0, contig, at + 1, ln, mapq), (1, contig, at + 1 + s - ln, ln, mapq1)
    if t == FR:
        return left, right
    if t == RF:                                                      # the reverse record on the left; mates that coincide would be FR
        ln = min(length, max(s - 1, 0))
        return (1, contig, at + 1, ln, mapq), (0, contig, at + 1 + s - ln, ln, mapq1)
    return (0, contig, at + 1, ln, mapq), (0, contig, at + 1 + s - ln, ln, mapq1)


def make_batch(pairs, extra=0):
    """pairs: per pair (head0, head1), a head being (strand, contig, offset, r_span, mapq) or None for a mate without records.
    Every mate with a head gets `extra` more records behind it (secondaries elsewhere, which no sample may use)."""
    rows, so = [], [0]
    for k, heads in enumerate(pairs):
        for m, h in enumerate(heads):
            if h is not None:
                strand, contig, offset, r_span, mapq = h
                rows.append((2 * k + m, 3 * len(rows) + 1, 0, strand, contig, offset, r_span, 0, max(r_span, 0), 50, 0, mapq))
                for _ in range(extra):
                    rows.append((2 * k + m, 3 * len(rows) + 1, 2, 1 - strand, contig, offset + 777, r_span, 0, max(r_span, 0), 40, 0, 0))
            so.append(len(rows))
    rec = np.asarray(rows, np.int64).reshape(-1, 12)
    return {"sel_offsets": np.asarray(so, np.int64), "records": np.clip(rec, -2**31, 2**31 - 1).astype(np.int32)}


def batch_of(plan, extra=0):
    """plan: per pair (t, s) or (t, s, mapq) or (t, s, mapq, mapq1) as planted_pair takes them, "none" (no mate has records),
    "left" / "right" (only that mate has)."""
    pairs = []
    for k, item in enumerate(plan):
        if item == "none":
            pairs.append((None, None))
        elif item in ("left", "right"):
            h = planted_pair(FR, 300, at=1000 + 10 * k)[0]
            pairs.append((h, None) if item == "left" else (None, h))
        else:
            pairs.append(planted_pair(*item[:2], *(item[2:3] or (60,)), at=1000 + 10 * (k % 5000), mapq1=item[3] if len(item) > 3 else None))
    return make_batch(pairs, extra)


# ------------------------------------------------------------------ the call
def call(lib, ix, b, p, n_records=None, samples=True, totals=True, want_rc=0):
    """The raw call on torch tensors of the current device -> the outputs as numpy arrays, as expected() returns them."""
    import torch
    dev = "cuda"
    so, rec = b["sel_offsets"], b["records"]
    N = so.size - 1
    n_records = rec.shape[0] if n_records is None else n_records
    held = np.zeros((max(n_records, 1), 12), np.int32)
    held[:min(n_records, rec.shape[0])] = rec[:n_records]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    d_so, d_rec = t(so), t(held)
    stats = torch.full((3, 12), -77, dtype=torch.int64, device=dev)
    smp = torch.full((N // 2 + 3, 2), -77, dtype=torch.int32, device=dev) if samples else None
    tt = torch.full((4,), -77, dtype=torch.int64, device=dev) if totals else None
    wsb = lib.genie_insert_size_stats_workspace_bytes(N, p.max_span)
    ws = torch.full((max(wsb, 256),), 0x5A, dtype=torch.uint8, device=dev)
    assert ws.data_ptr() % 256 == 0
    vp = lambda x, on=True: C.c_void_p(x.data_ptr() if x is not None and on else 0)      # noqa: E731
    rc = lib.genie_insert_size_stats(ix._h, N, vp(d_so), vp(d_rec, n_records > 0), n_records, *[int(v) for v in p], vp(stats), vp(smp),
                                     vp(tt), vp(ws), wsb, C.c_void_p(0))
    torch.cuda.synchronize()
    assert rc == want_rc, rc
    if want_rc:
        return None
    res = {"stats": stats.cpu().numpy()}
    if samples:
        assert (smp[N // 2:] == -77).all(), "rows past the last pair were written"
        res["samples"] = smp[:N // 2].cpu().numpy()
    if totals:
        res["totals"] = tt.cpu().numpy()
    return res


def guarded_call(lib, ix, a, s, b, p, n_records=None, samples=True, totals=True, want_rc=0):
    """The call on the guarded buffers of tests/guarded.py: inputs frozen, every output and the workspace cut from the arena
    `a` with exactly the declared bytes and the weakest alignment the header allows, ONE call on stream `s` without
    synchronising -> a contract_calls.Call."""
    import contract_calls as CC
    from guarded import as_numpy
    so, rec = b["sel_offsets"], b["records"]
    N = so.size - 1
    n_records = rec.shape[0] if n_records is None else n_records
    held = np.zeros((n_records, 12), np.int32)
    held[:min(n_records, rec.shape[0])] = rec[:n_records]
    pso = CC._inp(a, "sel_offsets", so, 8)
    prec = CC._inp(a, "records", held, 16) if n_records else 0
    P = N // 2
    stats = a.alloc("stats", 3 * 12 * 8, 8)
    smp = a.alloc("samples", P * 8, 8) if samples else None
    tt = a.alloc("totals", 32, 8) if totals else None
    w, wb = CC._workspace(a, lib.genie_insert_size_stats_workspace_bytes(N, p.max_span), None)
    adr = lambda t_, name: CC._vp(a.addr(name) if t_ is not None else 0)      # noqa: E731
    rc_ = lib.genie_insert_size_stats(ix._h, N, CC._vp(pso), CC._vp(prec), n_records, *[int(v) for v in p], adr(stats, "stats"),
                                      adr(smp, "samples"), adr(tt, "totals"), CC._vp(w), wb, CC._vp(s))

    def collect():
        res = {"stats": as_numpy(stats, np.int64, (3, 12))}
        if samples:
            res["samples"] = as_numpy(smp, np.int32, (P, 2))
        if totals:
            res["totals"] = as_numpy(tt, np.int64)
        return res
    return CC.Call("insert_size_stats", rc_, collect, want_rc)
