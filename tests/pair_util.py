"""The brute force of genie_pair_alignments (include/genie_smem.h) in plain Python -- every combination of every pair, straight
from the definition -- with the raw ctypes call, the call on the guarded buffers of tests/guarded.py, and a generator of
synthetic record batches.

A batch is a dict: sel_offsets int64[N+1] (N even: reads 2k and 2k + 1 are mates), records int32[T, 12] = (read, chain, kind,
strand, contig, offset, r_span, q_begin, q_end, score, sub, mapq) and klass int32[C, 4] = (kind, parent, order, mapq), as
genie_select_alignments writes them."""
import ctypes as C
from collections import namedtuple

import numpy as np

Params = namedtuple("PairParams", "orient isize_min isize_max isize_mean pen_slope pen_max pen_unpaired mapq_boost")
DEFAULTS = Params(1, 0, 1000, 300, 8, 16, 17, 40)        # GenieIndex.pair_alignments' defaults
LANE_MAX, TILE = 64, 256                                 # GENIE_PAIR_LANE_MAX, GENIE_PAIR_TILE
PAIR_BYTES, PAIR_SCAN_BYTES_PER_1024 = 48, 8
FR, RF, SAME, NO_TYPE = 0, 1, 2, 3
INVALID, NO_DEVICE, CAPACITY, TOO_LONG = -1, -4, -10, -6
I32 = (-2**31, 2**31 - 1)


def clamp(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


class Rec:
    """A record as the definition names its parts."""

    def __init__(self, j, row):
        self.j, self.chain, self.kind, self.s, self.contig = j, int(row[1]), int(row[2]), int(row[3]), int(row[4])
        self.b = int(row[5]) - 1
        self.e = self.b + int(row[6])
        self.w, self.q = int(row[9]), clamp(int(row[11]), 0, 60)
        self.own_mapq = int(row[11])


def combo_type(x, y):
    """None without the same contig, else FR, RF, SAME or NO_TYPE."""
    if x.contig != y.contig:
        return None
    if x.s == y.s:
        return SAME
    f, r = (x, y) if x.s == 0 else (y, x)
    if f.b <= r.b and f.e <= r.e:
        return FR
    if r.b <= f.b and r.e <= f.e:
        return RF
    return NO_TYPE


def span(x, y):
    return max(x.e, y.e) - min(x.b, y.b)


def concordant(x, y, p):
    t = combo_type(x, y)
    return t is not None and t != NO_TYPE and (p.orient >> t) & 1 == 1 and p.isize_min <= span(x, y) <= p.isize_max


def value(x, y, p):
    return x.w + y.w - min(p.pen_max, abs(span(x, y) - p.isize_mean) * p.pen_slope // 256)


def pair_mapq(W1, W2, U):
    return 0 if W1 <= 0 else 60 * (W1 - min(max(W2, U, 0), W1)) // W1


def record_mapq(q, proper, pmapq, boost):
    """The mapq of a chosen record whose own is q (already in [0, 60])."""
    return max(q, min(pmapq, q + boost)) if proper else q


def read_records(b, r, R):
    so = b["sel_offsets"]
    lo = clamp(int(so[r]), 0, R)
    return lo, clamp(int(so[r + 1]), lo, R)


def candidates(b, r, R, cap):
    lo, hi = read_records(b, r, R)
    rec, klass = b["records"], b["klass"]
    out = []
    for j in range(lo, hi):
        x = Rec(j, rec[j])
        if j == lo or (x.kind == 2 and cap > 0 and int(klass[clamp(x.chain, 0, cap - 1), 1]) == int(rec[lo, 1])):
            out.append(x)
    return out


def expected(b, p, n_records=None, cap=None):
    """Every output of the call: {"pairs": int32[P, 8], "sam": int32[R, 4], "totals": int64[4], "mapq": the pairs' mapq}."""
    so, rec = b["sel_offsets"], b["records"]
    N = so.size - 1
    assert N % 2 == 0
    n_records = rec.shape[0] if n_records is None else n_records
    cap = b["klass"].shape[0] if cap is None else cap
    R = clamp(int(so[N]), 0, n_records)
    pairs = np.zeros((N // 2, 8), np.int32)
    sam = np.zeros((R, 4), np.int32)
    pmapqs = np.zeros(N // 2, np.int64)
    totals = np.zeros(4, np.int64)
    for k in range(N // 2):
        c0, c1 = candidates(b, 2 * k, R, cap), candidates(b, 2 * k + 1, R, cap)
        combos = sorted(((-value(x, y, p), x.j, y.j, x, y) for x in c0 for y in c1 if concordant(x, y, p)), key=lambda t: t[:3])
        has0, has1 = bool(c0), bool(c1)
        W1 = -combos[0][0] if combos else 0
        W2 = -combos[1][0] if len(combos) > 1 else 0                # the list is sorted by W descending
        U = c0[0].w + c1[0].w - p.pen_unpaired if has0 and has1 else None
        proper = has0 and has1 and bool(combos) and W1 >= U
        chosen = [c0[0] if has0 else None, c1[0] if has1 else None]
        pmapq = 0
        if proper:
            chosen = [combos[0][3], combos[0][4]]
            pmapq = pair_mapq(W1, W2, U)
        pmapqs[k] = pmapq
        flags = (1 if proper else 0) | (2 if has0 else 0) | (4 if has1 else 0)
        flags |= (8 if has0 and chosen[0].j != c0[0].j else 0) | (16 if has1 and chosen[1].j != c1[0].j else 0)
        isize, typ = 0, -1
        if has0 and has1 and combo_type(*chosen) is not None:
            isize, typ = span(*chosen), combo_type(*chosen)
        pairs[k] = [chosen[0].j if has0 else -1, chosen[1].j if has1 else -1, flags, clamp(W1, *I32), clamp(W2, *I32), clamp(isize, *I32),
                    clamp(len(combos), *I32), typ]
        totals += [has0 and has1, proper, bool(flags & 8) + bool(flags & 16), has0 != has1]
        for m in (0, 1):
            lo, hi = read_records(b, 2 * k + m, R)
            mine, mate = chosen[m], chosen[1 - m]
            for j in range(lo, hi):
                x = Rec(j, rec[j])
                flag = 0x1 | (0x2 if proper else 0) | (0x8 if mate is None else 0) | (0x10 if x.s == 1 else 0)
                flag |= (0x20 if mate is not None and mate.s == 1 else 0) | (0x80 if m else 0x40) | (0x800 if x.kind == 1 else 0)
                is_chosen = mine is not None and mine.j == j
                if not is_chosen and x.kind != 1:
                    flag |= 0x100
                mapq = record_mapq(x.q, proper, pmapq, p.mapq_boost) if is_chosen else (x.own_mapq if x.kind == 1 else 0)
                tlen = 0
                if mate is not None and mate.contig == x.contig:
                    tlen = span(x, mate) if x.b < mate.b or (x.b == mate.b and m == 0) else -span(x, mate)
                sam[j] = [flag, mapq, mate.j if mate is not None else -1, clamp(tlen, *I32)]
    return {"pairs": pairs, "sam": sam, "totals": totals, "mapq": pmapqs}


def agrees(got, want, keys=("pairs", "sam", "totals")):
    for k in keys:
        if k in got:
            assert got[k].shape == want[k].shape, (k, got[k].shape, want[k].shape)
            bad = np.argwhere(got[k] != want[k])
            assert bad.size == 0, (k, bad[:4].tolist(), got[k][bad[0][0]].tolist(), want[k][bad[0][0]].tolist())


# ------------------------------------------------------------------ batches
def make_batch(reads):
    """reads: per read a list of (kind, parent, strand, contig, offset, r_span, score, mapq); parent is an index into the read's
    own list (the record whose secondary this one is; ignored for kinds 0 and 1).  The chain of record j is 3 j + 1, so chain
    and record indices never agree by accident; klass has a row per chain and rows of kind 3 between them."""
    N = len(reads)
    assert N % 2 == 0
    so = np.zeros(N + 1, np.int64)
    so[1:] = np.cumsum([len(r) for r in reads])
    T = int(so[-1])
    rec, klass = np.zeros((T, 12), np.int32), np.zeros((3 * T + 1, 4), np.int32)
    klass[:] = (3, -1, -1, 0)
    for i, rows in enumerate(reads):
        for n, (kind, parent, strand, contig, offset, r_span, score, mapq) in enumerate(rows):
            j = int(so[i]) + n
            chain = 3 * j + 1
            par = chain if kind < 2 else 3 * (int(so[i]) + parent) + 1
            rec[j] = (i, chain, kind, strand, contig, offset, r_span, 0, r_span, score, 0, mapq)
            klass[chain] = (kind, par, n, mapq)
    return {"sel_offsets": so, "records": rec, "klass": klass}


def random_batch(rng, counts, scores=(60, 90), spread=900, contigs=2, far=0.1):
    """One pair per entry (n0, n1) of counts.  The records of a pair lie within `spread` bases of the pair's anchor on the
    pair's contig, a share `far` of them elsewhere, on either strand; most records past the head are secondaries of the head,
    some are supplementary or secondaries of a supplementary."""
    reads = []
    for n0, n1 in counts:
        contig, anchor = int(rng.integers(0, contigs)), int(rng.integers(1, 100000))
        for n in (n0, n1):
            rows, supp = [], []
            for r in range(n):
                kind, parent = 0, 0
                if r > 0:
                    u = rng.random()
                    kind = 2 if u < 0.8 else 1
                    if kind == 1:
                        supp.append(r)
                    elif supp and u < 0.1:
                        parent = supp[int(rng.integers(0, len(supp)))]
                away = rng.random() < far
                rows.append((kind, parent, int(rng.integers(0, 2)), int(rng.integers(0, contigs)) if away else contig,
                             anchor + int(rng.integers(0, spread)), int(rng.integers(50, 151)), int(rng.integers(scores[0], scores[1])),
                             int(rng.integers(0, 61)) if kind < 2 else 0))
            reads.append(rows)
    return make_batch(reads)


# ------------------------------------------------------------------ the call
def call(lib, ix, b, p, n_records=None, cap=None, totals=True, want_rc=0):
    """The raw call on torch tensors of the current device -> the outputs as numpy arrays, as expected() returns them."""
    import torch
    dev = "cuda"
    so, rec, klass = b["sel_offsets"], b["records"], b["klass"]
    N = so.size - 1
    n_records = rec.shape[0] if n_records is None else n_records
    cap = klass.shape[0] if cap is None else cap
    held_r, held_k = np.zeros((max(n_records, 1), 12), np.int32), np.zeros((max(cap, 1), 4), np.int32)
    held_r[:min(n_records, rec.shape[0])] = rec[:n_records]
    held_k[:min(cap, klass.shape[0])] = klass[:cap]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    d_so, d_rec, d_kl = t(so), t(held_r), t(held_k)
    pairs = torch.full((max(N // 2, 1), 8), -77, dtype=torch.int32, device=dev)
    sam = torch.full((n_records + 3, 4), -77, dtype=torch.int32, device=dev)
    tt = torch.full((4,), -77, dtype=torch.int64, device=dev) if totals else None
    wsb = lib.genie_pair_alignments_workspace_bytes(N, n_records)
    ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device=dev)
    assert ws.data_ptr() % 256 == 0
    vp = lambda x, on=True: C.c_void_p(x.data_ptr() if x is not None and on else 0)      # noqa: E731
    rc = lib.genie_pair_alignments(ix._h, N, vp(d_so), vp(d_rec, n_records > 0), n_records, vp(d_kl, cap > 0), cap, *[int(v) for v in p],
                                   vp(pairs), vp(sam, n_records > 0), vp(tt), vp(ws), wsb, C.c_void_p(0))
    torch.cuda.synchronize()
    assert rc == want_rc, rc
    if want_rc:
        return None
    R = clamp(int(so[N]), 0, n_records)
    assert (sam[R:] == -77).all(), "rows at or past R were written"
    res = {"pairs": pairs[:N // 2].cpu().numpy(), "sam": sam[:R].cpu().numpy()}
    if totals:
        res["totals"] = tt.cpu().numpy()
    return res


def guarded_call(lib, ix, a, s, b, p, n_records=None, cap=None, totals=True, want_rc=0):
    """The call on the guarded buffers of tests/guarded.py: inputs frozen, every output and the workspace cut from the arena
    `a` with exactly the declared bytes and the weakest alignment the header allows, ONE call on stream `s` without
    synchronising -> a contract_calls.Call."""
    import contract_calls as CC
    from guarded import as_numpy
    so, rec, klass = b["sel_offsets"], b["records"], b["klass"]
    N = so.size - 1
    n_records = rec.shape[0] if n_records is None else n_records
    cap = klass.shape[0] if cap is None else cap
    held_r, held_k = np.zeros((n_records, 12), np.int32), np.zeros((cap, 4), np.int32)
    held_r[:min(n_records, rec.shape[0])] = rec[:n_records]
    held_k[:min(cap, klass.shape[0])] = klass[:cap]
    pso = CC._inp(a, "sel_offsets", so, 8)
    prec = CC._inp(a, "records", held_r, 16) if n_records else 0
    pkl = CC._inp(a, "class", held_k, 16) if cap else 0
    P = N // 2
    pairs = a.alloc("pairs", P * 32, 16)
    sam = a.alloc("sam", n_records * 16, 16) if n_records else None
    tt = a.alloc("totals", 32, 8) if totals else None
    w, wb = CC._workspace(a, lib.genie_pair_alignments_workspace_bytes(N, n_records), None)
    adr = lambda t_, name: CC._vp(a.addr(name) if t_ is not None else 0)      # noqa: E731
    rc_ = lib.genie_pair_alignments(ix._h, N, CC._vp(pso), CC._vp(prec), n_records, CC._vp(pkl), cap, *[int(v) for v in p],
                                    adr(pairs, "pairs"), adr(sam, "sam"), adr(tt, "totals"), CC._vp(w), wb, CC._vp(s))
    R = clamp(int(so[N]), 0, n_records)

    def collect():
        res = {"pairs": as_numpy(pairs, np.int32, (P, 8))}
        res["sam"] = as_numpy(sam, np.int32, (n_records, 4))[:R] if n_records else np.zeros((0, 4), np.int32)
        if n_records:
            assert a.holds_poison(sam[R * 16:]), "rows at or past R were written"
        if totals:
            res["totals"] = as_numpy(tt, np.int64)
        return res
    return CC.Call("pair_alignments", rc_, collect, want_rc)
