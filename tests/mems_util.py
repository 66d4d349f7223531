"""The specification of genie_find_mems restated in Python by brute force, for the references of lookup_util.family() (at
most 4096 bases): along every diagonal t - p of the (read, reference) grid, the maximal runs of equal non-break bases.
Nothing here comes from the library under test; the suffix-array rows are lookup_util.suffix_rows, the occurrences of a
seed lookup_util.interval.  Also the raw ctypes call the GPU tests make and the call on guarded buffers.

A MEM of a strand-read Q (L bases) on the reference T (n bases) is (p, t, l), l >= m: Q[p .. p+l) == T[t .. t+l) with no
break inside, Q[p+l] != T[t+l] or an end on the right, Q[p-1] != T[t-1] or a start on the left; a break (a code > 3, with
SPLIT also a base the reference lacks) equals nothing.  Its row is (p, p + l, t + 1, r), r the suffix-array row of suffix
t; the rows of a strand-read are ordered by (p, r).  Without SPLIT a strand-read with a code > 3 is flagged
GENIE_READ_BAD_BASE and has no rows.  max_occ > 0: a position whose m bases from p on hold no break and occur more than
max_occ times contributes no rows and counts as skipped."""
import ctypes as C

import numpy as np

import lookup_util as U
import match_stats_util as MS

BOTH, SPLIT = MS.BOTH, MS.SPLIT
READ_OK, READ_BAD_BASE, READ_ABSENT_BASE = MS.READ_OK, MS.READ_BAD_BASE, MS.READ_ABSENT_BASE
KEEP = 3                # remembered runs: those of at least this many bases
_RUNS = {}              # (reference bytes, strand-read bytes) -> (p, t, l) of every maximal run of at least KEEP bases
_INV = {}               # reference bytes -> row of every suffix start


def _inverse_rows(ref):
    key = U._bytes(ref)
    if key not in _INV:
        rows = U.suffix_rows(ref)
        inv = np.zeros(len(rows), np.int64)
        inv[rows] = np.arange(len(rows))
        _INV[key] = inv
    return _INV[key]


def maximal_runs(ref, read, floor=1):
    """(p, t, l) int64 arrays of every maximal run of at least `floor` equal bases along a diagonal; a code > 3 of the read
    equals nothing (a base the reference lacks equals nothing by itself)."""
    ref, read = np.asarray(ref, np.uint8), np.asarray(read, np.uint8)
    n, L = len(ref), len(read)
    ps, ts, ls = [], [], []
    nxt = np.zeros(n + 1, np.int64)                              # run length from (p + 1, t + 1) on
    eq = (ref == read[L - 1]) & (read[L - 1] < 4) if L else None
    for p in range(L - 1, -1, -1):
        before = (ref == read[p - 1]) & (read[p - 1] < 4) if p else np.zeros(n, bool)
        run = np.where(eq, nxt[1:] + 1, 0)
        first = eq.copy()
        first[1:] &= ~before[:-1]                                # t == 0 or p == 0 or the bases in front differ
        t = np.flatnonzero(first & (run >= floor))
        ps.append(np.full(t.size, p, np.int64))
        ts.append(t)
        ls.append(run[t])
        nxt[:n] = run
        eq = before
    cat = lambda x: np.concatenate(x) if x else np.zeros(0, np.int64)      # noqa: E731
    return cat(ps), cat(ts), cat(ls)


def _runs(ref, read, m):
    if m < KEEP:
        return maximal_runs(ref, read, m)
    key = (U._bytes(ref), U._bytes(read))
    if key not in _RUNS:
        _RUNS[key] = maximal_runs(ref, read, KEEP)
    return _RUNS[key]


def breaks_of(ref, read, split):
    read = np.asarray(read, np.uint8)
    brk = read > 3
    if split:
        brk |= ~np.isin(read, np.unique(ref))
    return brk


def skipped_positions(ref, read, m, split, max_occ):
    """The positions whose seed (m bases, no break) occurs more than max_occ times."""
    if max_occ <= 0:
        return np.zeros(0, np.int64)
    read = np.asarray(read, np.uint8)
    rows, brk = U.suffix_rows(ref), breaks_of(ref, read, split)
    nb = np.concatenate([[0], np.cumsum(brk)])
    out = []
    for p in range(0, len(read) - m + 1):
        if nb[p + m] - nb[p]:
            continue
        lo, hi = U.interval(ref, rows, read[p:p + m])
        if lo >= 0 and hi - lo + 1 > max_occ:
            out.append(p)
    return np.asarray(out, np.int64)


def expected_one(ref, read, m, split, max_occ=0):
    """(rows int32 [R, 4], status, skipped) of one strand-read."""
    read = np.asarray(read, np.uint8)
    assert m >= 1
    lacks = bool((~np.isin(read, np.unique(ref)) & (read < 4)).any())
    if not split and (read > 3).any():
        return np.zeros((0, 4), np.int32), READ_BAD_BASE, 0
    status = READ_OK if split or not lacks else READ_ABSENT_BASE
    p, t, l = _runs(ref, read, m)
    keep = l >= m
    skip = skipped_positions(ref, read, m, split, max_occ)
    if skip.size:
        keep &= ~np.isin(p, skip)
    p, t, l = p[keep], t[keep], l[keep]
    r = _inverse_rows(ref)[t]
    order = np.lexsort((r, p))
    rows = np.stack([p, p + l, t + 1, r], 1)[order].astype(np.int32).reshape(-1, 4)
    return rows, status, int(skip.size)


def expected(ref, reads, flags, m, max_occ=0):
    """What the call returns -> (offsets int64 [S N + 1], rows int32 [R, 4], status int32 [S N], skipped)."""
    strands, split = (2 if flags & BOTH else 1), bool(flags & SPLIT)
    res = [expected_one(ref, r, m, split, max_occ) for r in MS.strand_reads(reads, strands)]
    off = np.zeros(len(res) + 1, np.int64)
    off[1:] = np.cumsum([x[0].shape[0] for x in res])
    rows = np.concatenate([x[0] for x in res] + [np.zeros((0, 4), np.int32)]).astype(np.int32).reshape(-1, 4)
    return off, rows, np.asarray([x[1] for x in res], np.int32), sum(x[2] for x in res)


def is_mem(ref, read, row, split):
    """One row checked against the definition, base by base."""
    ref, read = np.asarray(ref, np.uint8), np.asarray(read, np.uint8)
    brk = breaks_of(ref, read, split)
    p, e, t = int(row[0]), int(row[1]), int(row[2]) - 1
    l = e - p
    same = lambda a, b: 0 <= a < len(read) and 0 <= b < len(ref) and not brk[a] and read[a] == ref[b]      # noqa: E731
    return (l >= 1 and all(same(p + j, t + j) for j in range(l)) and not same(p + l, t + l) and not same(p - 1, t - 1)
            and int(U.suffix_rows(ref)[int(row[3])]) == t)


# ------------------------------------------------------------------ the raw call
def call(lib, ix, flags, bases, offs, m, max_occ=0, cap=0, rows=True, status=True, totals=True, max_len=None, ws_mult=1, fill=-7,
         want_rc=0, spare=0):
    """One raw genie_find_mems on torch buffers of exactly the declared sizes (d_rows: cap + spare rows, of which the call
    is told cap; rows=False: NULL), the workspace exactly what its size function returns, every output filled with `fill`
    first -> (offsets, rows [cap + spare, 4] or None, status or None, totals or None) as numpy."""
    import torch
    bases, offs = np.asarray(bases, np.uint8), np.asarray(offs, np.int64)
    n, total = offs.size - 1, int(bases.size)
    strands = 2 if flags & BOTH else 1
    if max_len is None:
        max_len = int(np.diff(offs).max()) if n else 0
    b = torch.as_tensor(bases if total else np.zeros(1, np.uint8)).cuda()
    of = torch.as_tensor(offs).cuda()
    ws_bytes = lib.genie_find_mems_workspace_bytes(n, total, max_len, flags)
    assert ws_bytes >= lib.genie_match_stats_workspace_bytes(n, total, max_len, flags) >= 0
    ws_bytes *= ws_mult
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device="cuda")
    out = torch.full((strands * n + 1,), fill, dtype=torch.int64, device="cuda")
    rw = torch.full((max(cap + spare, 1), 4), fill, dtype=torch.int32, device="cuda") if rows else None
    st = torch.full((strands * n,), fill, dtype=torch.int32, device="cuda") if status else None
    tt = torch.full((2,), fill, dtype=torch.int64, device="cuda") if totals else None
    p = lambda t: C.c_void_p(t.data_ptr() if t is not None and t.numel() else 0)      # noqa: E731
    rc_ = lib.genie_find_mems(ix._h, flags, p(b), p(of), n, total, max_len, m, max_occ, p(out), p(rw), cap, p(st), p(tt), p(ws),
                              ws_bytes, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc_ == want_rc, rc_
    if rc_:
        return None
    return (out.cpu().numpy(), rw.cpu().numpy()[:cap + spare] if rows else None, st.cpu().numpy() if status else None,
            tt.cpu().numpy() if totals else None)


def sized_call(lib, ix, flags, bases, offs, m, max_occ=0):
    """The sizing call (d_rows NULL), then the call with exactly that room -> (offsets, rows, status, totals)."""
    off0, none, st0, tt0 = call(lib, ix, flags, bases, offs, m, max_occ, rows=False)
    assert none is None and tt0[0] == off0[-1]
    off, rows, st, tt = call(lib, ix, flags, bases, offs, m, max_occ, cap=int(off0[-1]))
    assert np.array_equal(off, off0) and np.array_equal(st, st0) and np.array_equal(tt, tt0)
    return off, rows, st, tt


def guarded_call(lib, ix, a, s, flags, reads, m, max_occ, cap, lead=0, tail=0, status=True, totals=True):
    """The call on the guarded buffers of tests/guarded.py, as tests/contract_calls.py makes the others: inputs frozen,
    every output and the workspace cut from the arena `a` with exactly the declared bytes and the weakest alignment the
    header allows, ONE call on stream `s` without synchronising -> a contract_calls.Call."""
    import contract_calls as CC
    from guarded import as_numpy
    bases, offs = MS.csr(reads, lead, tail, fill=3)
    n, total = len(reads), int(bases.size)
    strands = 2 if flags & BOTH else 1
    max_len = max([len(r) for r in reads] + [0])
    p = CC._inp(a, "bases", bases)
    po = CC._inp(a, "read_offsets", offs, 8)
    out = a.alloc("offsets", (strands * n + 1) * 8, 8)
    rows = a.alloc("rows", cap * 16, 16)
    st = a.alloc("status", strands * n * 4, 4) if status else None
    tt = a.alloc("totals", 16, 8) if totals else None
    w, wb = CC._workspace(a, lib.genie_find_mems_workspace_bytes(n, total, max_len, flags), None)
    rc_ = lib.genie_find_mems(ix._h, flags, CC._vp(p), CC._vp(po), n, total, max_len, m, max_occ, CC._vp(a.addr("offsets")),
                              CC._vp(a.addr("rows")), cap, CC._vp(a.addr("status") if status else 0),
                              CC._vp(a.addr("totals") if totals else 0), CC._vp(w), wb, CC._vp(s))

    def collect():
        off = as_numpy(out, np.int64)
        held = min(int(off[-1]), cap)
        res = {"offsets": off, "rows": as_numpy(rows, np.int32, (cap, 4))[:held]}
        assert a.holds_poison(rows[held * 16:]), "rows past the total were written"
        if status:
            res["status"] = as_numpy(st, np.int32)
        if totals:
            res["totals"] = as_numpy(tt, np.int64)
        return res
    return CC.Call("find_mems", rc_, collect)
