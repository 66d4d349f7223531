"""The brute forces of genie_rescue_windows and genie_window_mems (include/genie_smem.h) in plain Python -- the planner's rule
restated line by line, the window MEMs from mems_util.maximal_runs on the slice T[wb:we], then the union and the sort -- with
the raw ctypes calls, the calls on the guarded buffers of tests/guarded.py, and generators.  Nothing here comes from the
library under test."""
import ctypes as C

import numpy as np

import match_stats_util as MS
import mems_util as MM

WINDOW_MAX, WINDOW_MAX_ROWS, MAX_READ_LEN = 65536, 2048, 8192      # GENIE_WINDOW_MAX, GENIE_WINDOW_MAX_ROWS, GENIE_MAX_READ_LEN
SEARCHED, ROW_CAP, TOO_LONG_READ = 1, 2, 4                         # d_status
UNIT_BYTES = (8, 4, 4, 4, 4, 16, 16)                               # the workspace pieces per unit, each rounded to 256 on its own
BOTH, SPLIT = 1, 2
INVALID, NO_DEVICE, CAPACITY, TOO_LONG = -1, -4, -10, -6
FR, RF, SAME = 1, 2, 4


def clamp(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


# ------------------------------------------------------------------ the planner
def plan(n, table, read_offsets, sel_offsets, records, pairs, orient, isize_max, min_anchor_score, n_records=None):
    """-> (windows int32[2 N, 2], totals int64[3]); table: the contig offsets or None."""
    N = len(sel_offsets) - 1
    assert N % 2 == 0
    n_records = records.shape[0] if n_records is None else n_records
    R = clamp(int(sel_offsets[N]), 0, n_records)
    windows = np.zeros((2 * N, 2), np.int32)
    target = np.zeros(N, np.int64)

    def cut(lo, hi, clo, clen):
        lo, hi = clamp(lo, 0, clen), clamp(hi, 0, clen)
        if hi <= lo:
            return (0, 0)
        return (clo + lo, clo + min(hi, lo + WINDOW_MAX))
    for r in range(N):
        pr = pairs[r // 2]
        a = int(pr[0] if r % 2 else pr[1])                           # the other mate's chosen record
        if int(pr[2]) & 1 or not 0 <= a < R or int(records[a, 9]) < min_anchor_score:
            continue
        target[r] = 1
        if read_offsets[r + 1] <= read_offsets[r]:
            continue
        sa = 1 if int(records[a, 3]) != 0 else 0
        clo, chi = 0, n
        if table is not None:
            c = clamp(int(records[a, 4]), 0, len(table) - 2)
            clo = clamp(int(table[c]), 0, n)
            chi = clamp(int(table[c + 1]), clo, n)
        b = int(records[a, 5]) - 1
        e = b + int(records[a, 6])
        fr, rf = bool(orient & FR), bool(orient & RF)
        right = (fr and sa == 0) or (rf and sa == 1)
        left = (fr and sa == 1) or (rf and sa == 0)
        if right or left:
            windows[2 * r + 1 - sa] = cut(e - isize_max if left else b, b + isize_max if right else e, clo, chi - clo)
        if orient & SAME:
            windows[2 * r + sa] = cut(e - isize_max, b + isize_max, clo, chi - clo)
    has = (windows[:, 1] > windows[:, 0]).reshape(-1, 4) if N else np.zeros((0, 4), bool)
    totals = np.asarray([has.sum(), has.any(axis=1).sum(), target.sum()], np.int64)
    return windows, totals


def plan_batch(reads, lengths=None):
    """reads: per read a list of (strand, contig, offset, r_span, score), its first the chosen record -> a dict with
    read_offsets, sel_offsets, records and pairs whose rec0 / rec1 are the heads and whose proper bit is clear."""
    N = len(reads)
    so = np.zeros(N + 1, np.int64)
    so[1:] = np.cumsum([len(r) for r in reads])
    rec = np.zeros((int(so[-1]), 12), np.int32)
    for i, rows in enumerate(reads):
        for k, (strand, contig, offset, r_span, score) in enumerate(rows):
            rec[so[i] + k] = (i, so[i] + k, 0 if k == 0 else 2, strand, contig, offset, r_span, 0, r_span, score, 0, 0)
    pairs = np.zeros((N // 2, 8), np.int32)
    for k in range(N // 2):
        h0, h1 = len(reads[2 * k]) > 0, len(reads[2 * k + 1]) > 0
        pairs[k] = (so[2 * k] if h0 else -1, so[2 * k + 1] if h1 else -1, (2 if h0 else 0) | (4 if h1 else 0), 0, 0, 0, 0, -1)
    roff = np.zeros(N + 1, np.int64)
    roff[1:] = np.cumsum([100] * N if lengths is None else lengths)
    return {"read_offsets": roff, "sel_offsets": so, "records": rec, "pairs": pairs}


# ------------------------------------------------------------------ window MEMs
def clamp_window(w, n):
    wb, we = clamp(int(w[0]), 0, n), clamp(int(w[1]), 0, n)
    we = max(we, wb)
    return wb, min(we, wb + WINDOW_MAX)


def window_rows(T, Q, wb, we, m):
    """The MEMs of Q against T[wb:we) as a reference of its own -> a list of (start, end, pos, -1)."""
    p, t, l = MM.maximal_runs(np.asarray(T[wb:we], np.uint8), Q, m)
    return [(int(a), int(a + c), wb + int(b) + 1, -1) for a, b, c in zip(p, t, l)]


def union(in_rows, win_rows):
    """The set union on (start, end, pos), column 3 from the first input row with the triple, by (start, pos, end)."""
    col3 = {}
    for r in list(in_rows) + list(win_rows):
        col3.setdefault((int(r[0]), int(r[1]), int(r[2])), int(r[3]))
    return [(s, e, p, col3[(s, e, p)]) for s, e, p in sorted(col3, key=lambda k: (k[0], k[2], k[1]))]


def expected(T, reads, S, windows, m, in_offsets=None, in_rows=None):
    """What the call returns -> (offsets int64[U + 1], rows int32[R, 4], status int32[U], totals int64[3])."""
    n = len(T)
    units = MS.strand_reads(reads, S)
    U = len(units)
    assert len(windows) == U
    out, status, offs, added = [], np.zeros(U, np.int32), np.zeros(U + 1, np.int64), 0
    for u, Q in enumerate(units):
        mine = [] if in_offsets is None else [tuple(int(v) for v in r) for r in in_rows[in_offsets[u]:in_offsets[u + 1]]]
        wb, we = clamp_window(windows[u], n)
        if we > wb:
            if len(Q) > MAX_READ_LEN:
                status[u] = TOO_LONG_READ
            else:
                found = window_rows(T, Q, wb, we, m)
                if len(mine) + len(found) > WINDOW_MAX_ROWS:
                    status[u] = ROW_CAP
                else:
                    status[u] = SEARCHED
                    both = union(mine, found)
                    added += len(both) - len(union(mine, []))
                    mine = both
        out += mine
        offs[u + 1] = len(out)
    rows = np.asarray(out, np.int32).reshape(-1, 4)
    return offs, rows, status, np.asarray([len(out), added, int(((status & 6) != 0).sum())], np.int64)


def csr(reads):
    off = np.zeros(len(reads) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in reads])
    bases = np.concatenate([np.asarray(r, np.uint8) for r in reads]) if len(reads) and off[-1] else np.zeros(0, np.uint8)
    return bases.astype(np.uint8), off


def planted_units(rng, T, lengths, windows_len, m, S=1, subs=0.08):
    """One read per entry of lengths: a piece of T with substitutions (and, for some, a code 4), on either strand, with a window
    of windows_len[i] bases laid over where it came from (strand 1 of a read with S == 2) -> (reads, windows int32[S N, 2])."""
    n = len(T)
    reads, windows = [], []
    for L, B in zip(lengths, windows_len):
        at = int(rng.integers(0, max(n - L, 1)))
        q = np.asarray(T[at:at + L], np.uint8).copy()
        if len(q) < L:                                               # a read longer than the reference: its piece, repeated
            q = np.resize(q, L)
        hit = rng.random(L) < subs
        q[hit] = (q[hit] + rng.integers(1, 4, int(hit.sum()))) % 4
        if L > 3 and rng.random() < 0.3:
            q[int(rng.integers(0, L))] = 4
        strand = int(rng.integers(0, S))
        reads.append(MS.rc(q) if strand else q)
        wb = clamp(at - int(rng.integers(0, max(B // 2, 1))), 0, n)
        for s in range(S):
            windows.append((wb, min(wb + B, n)) if s == strand else (0, 0))
    return reads, np.asarray(windows, np.int32).reshape(-1, 2)


# ------------------------------------------------------------------ the raw calls
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _vp(t, on=True):
    return C.c_void_p(t.data_ptr() if t is not None and on else 0)


def call_plan(lib, ix, b, table, orient, isize_max, min_anchor_score, n_records=None, totals=True, want_rc=0):
    """The raw genie_rescue_windows on torch buffers of exactly the declared sizes -> (windows, totals or None) as numpy."""
    import torch
    so, rec, pairs, roff = b["sel_offsets"], b["records"], b["pairs"], b["read_offsets"]
    N = so.size - 1
    n_records = rec.shape[0] if n_records is None else n_records
    held = np.zeros((max(n_records, 1), 12), np.int32)
    held[:min(n_records, rec.shape[0])] = rec[:n_records]
    d_so, d_rec, d_pairs, d_roff = _dev(so), _dev(held), _dev(pairs if N else np.zeros((1, 8), np.int32)), _dev(roff)
    d_tab = _dev(np.asarray(table, np.int64)) if table is not None else None
    win = torch.full((max(2 * N, 1) + 3, 2), -77, dtype=torch.int32, device="cuda")
    tt = torch.full((3,), -77, dtype=torch.int64, device="cuda") if totals else None
    wsb = lib.genie_rescue_windows_workspace_bytes(N)
    ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device="cuda")
    rc = lib.genie_rescue_windows(ix._h, _vp(d_tab), 0 if table is None else len(table) - 1, _vp(d_roff), N, _vp(d_so),
                                  _vp(d_rec, n_records > 0), n_records, _vp(d_pairs, N > 0), orient, isize_max, min_anchor_score,
                                  _vp(win, N > 0), _vp(tt), _vp(ws), wsb, C.c_void_p(0))
    torch.cuda.synchronize()
    assert rc == want_rc, rc
    if want_rc:
        return None
    assert (win[2 * N:] == -77).all(), "windows past 2 N were written"
    return win[:2 * N].cpu().numpy(), (tt.cpu().numpy() if totals else None)


def call_mems(lib, ix, flags, reads, windows, m, in_offsets=None, in_rows=None, cap=0, rows=True, status=True, totals=True, spare=3,
              want_rc=0):
    """One raw genie_window_mems on torch buffers of exactly the declared sizes (d_rows: cap + spare rows, of which the call is
    told cap; rows=False: NULL) -> (offsets, rows [cap + spare, 4] or None, status or None, totals or None) as numpy."""
    import torch
    bases, off = csr(reads)
    N, S = len(reads), 2 if flags & BOTH else 1
    U = S * N
    d_bases, d_off = _dev(bases if bases.size else np.zeros(1, np.uint8)), _dev(off)
    d_win = _dev(np.asarray(windows, np.int32).reshape(-1, 2) if U else np.zeros((1, 2), np.int32))
    d_ioff = _dev(np.asarray(in_offsets, np.int64)) if in_offsets is not None else None
    n_in = 0 if in_rows is None else len(in_rows)
    d_irows = _dev(np.asarray(in_rows, np.int32).reshape(-1, 4)) if n_in else None
    offs = torch.full((U + 1,), -7, dtype=torch.int64, device="cuda")
    out = torch.full((cap + spare, 4), -7, dtype=torch.int32, device="cuda") if rows else None
    st = torch.full((max(U, 1),), -7, dtype=torch.int32, device="cuda") if status else None
    tt = torch.full((3,), -7, dtype=torch.int64, device="cuda") if totals else None
    wsb = lib.genie_window_mems_workspace_bytes(U)
    ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device="cuda")
    max_len = int(np.diff(off).max()) if N else 0
    rc = lib.genie_window_mems(ix._h, flags, _vp(d_bases), _vp(d_off), N, int(off[-1]), max_len, U, _vp(d_win, U > 0), m, _vp(d_ioff),
                               _vp(d_irows), n_in, _vp(offs), _vp(out), cap, _vp(st), _vp(tt), _vp(ws), wsb, C.c_void_p(0))
    torch.cuda.synchronize()
    assert rc == want_rc, rc
    if want_rc:
        return None
    host = lambda t: None if t is None else t.cpu().numpy()      # noqa: E731
    return host(offs), host(out), (host(st)[:U] if status else None), host(tt)


def sized_call(lib, ix, flags, reads, windows, m, in_offsets=None, in_rows=None):
    """The sizing call (d_rows NULL), then the call with exactly that room -> (offsets, rows, status, totals)."""
    off0, none, st0, tt0 = call_mems(lib, ix, flags, reads, windows, m, in_offsets, in_rows, rows=False)
    assert none is None and tt0[0] == off0[-1]
    cap = int(off0[-1])
    off, rows, st, tt = call_mems(lib, ix, flags, reads, windows, m, in_offsets, in_rows, cap=cap)
    assert np.array_equal(off, off0) and np.array_equal(st, st0) and np.array_equal(tt, tt0)
    assert (rows[cap:] == -7).all(), "rows past the capacity were written"
    return off, rows[:cap], st, tt


def agrees(got, want):
    for k, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, (k, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert bad.size == 0, (k, bad[:4].tolist(), g[tuple(bad[0])].tolist() if g.ndim == 1 else g[bad[0][0]].tolist(),
                               w[tuple(bad[0])].tolist() if w.ndim == 1 else w[bad[0][0]].tolist())


# ------------------------------------------------------------------ the calls on guarded buffers
def guarded_plan(lib, ix, a, s, b, table, orient, isize_max, min_anchor_score, n_records=None, totals=True, want_rc=0):
    """genie_rescue_windows on the guarded buffers of tests/guarded.py: inputs frozen, every output and the workspace cut from
    the arena `a` with exactly the declared bytes and the weakest alignment the header allows, ONE call on stream `s` without
    synchronising -> a contract_calls.Call."""
    import contract_calls as CC
    from guarded import as_numpy
    so, rec, pairs, roff = b["sel_offsets"], b["records"], b["pairs"], b["read_offsets"]
    N = so.size - 1
    n_records = rec.shape[0] if n_records is None else n_records
    held = np.zeros((n_records, 12), np.int32)
    held[:min(n_records, rec.shape[0])] = rec[:n_records]
    ptab = CC._inp(a, "table", np.asarray(table, np.int64), 8) if table is not None else 0
    proff, pso = CC._inp(a, "read_offsets", roff, 8), CC._inp(a, "sel_offsets", so, 8)
    prec = CC._inp(a, "records", held, 16) if n_records else 0
    ppairs = CC._inp(a, "pairs", pairs, 16)
    win = a.alloc("windows", 2 * N * 8, 8)
    tt = a.alloc("totals", 24, 8) if totals else None
    w, wb = CC._workspace(a, lib.genie_rescue_windows_workspace_bytes(N), None)
    rc = lib.genie_rescue_windows(ix._h, CC._vp(ptab), 0 if table is None else len(table) - 1, CC._vp(proff), N, CC._vp(pso), CC._vp(prec),
                                  n_records, CC._vp(ppairs), orient, isize_max, min_anchor_score, CC._vp(a.addr("windows")),
                                  CC._vp(a.addr("totals") if totals else 0), CC._vp(w), wb, CC._vp(s))

    def collect():
        res = {"windows": as_numpy(win, np.int32, (2 * N, 2))}
        if totals:
            res["totals"] = as_numpy(tt, np.int64)
        return res
    return CC.Call("rescue_windows", rc, collect, want_rc)


def guarded_mems(lib, ix, a, s, flags, reads, windows, m, in_offsets=None, in_rows=None, cap=0, status=True, totals=True, want_rc=0):
    """genie_window_mems on guarded buffers, as guarded_plan -> a contract_calls.Call whose result holds offsets, rows (the first
    min(total, cap)), status and totals; rows past the total still hold the poison."""
    import contract_calls as CC
    from guarded import as_numpy
    bases, off = csr(reads)
    N, S = len(reads), 2 if flags & BOTH else 1
    U = S * N
    pb = CC._inp(a, "bases", bases, 1) if bases.size else 0
    po = CC._inp(a, "read_offsets", off, 8)
    pw = CC._inp(a, "windows", np.asarray(windows, np.int32).reshape(-1, 2), 8)
    pio = CC._inp(a, "in_offsets", np.asarray(in_offsets, np.int64), 8) if in_offsets is not None else 0
    n_in = 0 if in_rows is None else len(in_rows)
    pir = CC._inp(a, "in_rows", np.asarray(in_rows, np.int32).reshape(-1, 4), 16) if n_in else 0
    offs = a.alloc("offsets", (U + 1) * 8, 8)
    out = a.alloc("rows", cap * 16, 16)
    st = a.alloc("status", U * 4, 4) if status else None
    tt = a.alloc("totals", 24, 8) if totals else None
    w, wb = CC._workspace(a, lib.genie_window_mems_workspace_bytes(U), None)
    max_len = int(np.diff(off).max()) if N else 0
    rc = lib.genie_window_mems(ix._h, flags, CC._vp(pb), CC._vp(po), N, int(off[-1]), max_len, U, CC._vp(pw), m, CC._vp(pio), CC._vp(pir),
                               n_in, CC._vp(a.addr("offsets")), CC._vp(a.addr("rows") if cap else 0), cap,
                               CC._vp(a.addr("status") if status else 0), CC._vp(a.addr("totals") if totals else 0), CC._vp(w), wb,
                               CC._vp(s))

    def collect():
        res = {"offsets": as_numpy(offs, np.int64)}
        kept = min(int(res["offsets"][-1]), cap)
        res["rows"] = as_numpy(out, np.int32, (cap, 4))[:kept]
        assert a.holds_poison(out[kept * 16:]), "rows past the total were written"
        if status:
            res["status"] = as_numpy(st, np.int32)
        if totals:
            res["totals"] = as_numpy(tt, np.int64)
        return res
    return CC.Call("window_mems", rc, collect, want_rc)
