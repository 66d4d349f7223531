"""The specification of genie_chain_mems restated in Python by brute force, int64 throughout, vectorised per anchor in numpy:
O(n * window) per unit.  Nothing here comes from the library under test.  Also a second, independent extraction of the chains
(minimap2's: anchors by (f descending, index ascending), backtrack until a used anchor), a generator of synthetic anchors,
and the raw ctypes calls the GPU tests make.

A unit is one strand-read's MEM rows (s, e, pos, row), s non-decreasing; l = e - s, t = pos - 1, c the contig of t (0 without
a table).  j may precede i iff j < i, j >= i - max_pred (max_pred > 0), c_j == c_i, dq = s_i - s_j and dr = t_i - t_j in
[1, max_dist], g = |dr - dq| <= bandwidth and gain = min(l_i, dq, dr) - ((g * gap_cost) >> 4) >= 1.
f(i) = max(l_i, max f(j) + gain); p(i) = the largest j attaining it if it exceeds l_i, else -1.  top(i) = the node of i's
subtree with the largest (f, then smallest index); a chain = the anchors of one top; its score = f(top) - f(p(first)) (or
f(top)); kept iff score >= min_score.  Chain rows: (q_begin, q_end, r_begin, r_end, score, n_anchors, contig, last)."""
import ctypes as C
from collections import namedtuple

import numpy as np

Params = namedtuple("Params", "max_dist bandwidth gap_cost max_pred min_score")
DEFAULTS = Params(5000, 500, 2, 5000, 40)
INVALID, NO_DEVICE, CAPACITY, TOO_LONG = -1, -4, -10, -6
ROW_BYTES, ROW_BYTES_CONTIGS, UNIT_BYTES = 24, 28, 8     # the header's workspace figures


def contig_of(ctg_off, t):
    """The contig of 0-based positions t: the unique c with off[c] <= t < off[c+1] (None: all 0)."""
    t = np.asarray(t, np.int64)
    if ctg_off is None:
        return np.zeros(t.shape, np.int64)
    off = np.asarray(ctg_off, np.int64)
    return np.minimum(np.searchsorted(off[1:], t, side="right"), off.size - 2)


def forward(rows, prm, ctg_off=None):
    """(f, p, ties) of one unit; ties counts the anchors whose maximum is attained by more than one j."""
    rows = np.asarray(rows, np.int64).reshape(-1, 4)
    n = rows.shape[0]
    s, l, t = rows[:, 0], rows[:, 1] - rows[:, 0], rows[:, 2] - 1
    c = contig_of(ctg_off, t)
    f, p, ties = np.zeros(n, np.int64), np.full(n, -1, np.int64), 0
    first = np.searchsorted(s, s - prm.max_dist, side="left")        # s sorted: the window is contiguous
    for i in range(n):
        lo = int(first[i])
        if prm.max_pred > 0:
            lo = max(lo, i - prm.max_pred)
        f[i] = l[i]
        if lo >= i:
            continue
        j = np.arange(lo, i)
        dq, dr = s[i] - s[j], t[i] - t[j]
        g = np.abs(dr - dq)
        gain = np.minimum(l[i], np.minimum(dq, dr)) - ((g * prm.gap_cost) >> 4)
        ok = (c[j] == c[i]) & (dq >= 1) & (dq <= prm.max_dist) & (dr >= 1) & (dr <= prm.max_dist) & (g <= prm.bandwidth) & (gain >= 1)
        if not ok.any():
            continue
        v = f[j][ok] + gain[ok]
        m = int(v.max())
        if m > l[i]:
            at = np.flatnonzero(v == m)
            ties += at.size > 1
            f[i], p[i] = m, j[ok][at[-1]]
    return f, p, int(ties)


def tops(f, p):
    """top(i) by the definition: the reverse sweep over the forest."""
    n = len(f)
    top = np.arange(n, dtype=np.int64)
    for i in range(n - 1, -1, -1):
        q = p[i]
        if q >= 0 and (f[top[i]], -top[i]) > (f[top[q]], -top[q]):
            top[q] = top[i]
    return top


def chains_by_top(f, p):
    """[(top, members from the top down)] in top order, by the definition."""
    top = tops(f, p)
    out = []
    for v in np.flatnonzero(top == np.arange(len(f))).tolist():
        members, j = [], v
        while j >= 0 and top[j] == v:
            members.append(j)
            j = int(p[j])
        out.append((v, members))
    assert sum(len(m) for _, m in out) == len(f)
    return out


def chains_by_backtrack(f, p):
    """The same list by minimap2's rule: anchors by (f descending, index ascending), backtrack until a used anchor."""
    n = len(f)
    used = np.zeros(n, bool)
    out = []
    for v in np.lexsort((np.arange(n), -np.asarray(f))).tolist():
        if used[v]:
            continue
        members, j = [], v
        while j >= 0 and not used[j]:
            used[j] = True
            members.append(j)
            j = int(p[j])
        out.append((v, members))
    return sorted(out)


def expected_unit(rows, prm, ctg_off=None, extract=chains_by_top):
    """-> (chains int64 [K, 8] kept ones in top order, anchor_chain, p, f, not kept, ties) of one unit."""
    rows = np.asarray(rows, np.int64).reshape(-1, 4)
    f, p, ties = forward(rows, prm, ctg_off)
    c = contig_of(ctg_off, rows[:, 2] - 1)
    achain = np.full(len(f), -1, np.int64)
    kept, lost = [], 0
    for v, members in extract(f, p):
        u = members[-1]
        score = int(f[v] - (f[p[u]] if p[u] >= 0 else 0))
        if score < prm.min_score:
            lost += 1
            continue
        m = rows[members]
        achain[members] = len(kept)
        kept.append([rows[u, 0], m[:, 1].max(), rows[u, 2], (m[:, 2] + m[:, 1] - m[:, 0]).max(), score, len(members), c[v], v])
    return np.asarray(kept, np.int64).reshape(-1, 8), achain, p, f, lost, ties


def expected(offs, rows, prm, ctg_off=None, extract=chains_by_top):
    """What the call returns -> dict of offsets int64 [U + 1], chains int32 [C, 8], anchor_chain / anchor_pred / anchor_score
    int32 [off[U]], totals int64 [2], and ties (the anchors with more than one best predecessor)."""
    offs, rows = np.asarray(offs, np.int64), np.asarray(rows, np.int64).reshape(-1, 4)
    res = [expected_unit(rows[offs[u]:offs[u + 1]], prm, ctg_off, extract) for u in range(offs.size - 1)]
    co = np.zeros(offs.size, np.int64)
    co[1:] = np.cumsum([r[0].shape[0] for r in res])
    cat = lambda k, w: np.concatenate([r[k] for r in res] + [np.zeros((0,) + w, np.int64)]).astype(np.int32)      # noqa: E731
    return {"offsets": co, "chains": cat(0, (8,)), "anchor_chain": cat(1, ()), "anchor_pred": cat(2, ()), "anchor_score": cat(3, ()),
            "totals": np.asarray([co[-1], sum(r[4] for r in res)], np.int64), "ties": sum(r[5] for r in res)}


# ------------------------------------------------------------------ synthetic anchors
def synth_unit(rng, n, n_ref, diagonals=3, jitter=2, step=3):
    """n rows (s, e, pos, row): sorted starts with repeats (steps 0 .. step - 1), lengths 1 .. 40, positions on a few diagonals
    with jitter, inside [1, n_ref]; column 3 holds a value no call may read."""
    s = np.cumsum(rng.integers(0, step, n)).astype(np.int64)
    l = rng.integers(1, 41, n)
    room = max(1, n_ref - (int(s[-1]) if n else 0) - 60)
    d = rng.integers(0, room, diagonals)
    t = np.clip(s + d[rng.integers(0, diagonals, n)] + rng.integers(-jitter, jitter + 1, n), 0, n_ref - 1)
    return np.stack([s, s + l, t + 1, np.full(n, -12345)], 1).astype(np.int32).reshape(-1, 4)


def synth_batch(rng, sizes, n_ref, **kw):
    """(offsets int64 [U + 1], rows int32 [R, 4]) of units of the given sizes."""
    units = [synth_unit(rng, int(n), n_ref, **kw) for n in sizes]
    offs = np.zeros(len(units) + 1, np.int64)
    offs[1:] = np.cumsum([u.shape[0] for u in units])
    return offs, np.concatenate(units + [np.zeros((0, 4), np.int32)]).astype(np.int32).reshape(-1, 4)


# ------------------------------------------------------------------ the raw calls
def _p(t):
    return C.c_void_p(t.data_ptr() if t is not None and t.numel() else 0)


def call(lib, ix, offs, rows, prm, ctg_off=None, cap=0, chains=True, anchors=(True, True, True), totals=True, total_rows=None,
         fill=-7, want_rc=0, spare=0):
    """One raw genie_chain_mems on torch buffers of exactly the declared sizes (d_chains: cap + spare rows, of which the call is
    told cap; chains=False: NULL; anchors: which of chain / pred / score are given), the workspace exactly what its size function
    returns, every output filled with `fill` first -> dict of numpy arrays (None where the buffer was NULL)."""
    import torch
    offs, rows = np.asarray(offs, np.int64), np.ascontiguousarray(np.asarray(rows, np.int32).reshape(-1, 4))
    U = offs.size - 1
    R = rows.shape[0] if total_rows is None else int(total_rows)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()      # noqa: E731
    of = dev(offs)
    rw = dev(rows if rows.size else np.zeros((1, 4), np.int32))
    tab = dev(np.asarray(ctg_off, np.int64)) if ctg_off is not None else None
    nc = len(ctg_off) - 1 if ctg_off is not None else 0
    ws_bytes = lib.genie_chain_mems_workspace_bytes(U, R, nc)
    assert ws_bytes >= 0 and ws_bytes % 256 == 0
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device="cuda")
    co = torch.full((U + 1,), fill, dtype=torch.int64, device="cuda")
    ch = torch.full((max(cap + spare, 1), 8), fill, dtype=torch.int32, device="cuda") if chains else None
    an = [torch.full((max(R, 1),), fill, dtype=torch.int32, device="cuda") if w else None for w in anchors]
    tt = torch.full((2,), fill, dtype=torch.int64, device="cuda") if totals else None
    rc_ = lib.genie_chain_mems(ix._h, _p(tab), nc, _p(of), _p(rw) if R else C.c_void_p(0), U, R, *[int(x) for x in prm], _p(co), _p(ch),
                               cap, _p(an[0]), _p(an[1]), _p(an[2]), _p(tt), _p(ws), ws_bytes,
                               C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc_ == want_rc, rc_
    if rc_:
        return None
    host = lambda t, k=None: None if t is None else t.cpu().numpy()[:k]      # noqa: E731
    return {"offsets": host(co), "chains": host(ch, cap + spare), "anchor_chain": host(an[0], R), "anchor_pred": host(an[1], R),
            "anchor_score": host(an[2], R), "totals": host(tt)}


def sized_call(lib, ix, offs, rows, prm, ctg_off=None):
    """The sizing call (d_chains NULL), then the call with exactly that room; the two agree in everything else."""
    a = call(lib, ix, offs, rows, prm, ctg_off, chains=False)
    assert a["chains"] is None and a["totals"][0] == a["offsets"][-1]
    b = call(lib, ix, offs, rows, prm, ctg_off, cap=int(a["offsets"][-1]))
    for k in ("offsets", "anchor_chain", "anchor_pred", "anchor_score", "totals"):
        assert np.array_equal(a[k], b[k]), k
    return b


def agrees(got, want, cap=None):
    """Every output of a call equals the brute force (chains up to cap)."""
    R = want["anchor_pred"].size
    assert np.array_equal(got["offsets"], want["offsets"])
    for k in ("anchor_pred", "anchor_score", "anchor_chain"):
        if got[k] is not None:
            assert np.array_equal(got[k][:R], want[k]), k
    if got["totals"] is not None:
        assert np.array_equal(got["totals"], want["totals"])
    if got["chains"] is not None:
        held = want["chains"].shape[0] if cap is None else min(cap, want["chains"].shape[0])
        assert np.array_equal(got["chains"][:held], want["chains"][:held])


def guarded_call(lib, ix, a, s, offs, rows, prm, ctg_off, cap, anchors=(True, True, True), totals=True, want_rc=0, slack=0):
    """The call on the guarded buffers of tests/guarded.py, as tests/contract_calls.py makes the others: inputs frozen, every
    output and the workspace cut from the arena `a` with exactly the declared bytes and the weakest alignment the header
    allows, ONE call on stream `s` without synchronising -> a contract_calls.Call.  slack: rows of d_rows and the anchor arrays
    past off[U], which the call must leave alone."""
    import contract_calls as CC
    from guarded import as_numpy
    offs, rows = np.asarray(offs, np.int64), np.asarray(rows, np.int32).reshape(-1, 4)
    U, used = offs.size - 1, rows.shape[0]
    R = used + slack
    rows = np.concatenate([rows, np.full((slack, 4), 77, np.int32)])
    po = CC._inp(a, "offsets", offs, 8)
    pr = CC._inp(a, "rows", rows, 16) if R else 0
    nc = len(ctg_off) - 1 if ctg_off is not None else 0
    pt = CC._inp(a, "table", np.asarray(ctg_off, np.int64), 8) if ctg_off is not None else 0
    co = a.alloc("chain_offsets", (U + 1) * 8, 8)
    ch = a.alloc("chains", cap * 32, 16)
    names = ("anchor_chain", "anchor_pred", "anchor_score")
    an = [a.alloc(nm, R * 4, 4) if w else None for nm, w in zip(names, anchors)]
    tt = a.alloc("totals", 16, 8) if totals else None
    w, wb = CC._workspace(a, lib.genie_chain_mems_workspace_bytes(U, R, nc), None)
    rc_ = lib.genie_chain_mems(ix._h, CC._vp(pt), nc, CC._vp(po), CC._vp(pr), U, R, *[int(x) for x in prm], CC._vp(a.addr("chain_offsets")),
                               CC._vp(a.addr("chains")), cap, *[CC._vp(a.addr(nm) if w_ else 0) for nm, w_ in zip(names, anchors)],
                               CC._vp(a.addr("totals") if totals else 0), CC._vp(w), wb, CC._vp(s))

    def collect():
        off = as_numpy(co, np.int64)
        held = min(int(off[-1]), cap)
        res = {"offsets": off, "chains": as_numpy(ch, np.int32, (cap, 8))[:held]}
        assert a.holds_poison(ch[held * 32:]), "chains past the total were written"
        for nm, t in zip(names, an):
            if t is not None:
                res[nm] = as_numpy(t, np.int32)[:used]
                assert a.holds_poison(t[used * 4:]), nm + " past off[U] was written"
        if totals:
            res["totals"] = as_numpy(tt, np.int64)
        return res
    return CC.Call("chain_mems", rc_, collect, want_rc)
