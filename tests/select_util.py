"""The brute force of genie_select_alignments (include/genie_smem.h) in plain Python, in two forms -- the walk in key order,
straight from the definition, and the greedy rounds the kernels run -- with the raw ctypes call, the call on the guarded buffers
of tests/guarded.py, and the checks that hold whatever the tie-breaks.

A batch is a dict: read_offsets int64[N+1], S, chain_offsets int64[U+1], chains int32[T, 8] (only column 6 is read) and aln
int32[T, 8] = (score, q_begin, q_end, r_begin, r_end, flags, n_used, matched), T >= chain_offsets[U] or not: cap cuts it."""
import ctypes as C
from collections import namedtuple

import numpy as np

Params = namedtuple("SelParams", "mask_level pri_ratio max_secondary min_score mapq_full")
DEFAULTS = Params(50, 80, 5, 1, 40)
LANE_MAX, TILE = 8, 512                                  # GENIE_SELECT_LANE_MAX, GENIE_SELECT_TILE
CHAIN_BYTES, READ_BYTES, READ_SCAN_BYTES_PER_1024 = 4, 64, 8
BOTH = 1
INVALID, NO_DEVICE, CAPACITY, TOO_LONG = -1, -4, -10, -6
Cand = namedtuple("Cand", "chain score begin end matched")


def clamp(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


def forward(qb, qe, strand, L):
    b, e = (L - qe, L - qb) if strand else (qb, qe)
    return clamp(b, 0, L), clamp(e, 0, L)


def overlap(x, y, mask_level):
    ov = max(0, min(x.end, y.end) - max(x.begin, y.begin))
    return 100 * ov > mask_level * min(x.end - x.begin, y.end - y.begin)


def mapq(score, sub, matched, full):
    return 60 * (score - min(sub, score)) * clamp(matched, 0, full) // (score * full)


def key(c):
    return (-c.score, c.chain)


def walk(cands, p):
    """The definition: the candidates in key order -> {chain: (kind, parent)}, primaries in key order."""
    out, prim = {}, []
    for c in sorted(cands, key=key):
        parent = next((q for q in prim if overlap(c, q, p.mask_level)), None)
        if parent is None:
            out[c.chain] = (1 if prim else 0, c.chain)
            prim.append(c)
        else:
            out[c.chain] = (2, parent.chain)
    return out, prim


def greedy(cands, p):
    """The rounds: the best unassigned candidate becomes a primary and takes every unassigned candidate that overlaps it."""
    out, prim, left = {}, [], list(cands)
    while left:
        top = min(left, key=key)
        out[top.chain] = (1 if prim else 0, top.chain)
        prim.append(top)
        rest = []
        for c in left:
            if c is top:
                continue
            if overlap(c, top, p.mask_level):
                out[c.chain] = (2, top.chain)
            else:
                rest.append(c)
        left = rest
    return out, prim


def select_read(cands, p, classify=walk):
    """-> (rows {chain: [kind, parent, order, mapq]}, sub {primary: sub}, the selection as a list of chains, secondaries)."""
    kinds, prim = classify(cands, p)
    by = {c.chain: c for c in cands}
    secs = sorted((c for c in cands if kinds[c.chain][0] == 2), key=key)
    sub = {q.chain: max([c.score for c in secs if kinds[c.chain][1] == q.chain], default=0) for q in prim}
    rows = {c.chain: [kinds[c.chain][0], kinds[c.chain][1], -1, 0] for c in cands}
    sel = [q.chain for q in prim]
    for q in prim:
        rows[q.chain][3] = mapq(q.score, sub[q.chain], q.matched, p.mapq_full)
    if classify is walk:
        eligible = [c for c in secs if 100 * c.score >= p.pri_ratio * by[kinds[c.chain][1]].score]
        sel += [c.chain for c in eligible[:p.max_secondary]]
    else:                                                            # arg-max rounds over the eligible ones
        pending = [c for c in secs if 100 * c.score >= p.pri_ratio * by[kinds[c.chain][1]].score]
        for _ in range(min(p.max_secondary, len(pending))):
            top = min(pending, key=key)
            pending.remove(top)
            sel.append(top.chain)
    for k, c in enumerate(sel):
        rows[c][2] = k
    return rows, sub, sel, len(secs)


def read_chains(b, i, C_):
    """(lo, mid, hi) of read i: its chains below C_, those from mid on on strand 1."""
    S, co = b["S"], b["chain_offsets"]
    lo, hi = min(int(co[S * i]), C_), min(int(co[S * i + S]), C_)
    return lo, (min(int(co[2 * i + 1]), C_) if S == 2 else hi), hi


def candidates(b, i, C_, p):
    lo, mid, hi = read_chains(b, i, C_)
    L = int(b["read_offsets"][i + 1] - b["read_offsets"][i])
    out = []
    for c in range(lo, hi):
        a = [int(v) for v in b["aln"][c]]
        if (a[5] & 4) == 0 and a[0] >= p.min_score:
            fb, fe = forward(a[1], a[2], c >= mid, L)
            out.append(Cand(c, a[0], fb, fe, a[7]))
    return out


def expected(b, p, table=None, cap=None, cap_sel=None, classify=walk):
    """Every output of the call; cap_sel None: room for all (the sizing call's outputs are those without sel and records)."""
    N = b["read_offsets"].size - 1
    total = int(b["chain_offsets"][-1])
    C_ = min(total, total if cap is None else cap)
    klass = np.zeros((C_, 4), np.int32)
    klass[:] = (3, -1, -1, 0)
    counts = np.zeros((N, 4), np.int32)
    offsets = np.zeros(N + 1, np.int64)
    sel, records = [], []
    for i in range(N):
        lo, mid, hi = read_chains(b, i, C_)
        cands = candidates(b, i, C_, p)
        rows, sub, chosen, nsec = select_read(cands, p, classify)
        for c, row in rows.items():
            klass[c] = row
        nprim = len(sub)
        counts[i] = (len(cands), nprim, nsec, chosen[0] if chosen else -1)
        offsets[i + 1] = offsets[i] + len(chosen)
        L = int(b["read_offsets"][i + 1] - b["read_offsets"][i])
        for c in chosen:
            a = [int(v) for v in b["aln"][c]]
            fb, fe = forward(a[1], a[2], c >= mid, L)
            g, off = 0, a[3]
            if table is not None:
                g = clamp(int(b["chains"][c, 6]), 0, len(table) - 2)
                off = a[3] - int(table[g])
            kind = rows[c][0]
            sel.append(c)
            records.append((i, c, kind, int(c >= mid), g, off, a[4] - a[3], fb, fe, a[0], sub[c] if kind < 2 else 0, rows[c][3]))
    got = len(sel) if cap_sel is None else min(len(sel), cap_sel)
    return {"klass": klass, "offsets": offsets, "sel": np.asarray(sel[:got], np.int64),
            "records": np.asarray(records[:got], np.int32).reshape(got, 12), "counts": counts,
            "totals": np.asarray([counts[:, 0].sum(), counts[:, 1].sum(), counts[:, 2].sum(), len(sel)], np.int64)}


def agrees(got, want, keys=None):
    for k in keys or want:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (k, got[k][:12], want[k][:12])


def check_result(b, p, res, cap=None):
    """What holds whatever the tie-breaks: every primary overlaps no earlier primary; every secondary overlaps its parent and
    no primary before it; the offsets are consistent with the counts; order is the inverse of sel; mapq lies in [0, 60]."""
    N = b["read_offsets"].size - 1
    total = int(b["chain_offsets"][-1])
    C_ = min(total, total if cap is None else cap)
    klass, off, sel, counts = res["klass"], res["offsets"], res["sel"], res["counts"]
    assert klass.shape == (C_, 4) and off[0] == 0 and (np.diff(off) >= 0).all()
    assert ((klass[:, 3] >= 0) & (klass[:, 3] <= 60)).all() and not klass[klass[:, 0] >= 2, 3].any()
    assert res["totals"][3] == off[N] and np.array_equal(res["totals"][:3], counts[:, :3].sum(0))
    full = sel.size == off[N]
    for i in range(N):
        lo, mid, hi = read_chains(b, i, C_)
        by = {c.chain: c for c in candidates(b, i, C_, p)}
        kinds = klass[lo:hi, 0]
        assert np.array_equal(kinds != 3, np.asarray([c in by for c in range(lo, hi)], bool).reshape(kinds.shape))
        prim = sorted((by[c] for c in by if klass[c, 0] < 2), key=key)
        assert counts[i, 0] == len(by) and counts[i, 1] == len(prim) and counts[i, 2] == len(by) - len(prim)
        assert counts[i, 3] == (prim[0].chain if prim else -1) and [klass[q.chain, 0] for q in prim] == [min(k, 1) for k in range(len(prim))]
        for k, q in enumerate(prim):
            assert klass[q.chain, 1] == q.chain and klass[q.chain, 2] == k
            assert not any(overlap(q, e, p.mask_level) for e in prim[:k])
        for c, x in by.items():
            if klass[c, 0] == 2:
                parent = by[int(klass[c, 1])]
                assert klass[parent.chain, 0] < 2 and key(parent) < key(x) and overlap(x, parent, p.mask_level)
                assert not any(overlap(x, e, p.mask_level) for e in prim if key(e) < key(parent))
        chosen = sorted((c for c in range(lo, hi) if klass[c, 2] >= 0), key=lambda c: klass[c, 2])
        assert off[i + 1] - off[i] == len(chosen) and [int(klass[c, 2]) for c in chosen] == list(range(len(chosen)))
        assert len(chosen) - len(prim) <= p.max_secondary
        if full:
            assert [int(v) for v in sel[off[i]:off[i + 1]]] == chosen


# ------------------------------------------------------------------ batches
def make_batch(lengths, units, S):
    """lengths: the reads'; units: per strand-read a list of (score, q_begin, q_end, r_begin, r_end, flags, matched, contig)."""
    assert len(units) == S * len(lengths)
    ro = np.zeros(len(lengths) + 1, np.int64)
    ro[1:] = np.cumsum(lengths)
    co = np.zeros(len(units) + 1, np.int64)
    co[1:] = np.cumsum([len(u) for u in units])
    T = int(co[-1])
    aln, chains = np.zeros((T, 8), np.int32), np.zeros((T, 8), np.int32)
    flat = [r for u in units for r in u]
    if flat:
        f = np.asarray(flat, np.int64)
        aln[:, :6] = f[:, :6]
        aln[:, 6] = 1
        aln[:, 7] = f[:, 6]
        chains[:, 6] = f[:, 7]
        chains[:, :4] = f[:, 1:5]
    return {"read_offsets": ro, "S": S, "chain_offsets": co, "chains": chains, "aln": aln}


def random_batch(rng, counts, S=1, L=(50, 200), scores=(20, 26), n_ref=16000, skipped=0.0, contigs=1):
    """One read per entry of counts: that many chains, split at random between its strand-reads; intervals of every length all
    over the read, scores from a small range so that ties are common, a share `skipped` of the rows with flag bit 4."""
    counts = np.asarray(counts, np.int64)
    N, T = counts.size, int(counts.sum())
    lengths = rng.integers(L[0], L[1], N)
    per_unit = counts
    if S == 2:
        first = (rng.random(N) * (counts + 1)).astype(np.int64)
        per_unit = np.stack([first, counts - first], 1).reshape(-1)
    ro, co = np.zeros(N + 1, np.int64), np.zeros(S * N + 1, np.int64)
    ro[1:], co[1:] = np.cumsum(lengths), np.cumsum(per_unit)
    Lc = np.repeat(lengths, counts)
    qb = (rng.random(T) * Lc).astype(np.int64)
    qe = qb + (rng.random(T) * (Lc - qb + 1)).astype(np.int64)
    rb = rng.integers(1, n_ref - L[1], T)
    aln, chains = np.zeros((T, 8), np.int32), np.zeros((T, 8), np.int32)
    aln[:, 0], aln[:, 1], aln[:, 2], aln[:, 3], aln[:, 4] = rng.integers(scores[0], scores[1], T), qb, qe, rb, rb + qe - qb
    aln[:, 5] = np.where(rng.random(T) < skipped, 4, rng.integers(0, 4, T))
    aln[:, 6], aln[:, 7] = 1, (rng.random(T) * (qe - qb + 1)).astype(np.int64)
    chains[:, 6] = rng.integers(0, contigs, T)
    return {"read_offsets": ro, "S": S, "chain_offsets": co, "chains": chains, "aln": aln}


# ------------------------------------------------------------------ the call
def _vp(t):
    return C.c_void_p(t.data_ptr() if t is not None and t.numel() else 0)


def call(lib, ix, b, p, table=None, cap=None, cap_sel=None, sizing=False, extras=True, want_rc=0):
    """The raw call on torch tensors of the current device -> the outputs as numpy arrays, as expected() returns them.
    sizing: d_sel and d_records NULL; cap_sel None: first the sizing call, then room for all."""
    import torch
    dev = "cuda"
    N, U = b["read_offsets"].size - 1, b["chain_offsets"].size - 1
    total = int(b["chain_offsets"][-1])
    cap = total if cap is None else cap
    C_ = min(total, cap)
    held_c, held_a = np.zeros((max(cap, 1), 8), np.int32), np.zeros((max(cap, 1), 8), np.int32)
    held_c[:C_], held_a[:C_] = b["chains"][:C_], b["aln"][:C_]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    ro, co, ch, al = t(b["read_offsets"]), t(b["chain_offsets"]), t(held_c), t(held_a)
    tab = t(np.asarray(table, np.int64)) if table is not None else None
    klass = torch.full((max(cap, 1), 4), -77, dtype=torch.int32, device=dev)
    off = torch.full((N + 1,), -77, dtype=torch.int64, device=dev)
    counts = torch.full((max(N, 1), 4), -77, dtype=torch.int32, device=dev) if extras else None
    totals = torch.full((4,), -77, dtype=torch.int64, device=dev) if extras else None
    wsb = lib.genie_select_alignments_workspace_bytes(N, cap)
    ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device=dev)
    assert ws.data_ptr() % 256 == 0
    prm = [int(v) for v in p]
    nul = C.c_void_p(0)

    def run(sel, rec, n):
        rc = lib.genie_select_alignments(ix._h, _vp(tab), len(table) - 1 if table is not None else 0, BOTH if b["S"] == 2 else 0,
                                         C.c_void_p(ro.data_ptr()), N, C.c_void_p(co.data_ptr()), U, C.c_void_p(ch.data_ptr()) if cap else nul,
                                         C.c_void_p(al.data_ptr()) if cap else nul, cap, *prm, C.c_void_p(klass.data_ptr()) if cap else nul,
                                         C.c_void_p(off.data_ptr()), C.c_void_p(sel.data_ptr()) if sel is not None else nul,
                                         C.c_void_p(rec.data_ptr()) if rec is not None else nul, n, _vp(counts), _vp(totals),
                                         C.c_void_p(ws.data_ptr()), wsb, nul)
        torch.cuda.synchronize()
        assert rc == want_rc, rc
    if want_rc:
        run(None, None, 0)
        return None
    if cap_sel is None and not sizing:
        run(None, None, 0)
        cap_sel = int(off[N].item())
    sel = rec = None
    if not sizing:
        sel = torch.full((cap_sel + 3,), -77, dtype=torch.int64, device=dev)
        rec = torch.full((cap_sel + 3, 12), -77, dtype=torch.int32, device=dev)
    run(sel, rec, 0 if sizing else cap_sel)
    res = {"klass": klass[:C_].cpu().numpy(), "offsets": off.cpu().numpy()}
    assert (klass[C_:] == -77).all(), "rows at or past C were written"
    if not sizing:
        got = min(int(res["offsets"][N]), cap_sel)
        assert (sel[got:] == -77).all() and (rec[got:] == -77).all(), "entries past the total or past cap_sel were written"
        res["sel"], res["records"] = sel[:got].cpu().numpy(), rec[:got].cpu().numpy()
    if extras:
        res["counts"], res["totals"] = counts[:N].cpu().numpy().reshape(N, 4), totals.cpu().numpy()
    return res


def guarded_call(lib, ix, a, s, b, p, table, cap, cap_sel, sizing=False, extras=True, want_rc=0):
    """The call on the guarded buffers of tests/guarded.py: inputs frozen, every output and the workspace cut from the arena
    `a` with exactly the declared bytes and the weakest alignment the header allows, ONE call on stream `s` without
    synchronising -> a contract_calls.Call."""
    import contract_calls as CC
    from guarded import as_numpy
    N, U = b["read_offsets"].size - 1, b["chain_offsets"].size - 1
    total = max(0, int(b["chain_offsets"][-1]))
    C_ = min(total, cap)
    held_c, held_a = np.zeros((cap, 8), np.int32), np.zeros((cap, 8), np.int32)
    held_c[:C_], held_a[:C_] = b["chains"][:C_], b["aln"][:C_]
    pro, pco = CC._inp(a, "read_offsets", b["read_offsets"], 8), CC._inp(a, "chain_offsets", b["chain_offsets"], 8)
    pch = CC._inp(a, "chains", held_c, 16) if cap else 0
    pal = CC._inp(a, "aln", held_a, 16) if cap else 0
    pt = CC._inp(a, "table", np.asarray(table, np.int64), 8) if table is not None else 0
    klass = a.alloc("class", cap * 16, 16) if cap else None
    off = a.alloc("sel_offsets", (N + 1) * 8, 8)
    sel = a.alloc("sel", cap_sel * 8, 8) if not sizing and cap_sel else None
    rec = a.alloc("records", cap_sel * 48, 16) if not sizing and cap_sel else None
    counts = a.alloc("read_counts", N * 16, 16) if extras and N else None
    tt = a.alloc("totals", 32, 8) if extras else None
    w, wb = CC._workspace(a, lib.genie_select_alignments_workspace_bytes(N, cap), None)
    adr = lambda t_, name, empty=0: CC._vp(a.addr(name) if t_ is not None else empty)      # noqa: E731
    given = not sizing
    rc_ = lib.genie_select_alignments(ix._h, CC._vp(pt), len(table) - 1 if table is not None else 0, BOTH if b["S"] == 2 else 0,
                                      CC._vp(pro), N, CC._vp(pco), U, CC._vp(pch), CC._vp(pal), cap, *[int(v) for v in p],
                                      adr(klass, "class"), adr(off, "sel_offsets"), adr(sel, "sel", 8 if given else 0),
                                      adr(rec, "records", 16 if given else 0), 0 if sizing else cap_sel, adr(counts, "read_counts"),
                                      adr(tt, "totals"), CC._vp(w), wb, CC._vp(s))

    def collect():
        res = {"klass": as_numpy(klass, np.int32, (cap, 4))[:C_] if cap else np.zeros((0, 4), np.int32), "offsets": as_numpy(off, np.int64)}
        if cap:
            assert a.holds_poison(klass[C_ * 16:]), "rows at or past C were written"
        n = int(res["offsets"][N])
        assert 0 <= n and (np.diff(res["offsets"]) >= 0).all()
        if sel is not None:
            got = min(n, cap_sel)
            res["sel"], res["records"] = as_numpy(sel, np.int64)[:got], as_numpy(rec, np.int32, (cap_sel, 12))[:got]
            assert a.holds_poison(sel[got * 8:]) and a.holds_poison(rec[got * 48:]), "entries past the total were written"
        if extras:
            res["counts"] = as_numpy(counts, np.int32, (N, 4)) if N else np.zeros((0, 4), np.int32)
            res["totals"] = as_numpy(tt, np.int64)
        return res
    return CC.Call("select_alignments", rc_, collect, want_rc)
