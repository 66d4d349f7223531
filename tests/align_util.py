"""The specification of genie_align_chains restated in Python twice, int64 throughout, with nothing taken from the library under
test: (1) dp_loops, the three full matrices H / E / F by plain loops with a band mask, for tiny cases; (2) dp_band, banded and
vectorised per anti-diagonal in numpy, for everything else.  Both return H as a band: Hb[i, j - i - dlo].  The chain-level
function (trimming, gap fills, extensions) is built on either.  Also a generator of synthetic units and the raw ctypes calls
the GPU tests make, as tests/chain_util.py has them for genie_chain_mems.

s(x, y) = a if x == y and x <= 3 else -b.  For x[0 .. A), y[0 .. B) and diagonals d = j - i in [dlo, dhi], cells outside the
rectangle or the band are -infinity, H(0, 0) = 0, E(i, j) = max(H(i, j-1) - o - e, E(i, j-1) - e), F(i, j) = max(H(i-1, j) - o - e,
F(i-1, j) - e), H(i, j) = max(H(i-1, j-1) + s(x_i, y_j), E(i, j), F(i, j)).
Members of a chain: from row `last` along anchor_pred while anchor_chain names the chain.  Trimming from the last member
backwards, cur = (qs, ts): ov = max(0, s_j + l_j - qs, t_j + l_j - ts), l' = l_j - ov; l' <= 0: skipped; gap A = qs - (s_j + l'),
B = ts - (t_j + l'); |B - A| > max_indel: the chain is skipped (flags 4, every other column 0); else a l' + H(A, B) on the band
[min(0, B - A) - w, max(0, B - A) + w] is added and cur = (s_j, t_j).
Extension of x against y cut to A + w bases, band [-w, w]: M the largest H (smallest i + j, then smallest i); G the largest H
of row A (smallest j) if that row has a cell; G + end_bonus >= M: to the end, value G + end_bonus, consumes (A, j_G); else
local, M at (i*, j*).  Rows: (score, q_begin, q_end, r_begin, r_end, flags, n_used, matched)."""
import ctypes as C
from collections import namedtuple

import numpy as np

Params = namedtuple("Params", "match mismatch gap_open gap_extend band max_indel end_bonus")
DEFAULTS = Params(1, 4, 6, 1, 32, 64, 5)
INVALID, NO_DEVICE, CAPACITY, TOO_LONG = -1, -4, -10, -6
CHAIN_BYTES, UNIT_BYTES, FIXED_BYTES = 4, 0, 256      # the header's workspace figures
MAX_DIAGS = 1024
NEG = -(1 << 60)
BOTH, SPLIT = 1, 2


# ------------------------------------------------------------------ form (1): plain loops
def dp_loops(x, y, dlo, dhi, p):
    A, B = len(x), len(y)
    H = [[NEG] * (B + 1) for _ in range(A + 1)]
    E = [[NEG] * (B + 1) for _ in range(A + 1)]
    F = [[NEG] * (B + 1) for _ in range(A + 1)]
    for i in range(A + 1):
        for j in range(B + 1):
            if not dlo <= j - i <= dhi:
                continue
            if i == 0 and j == 0:
                H[0][0] = 0
                continue
            if j > 0:
                E[i][j] = max(NEG, H[i][j - 1] - p.gap_open - p.gap_extend, E[i][j - 1] - p.gap_extend)
            if i > 0:
                F[i][j] = max(NEG, H[i - 1][j] - p.gap_open - p.gap_extend, F[i - 1][j] - p.gap_extend)
            d = NEG
            if i > 0 and j > 0 and H[i - 1][j - 1] > NEG:
                d = H[i - 1][j - 1] + (p.match if x[i - 1] == y[j - 1] and x[i - 1] <= 3 else -p.mismatch)
            H[i][j] = max(d, E[i][j], F[i][j])
    Hb = np.full((A + 1, dhi - dlo + 1), NEG, np.int64)
    for i in range(A + 1):
        for j in range(max(0, i + dlo), min(B, i + dhi) + 1):
            Hb[i, j - i - dlo] = H[i][j]
    return Hb


# ------------------------------------------------------------------ form (2): banded, one anti-diagonal at a time
def dp_band(x, y, dlo, dhi, p):
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    A, B = x.size, y.size
    oe, e = p.gap_open + p.gap_extend, p.gap_extend
    Hb = np.full((A + 1, dhi - dlo + 1), NEG, np.int64)
    fresh = lambda: np.full(A + 2, NEG, np.int64)      # noqa: E731   index i + 1; [0] stands for i = -1
    h2, h1, e1, f1 = fresh(), fresh(), fresh(), fresh()
    low = NEG // 2
    for s in range(A + B + 1):
        ilo, ihi = max(0, s - B, -((dhi - s) // 2)), min(A, s, (s - dlo) // 2)
        hc, ec, fc = fresh(), fresh(), fresh()
        if ilo <= ihi:
            i = np.arange(ilo, ihi + 1)
            j = s - i
            if s == 0:
                hv, ev, fv = np.zeros(1, np.int64), np.full(1, NEG), np.full(1, NEG)
            else:
                ev = np.maximum(h1[i + 1] - oe, e1[i + 1] - e)                    # (i, j - 1) lies on s - 1 at the same i
                fv = np.maximum(h1[i] - oe, f1[i] - e)                            # (i - 1, j)
                sc = np.where((x[np.maximum(i - 1, 0)] == y[np.clip(j - 1, 0, max(B - 1, 0))]) & (x[np.maximum(i - 1, 0)] <= 3),
                              p.match, -p.mismatch) if A and B else np.zeros(i.size, np.int64)
                dv = np.where((i >= 1) & (j >= 1) & (h2[i] > low), h2[i] + sc, NEG)      # (i - 1, j - 1) lies on s - 2
                hv = np.maximum(dv, np.maximum(ev, fv))
            hv, ev, fv = (np.where(v < low, NEG, v) for v in (hv, ev, fv))
            hc[i + 1], ec[i + 1], fc[i + 1] = hv, ev, fv
            Hb[i, j - i - dlo] = hv
        h2, h1, e1, f1 = h1, hc, ec, fc
    return Hb


def gap_fill(x, y, p, dp=dp_band):
    """H(A, B) on the gap's band."""
    A, B = len(x), len(y)
    dlo, dhi = min(0, B - A) - p.band, max(0, B - A) + p.band
    return int(dp(x, y, dlo, dhi, p)[A, B - A - dlo])


def extension(x, y_all, p, dp=dp_band):
    """-> (value, i consumed, j consumed, to the end, ties): ties counts an arg-max attained more than once and a to-end
    decision with G + end_bonus == M."""
    A, w = len(x), p.band
    y = y_all[:A + w]
    Hb = dp(x, y, -w, w, p)
    ii, kk = np.nonzero(Hb > NEG // 2)
    jj, vals = ii + kk - w, Hb[ii, kk]
    M = int(vals.max())
    at = np.flatnonzero(vals == M)
    best = at[np.lexsort((ii[at], (ii + jj)[at]))[0]]
    row = np.flatnonzero(ii == A)
    if row.size:
        G = int(vals[row].max())
        top = row[vals[row] == G]
        if G + p.end_bonus >= M:
            return G + p.end_bonus, A, int(jj[top].min()), 1, int(top.size > 1) + int(G + p.end_bonus == M)
    return M, int(ii[best]), int(jj[best]), 0, int(at.size > 1)


def align_chain(Q, T, clo, chi, members, p, dp=dp_band):
    """members: (s, l, t) from the last one backwards -> (row of 8, ties)."""
    s, l, t = members[0]
    qs, ts, qe, te = s, t, s + l, t + l
    score, matched, used, ties = p.match * l, l, 1, 0
    for sj, lj, tj in members[1:]:
        lp = lj - max(0, sj + lj - qs, tj + lj - ts)
        if lp <= 0:
            continue
        A, B = qs - (sj + lp), ts - (tj + lp)
        assert A >= 0 and B >= 0
        if abs(B - A) > p.max_indel:
            return [0, 0, 0, 0, 0, 4, 0, 0], ties
        score += p.match * lp + gap_fill(Q[sj + lp:qs], T[tj + lp:ts], p, dp)
        matched, used, qs, ts = matched + lp, used + 1, sj, tj
    rv, ri, rj, rend, rt = extension(Q[qe:], T[te:chi], p, dp)
    lv, li, lj_, lend, lt = extension(Q[:qs][::-1], T[clo:ts][::-1], p, dp)
    return [score + rv + lv, qs - li, qe + ri, ts - lj_ + 1, te + rj + 1, lend | (rend << 1), used, matched], ties + rt + lt


def strand_read(bases, roff, S, u):
    i, s = divmod(u, S)
    q = np.asarray(bases[roff[i]:roff[i + 1]], np.int64)
    return np.where(q[::-1] <= 3, 3 - q[::-1], q[::-1]) if s else q


def members_of(rows, achain, apred, last, lc):
    """(s, l, t) of the chain `lc` of one unit, from row `last` backwards."""
    out, j = [], int(last)
    while True:
        out.append((int(rows[j, 0]), int(rows[j, 1] - rows[j, 0]), int(rows[j, 2]) - 1))
        pj = int(apred[j])
        if pj < 0 or pj >= j or achain[pj] != lc:
            return out
        j = pj


def expected(b, p, T, ctg_off=None, cap=None, dp=dp_band):
    """What the call returns for the batch `b` (a dict as synth_batch makes it) -> (aln int32 [C, 8], totals int64 [2], ties)."""
    S, coff = b["S"], b["chain_offsets"]
    C_ = int(coff[-1]) if cap is None else min(int(coff[-1]), cap)
    out, ties = np.zeros((C_, 8), np.int64), 0
    for u in range(coff.size - 1):
        lo, hi = int(b["offsets"][u]), int(b["offsets"][u + 1])
        Q = strand_read(b["bases"], b["read_offsets"], S, u)
        for c in range(int(coff[u]), min(int(coff[u + 1]), C_)):
            g = int(b["chains"][c, 6])
            clo, chi = (0, len(T)) if ctg_off is None else (int(ctg_off[g]), int(ctg_off[g + 1]))
            mem = members_of(b["rows"][lo:hi], b["anchor_chain"][lo:hi], b["anchor_pred"][lo:hi], b["chains"][c, 7], c - int(coff[u]))
            out[c], t = align_chain(Q, np.asarray(T, np.int64), clo, chi, mem, p, dp)
            ties += t
    skipped = int((out[:, 5] & 4).astype(bool).sum())
    return out.astype(np.int32), np.asarray([C_ - skipped, skipped], np.int64), ties


# ------------------------------------------------------------------ synthetic units
def mutate(rng, seq, rate):
    seq = np.array(seq, np.uint8)
    hit = rng.random(seq.size) < rate
    seq[hit] = (seq[hit] + rng.integers(1, 4, int(hit.sum()))) & 3
    return seq


def synth_chain(rng, T, t0, spec, left, right, rate=0.1):
    """One strand-read and one chain on it.  spec: [(l, A, B), ...] in read order: a member of l bases copied from the reference,
    then a gap of A query and B reference bases (those of the last entry are ignored).  left / right: the bases in front of the
    first and behind the last member, mutated copies of the reference where it has them.  -> (Q uint8, [(s, e, pos)])."""
    q, rows, t = [], [], t0
    lo = max(0, t0 - left)
    q.append(np.concatenate([rng.integers(0, 4, left - (t0 - lo)).astype(np.uint8), mutate(rng, T[lo:t0], rate)]))
    s = left
    for k, (l, A, B) in enumerate(spec):
        q.append(np.array(T[t:t + l], np.uint8))
        rows.append((s, s + l, t + 1))
        s, t = s + l, t + l
        if k + 1 < len(spec):
            m = min(A, B)
            q.append(np.concatenate([mutate(rng, T[t:t + m], rate), rng.integers(0, 4, A - m).astype(np.uint8)]))
            s, t = s + A, t + B
    tail = mutate(rng, T[t:t + right], rate)
    q.append(np.concatenate([tail, rng.integers(0, 4, right - tail.size).astype(np.uint8)]))
    return np.concatenate(q), rows


def revcomp(q):
    q = np.asarray(q, np.uint8)[::-1]
    return np.where(q <= 3, 3 - q, q).astype(np.uint8)


def make_batch(units, S=1):
    """units: per strand-read (Q as the strand reads it, [chain, ...]) with chain = ([(s, e, pos), ...] in read order, contig);
    with S == 2 units 2i and 2i + 1 are the strands of read i and unit 2i + 1's Q must be the reverse complement of unit 2i's
    (only unit 2i's is stored).  A unit's rows are its chains' members one chain after another; anchor_pred links a member to
    the one before, anchor_chain names the chain -> the batch dict the calls and `expected` take."""
    bases, roff, offs, rows, ac, ap, coff, chains = [], [0], [0], [], [], [], [0], []
    for u, (Q, chs) in enumerate(units):
        if S == 1 or u % 2 == 0:
            bases.append(np.asarray(Q, np.uint8))
            roff.append(roff[-1] + len(Q))
        n = 0
        for k, (mem, ctg) in enumerate(chs):
            for m, (s, e, pos) in enumerate(mem):
                rows.append((s, e, pos, -12345))
                ac.append(k)
                ap.append(n - 1 if m else -1)
                n += 1
            chains.append((mem[0][0], mem[-1][1], mem[0][2], mem[-1][2] + mem[-1][1] - mem[-1][0], 0, len(mem), ctg, n - 1))
        offs.append(offs[-1] + n)
        coff.append(coff[-1] + len(chs))
    arr = lambda v, t, w: np.asarray(v, t).reshape((-1,) + w)      # noqa: E731
    return {"S": S, "bases": np.concatenate(bases + [np.zeros(0, np.uint8)]), "read_offsets": arr(roff, np.int64, ()),
            "offsets": arr(offs, np.int64, ()), "rows": arr(rows, np.int32, (4,)), "anchor_chain": arr(ac, np.int32, ()),
            "anchor_pred": arr(ap, np.int32, ()), "chain_offsets": arr(coff, np.int64, ()), "chains": arr(chains, np.int32, (8,))}


# ------------------------------------------------------------------ the raw calls
def _p(t):
    return C.c_void_p(t.data_ptr() if t is not None and t.numel() else 0)


def call(lib, ix, b, p, ctg_off=None, cap=None, spare=0, totals=True, fill=-7, want_rc=0, flags=0):
    """One raw genie_align_chains on torch buffers of exactly the declared sizes (d_chains and d_aln: cap + spare rows, of which
    the call is told cap), the workspace exactly what its size function returns, d_aln filled with `fill` first -> (aln int32
    [cap + spare, 8], totals or None)."""
    import torch
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()      # noqa: E731
    U, R, total = b["offsets"].size - 1, b["rows"].shape[0], int(b["chain_offsets"][-1])
    cap = total if cap is None else cap
    N = b["read_offsets"].size - 1
    lens = np.diff(b["read_offsets"])
    bs, ro, of, co = dev(b["bases"]), dev(b["read_offsets"]), dev(b["offsets"]), dev(b["chain_offsets"])
    rw, ac, ap = dev(b["rows"]), dev(b["anchor_chain"]), dev(b["anchor_pred"])
    held = np.zeros((cap + spare, 8), np.int32)
    held[:min(total, cap + spare)] = b["chains"][:cap + spare]
    ch = dev(held)
    tab = dev(np.asarray(ctg_off, np.int64)) if ctg_off is not None else None
    nc = len(ctg_off) - 1 if ctg_off is not None else 0
    ws_bytes = lib.genie_align_chains_workspace_bytes(U, cap)
    assert ws_bytes >= 0 and ws_bytes % 256 == 0
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device="cuda")
    al = torch.full((max(cap + spare, 1), 8), fill, dtype=torch.int32, device="cuda")
    tt = torch.full((2,), fill, dtype=torch.int64, device="cuda") if totals else None
    rc_ = lib.genie_align_chains(ix._h, _p(tab), nc, flags | (BOTH if b["S"] == 2 else 0), _p(bs), _p(ro), N, int(b["bases"].size),
                                 int(lens.max()) if N else 0, _p(of), _p(rw), U, R, _p(ac), _p(ap), _p(co), _p(ch), cap,
                                 *[int(v) for v in p], _p(al), _p(tt), _p(ws), ws_bytes, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc_ == want_rc, rc_
    if rc_:
        return None
    return al.cpu().numpy()[:cap + spare], None if tt is None else tt.cpu().numpy()


def agrees(got, want, fill=-7):
    """(aln, totals) of a call equal the brute force's; rows behind the aligned ones still hold `fill`."""
    aln, totals = got
    C_ = want[0].shape[0]
    bad = np.flatnonzero((aln[:C_] != want[0]).any(1))
    assert bad.size == 0, (bad[:5], aln[bad[:5]], want[0][bad[:5]])
    assert (aln[C_:] == fill).all()
    if totals is not None:
        assert np.array_equal(totals, want[1]), (totals, want[1])


def guarded_call(lib, ix, a, s, b, p, ctg_off, cap, totals=True, want_rc=0, slack=0):
    """The call on the guarded buffers of tests/guarded.py, as tests/contract_calls.py makes the others: inputs frozen, d_aln,
    d_totals and the workspace cut from the arena `a` with exactly the declared bytes and the weakest alignment the header
    allows, ONE call on stream `s` without synchronising -> a contract_calls.Call.  slack: rows of d_rows and the anchor
    arrays past off[U], which the call has no business with."""
    import contract_calls as CC
    from guarded import as_numpy
    U, used, total = b["offsets"].size - 1, b["rows"].shape[0], max(0, int(b["chain_offsets"][-1]))
    R, N = used + slack, b["read_offsets"].size - 1
    pad = lambda v, w: np.concatenate([v, np.full((slack,) + w, 77, np.int32)])      # noqa: E731
    held = np.zeros((cap, 8), np.int32)
    held[:min(total, cap)] = b["chains"][:min(total, cap)]
    pb =CC._inp(a, "bases", b["bases"], 1) if b["bases"].size else 0
    pro, po, pco = (CC._inp(a, nm, b[nm], 8) for nm in ("read_offsets", "offsets", "chain_offsets"))
    pr = CC._inp(a, "rows", pad(b["rows"], (4,)), 16) if R else 0
    pac = CC._inp(a, "anchor_chain", pad(b["anchor_chain"], ()), 4) if R else 0
    pap = CC._inp(a, "anchor_pred", pad(b["anchor_pred"], ()), 4) if R else 0
    pch = CC._inp(a, "chains", held, 16) if cap else 0
    nc = len(ctg_off) - 1 if ctg_off is not None else 0
    pt = CC._inp(a, "table", np.asarray(ctg_off, np.int64), 8) if ctg_off is not None else 0
    al = a.alloc("aln", cap * 32, 16)
    tt = a.alloc("totals", 16, 8) if totals else None
    w, wb = CC._workspace(a, lib.genie_align_chains_workspace_bytes(U, cap), None)
    lens = np.diff(b["read_offsets"])
    rc_ = lib.genie_align_chains(ix._h, CC._vp(pt), nc, BOTH if b["S"] == 2 else 0, CC._vp(pb), CC._vp(pro), N, int(b["bases"].size),
                                 int(lens.max()) if N else 0, CC._vp(po), CC._vp(pr), U, R, CC._vp(pac), CC._vp(pap), CC._vp(pco),
                                 CC._vp(pch), cap, *[int(v) for v in p], CC._vp(a.addr("aln") if cap else 0),
                                 CC._vp(a.addr("totals") if totals else 0), CC._vp(w), wb, CC._vp(s))

    def collect():
        held_ = min(total, cap)
        res = {"aln": as_numpy(al, np.int32, (cap, 8))[:held_]}
        assert a.holds_poison(al[held_ * 32:]), "aln rows past the total were written"
        if totals:
            res["totals"] = as_numpy(tt, np.int64)
        return res
    return CC.Call("align_chains", rc_, collect, want_rc)
