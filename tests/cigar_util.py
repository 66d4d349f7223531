"""The specification of genie_chain_cigars restated in Python, int64 throughout, with nothing taken from the library under test.
Members, trimming and the programs are those of tests/align_util.py; this adds the three full matrices H / E / F twice -- (1)
hef_loops, plain loops, for tiny cases; (2) hef_band, one anti-diagonal at a time in numpy, for everything else --, the
canonical trace on them, the merging of ops, `info`, the direction need, the checks that hold whatever the tie-breaks, and the
raw ctypes calls the GPU tests make.

The canonical path, from the piece's end cell backwards.  State H at (i, j): stop at (0, 0); else the first that holds: i, j >= 1,
(i-1, j-1) inside band and rectangle and H(i, j) == H(i-1, j-1) + s(x_i, y_j): '=' on a match (x_i == y_j <= 3) else 'X', to H at
(i-1, j-1); H(i, j) == F(i, j): state F; else state E.  State F: 'I', move to (i-1, j), stay iff F(i, j) == F(i-1, j) - e of the cell
before the move.  State E: 'D', move to (i, j-1), stay iff E(i, j) == E(i, j-1) - e.
Ops: len << 4 | op, I = 1, D = 2, S = 4, '=' = 7, X = 8.  info: (chain, flags, n_ops, nm, n_eq, n_x, ins_bases, del_bases); flags 4:
skipped by genie_align_chains, 8: no room for the directions, 16: bad index or end cell."""
import ctypes as C

import numpy as np

import align_util as AU

NEG = AU.NEG
LOW = NEG // 2
OP_I, OP_D, OP_S, OP_EQ, OP_X = 1, 2, 4, 7, 8
LETTER = {OP_I: "I", OP_D: "D", OP_S: "S", OP_EQ: "=", OP_X: "X"}
SKIPPED, NO_ROOM, BAD = 4, 8, 16
POISON = -0x543210FF
CHAIN_BYTES, SEL_BYTES, SEL_SCAN_BYTES_PER_1024, UNIT_BYTES = 4, 20, 8, 0      # the header's workspace figures


def score_of(x, y, p):
    return p.match if x == y and x <= 3 else -p.mismatch


# ------------------------------------------------------------------ form (1): plain loops
def hef_loops(x, y, dlo, dhi, p):
    A, B = len(x), len(y)
    H, E, F = (np.full((A + 1, B + 1), NEG, np.int64) for _ in range(3))
    for i in range(A + 1):
        for j in range(B + 1):
            if not dlo <= j - i <= dhi:
                continue
            if i == 0 and j == 0:
                H[0, 0] = 0
                continue
            if j > 0:
                E[i, j] = max(NEG, H[i, j - 1] - p.gap_open - p.gap_extend, E[i, j - 1] - p.gap_extend)
            if i > 0:
                F[i, j] = max(NEG, H[i - 1, j] - p.gap_open - p.gap_extend, F[i - 1, j] - p.gap_extend)
            d = NEG
            if i > 0 and j > 0 and H[i - 1, j - 1] > LOW:
                d = H[i - 1, j - 1] + score_of(x[i - 1], y[j - 1], p)
            H[i, j] = max(d, E[i, j], F[i, j])
    for M in (H, E, F):
        M[M < LOW] = NEG
    return H, E, F


# ------------------------------------------------------------------ form (2): one anti-diagonal at a time
def hef_band(x, y, dlo, dhi, p):
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    A, B = x.size, y.size
    oe, e = p.gap_open + p.gap_extend, p.gap_extend
    H, E, F = (np.full((A + 2, B + 2), NEG, np.int64) for _ in range(3))      # index (i + 1, j + 1): row and column 0 are -infinity
    for s in range(A + B + 1):
        ilo, ihi = max(0, s - B, -((dhi - s) // 2)), min(A, s, (s - dlo) // 2)
        if ilo > ihi:
            continue
        i = np.arange(ilo, ihi + 1)
        j = s - i
        if s == 0:
            H[1, 1] = 0
            continue
        ev = np.maximum(H[i + 1, j] - oe, E[i + 1, j] - e)
        fv = np.maximum(H[i, j + 1] - oe, F[i, j + 1] - e)
        xi, yj = x[np.maximum(i - 1, 0)] if A else np.zeros_like(i), y[np.clip(j - 1, 0, max(B - 1, 0))] if B else np.zeros_like(i)
        sc = np.where((xi == yj) & (xi <= 3), p.match, -p.mismatch)
        dv = np.where((i >= 1) & (j >= 1) & (H[i, j] > LOW), H[i, j] + sc, NEG)
        hv = np.maximum(dv, np.maximum(ev, fv))
        H[i + 1, j + 1], E[i + 1, j + 1], F[i + 1, j + 1] = (np.where(v < LOW, NEG, v) for v in (hv, ev, fv))
    return H[1:, 1:].copy(), E[1:, 1:].copy(), F[1:, 1:].copy()


# ------------------------------------------------------------------ the canonical trace
def trace(x, y, dlo, dhi, p, hef=hef_band):
    """The ops of the canonical path from (A, B) back to (0, 0), in forward order, one letter per base."""
    A, B = len(x), len(y)
    if A == 0 or B == 0:
        return ("I" if A else "D") * (A + B)
    H, E, F = hef(x, y, dlo, dhi, p)
    assert H[A, B] > LOW, "the end cell is not reachable"
    i, j, state, out = A, B, "H", []
    e = p.gap_extend
    while True:
        assert H[i, j] > LOW and len(out) <= A + B
        if state == "H":
            if i == 0 and j == 0:
                break
            if i >= 1 and j >= 1 and dlo <= j - i <= dhi and H[i - 1, j - 1] > LOW and \
                    H[i, j] == H[i - 1, j - 1] + score_of(x[i - 1], y[j - 1], p):
                out.append("=" if x[i - 1] == y[j - 1] and x[i - 1] <= 3 else "X")
                i, j = i - 1, j - 1
            elif H[i, j] == F[i, j]:
                state = "F"
            else:
                assert H[i, j] == E[i, j]
                state = "E"
        elif state == "F":
            out.append("I")
            state = "F" if i >= 2 and F[i - 1, j] > LOW and F[i, j] == F[i - 1, j] - e else "H"
            i -= 1
        else:
            out.append("D")
            state = "E" if j >= 2 and E[i, j - 1] > LOW and E[i, j] == E[i, j - 1] - e else "H"
            j -= 1
    return "".join(out[::-1])


def merge(letters):
    """One letter per base -> [(op, len)] with neighbouring equal ops merged."""
    code = {v: k for k, v in LETTER.items()}
    out = []
    for ch in letters:
        if out and out[-1][0] == code[ch]:
            out[-1][1] += 1
        else:
            out.append([code[ch], 1])
    return [(o, n) for o, n in out]


def piece_bytes(A, B, D):
    return 0 if A <= 0 or B <= 0 else A * ((min(D, AU.MAX_DIAGS) + 63) // 64) * 32


def chain_cigar(Q, T, clo, chi, members, p, row, hef=hef_band):
    """members: (s, l, t) from the last one backwards; row: the chain's d_aln row -> (flags, ops [(op, len)], direction need)."""
    Q, T = np.asarray(Q, np.int64), np.asarray(T, np.int64)
    L, w = len(Q), p.band
    if row[5] & 4:
        return SKIPPED, [], 0
    s, l, t = members[0]
    qs, ts, qe, te = s, t, s + l, t + l
    mid, need = "=" * l, 0                                           # from the first used member to the end of the last
    for sj, lj, tj in members[1:]:
        lp = lj - max(0, sj + lj - qs, tj + lj - ts)
        if lp <= 0:
            continue
        A, B = qs - (sj + lp), ts - (tj + lp)
        if abs(B - A) > p.max_indel:
            return SKIPPED, [], 0
        dlo, dhi = min(0, B - A) - w, max(0, B - A) + w
        mid = "=" * lp + trace(Q[sj + lp:qs], T[tj + lp:ts], dlo, dhi, p, hef) + mid
        need += piece_bytes(A, B, dhi - dlo + 1)
        qs, ts = sj, tj
    q_begin, q_end, r_begin, r_end = (int(v) for v in row[1:5])
    ri, rj = q_end - qe, (r_end - 1) - te
    li, lj_ = qs - q_begin, ts - (r_begin - 1)
    for i, j, A, avail in ((ri, rj, L - qe, chi - te), (li, lj_, qs, ts - clo)):
        B = min(max(avail, 0), A + w)
        if not (0 <= i <= A and 0 <= j <= B and abs(j - i) <= w and (i > 0 or j == 0)):
            return BAD, [], 0
    right = trace(Q[qe:qe + ri], T[te:te + rj], -w, w, p, hef)
    left = trace(Q[qs - li:qs][::-1], T[ts - lj_:ts][::-1], -w, w, p, hef)      # on the reversed strings: emitted backwards is forwards
    need += piece_bytes(ri, rj, 2 * w + 1) + piece_bytes(li, lj_, 2 * w + 1)
    letters = "S" * q_begin + left[::-1] + mid + right + "S" * (L - q_end)
    return 0, merge(letters), need


def info_row(chain, flags, ops):
    if flags:
        return [chain, flags, 0, 0, 0, 0, 0, 0]
    n = {o: sum(ln for op, ln in ops if op == o) for o in LETTER}
    return [chain, 0, len(ops), n[OP_X] + n[OP_I] + n[OP_D], n[OP_EQ], n[OP_X], n[OP_I], n[OP_D]]


def expected(b, p, T, aln, ctg_off=None, sel=None, cap=None, cap_ops=None, dir_bytes=None, hef=hef_band):
    """What the call returns for the batch `b`, the rows `aln` of genie_align_chains and the selection -> dict(offsets int64
    [n + 1], cigar uint32 [min(total, cap_ops)], info int32 [n, 8], need int64 [n], totals int64 [3])."""
    S, coff = b["S"], b["chain_offsets"]
    C_ = int(coff[-1]) if cap is None else min(int(coff[-1]), cap)
    sel = list(range(C_)) if sel is None else [int(c) for c in sel]
    units = np.searchsorted(coff, np.arange(C_), side="right") - 1
    memo, rows, ops_all, needs, run = {}, [], [], [], 0
    for c in sel:
        if not 0 <= c < C_:
            got = (BAD, [], 0)
        else:
            if c not in memo:
                u = int(units[c])
                lo, hi = int(b["offsets"][u]), int(b["offsets"][u + 1])
                Q = AU.strand_read(b["bases"], b["read_offsets"], S, u)
                g = int(b["chains"][c, 6])
                clo, chi = (0, len(T)) if ctg_off is None else (int(ctg_off[g]), int(ctg_off[g + 1]))
                mem = AU.members_of(b["rows"][lo:hi], b["anchor_chain"][lo:hi], b["anchor_pred"][lo:hi], b["chains"][c, 7], c - int(coff[u]))
                memo[c] = chain_cigar(Q, T, clo, chi, mem, p, aln[c], hef)
            got = memo[c]
        flags, ops, need = got
        run += need
        if dir_bytes is not None and run > dir_bytes:
            flags, ops = flags | NO_ROOM, []
        needs.append(need)
        rows.append(info_row(int(np.int64(c).astype(np.int32)), flags, ops))
        ops_all.append(ops)
    offsets = np.zeros(len(sel) + 1, np.int64)
    offsets[1:] = np.cumsum([len(o) for o in ops_all]) if sel else []
    cigar = np.asarray([(ln << 4) | op for ops in ops_all for op, ln in ops], np.uint32)
    flagged = sum(1 for r in rows if r[1])
    return {"offsets": offsets, "cigar": cigar if cap_ops is None else cigar[:cap_ops],
            "info": np.asarray(rows, np.int32).reshape(-1, 8), "need": np.asarray(needs, np.int64),
            "totals": np.asarray([len(sel) - flagged, flagged, sum(needs)], np.int64)}


# ------------------------------------------------------------------ checks that hold whatever the tie-breaks
def cigar_strings(offsets, cigar):
    return ["".join(f"{int(v) >> 4}{LETTER[int(v) & 15]}" for v in cigar[offsets[k]:offsets[k + 1]]) for k in range(len(offsets) - 1)]


def check_chain(Q, T, row, ops, p):
    """The ops [(op, len)] of an unflagged chain against its strand-read Q, the reference T and its d_aln row."""
    Q, T = np.asarray(Q, np.int64), np.asarray(T, np.int64)
    L = len(Q)
    score, q_begin, q_end, r_begin, r_end, flags = (int(v) for v in row[:6])
    assert all(ln > 0 for _, ln in ops) and all(a[0] != b_[0] for a, b_ in zip(ops, ops[1:])), ops
    assert all(op != OP_S or k in (0, len(ops) - 1) for k, (op, _) in enumerate(ops)), ops
    lead = ops[0][1] if ops and ops[0][0] == OP_S else 0
    tail = ops[-1][1] if len(ops) > 1 and ops[-1][0] == OP_S else 0
    assert lead == q_begin and tail == L - q_end, (ops, row)
    q, t, total = 0, r_begin - 1, 0
    for op, ln in ops:
        if op == OP_S:
            q += ln
        elif op == OP_EQ:
            assert np.array_equal(Q[q:q + ln], T[t:t + ln]) and (Q[q:q + ln] <= 3).all(), (q, t, ln)
            q, t, total = q + ln, t + ln, total + p.match * ln
        elif op == OP_X:
            assert ((Q[q:q + ln] != T[t:t + ln]) | (Q[q:q + ln] > 3)).all() and len(T[t:t + ln]) == ln, (q, t, ln)
            q, t, total = q + ln, t + ln, total - p.mismatch * ln
        elif op == OP_I:
            q, total = q + ln, total - p.gap_open - p.gap_extend * ln
        else:
            assert op == OP_D
            t, total = t + ln, total - p.gap_open - p.gap_extend * ln
    assert q == L and q - tail == q_end and t == r_end - 1, (q, t, row)
    total += p.end_bonus * (bool(flags & 1) + bool(flags & 2))
    assert total == score, (total, score, ops)


def check_result(b, p, T, aln, res, sel=None):
    """check_chain on every unflagged chain of a result (a dict as `expected` makes it)."""
    S, coff = b["S"], b["chain_offsets"]
    units = np.searchsorted(coff, np.arange(int(coff[-1])), side="right") - 1
    n = 0
    for k, inf in enumerate(res["info"]):
        if inf[1]:
            assert not inf[2:].any() and res["offsets"][k] == res["offsets"][k + 1]
            continue
        c = int(inf[0])
        assert sel is None or c == int(sel[k])
        ops = [(int(v) & 15, int(v) >> 4) for v in res["cigar"][res["offsets"][k]:res["offsets"][k + 1]]]
        assert inf.tolist() == info_row(c, 0, ops)
        check_chain(AU.strand_read(b["bases"], b["read_offsets"], S, int(units[c])), T, aln[c], ops, p)
        n += 1
    return n


# ------------------------------------------------------------------ the raw call
def _p(t):
    return C.c_void_p(t.data_ptr() if t is not None and t.numel() else 0)


def call(lib, ix, b, p, aln, ctg_off=None, sel=None, cap=None, cap_ops=None, dir_bytes=None, fill=-7, want_rc=0, sizing=False):
    """One raw genie_chain_cigars on torch buffers of exactly the declared sizes plus a spare tail that must keep `fill`, the
    workspace exactly what its size function returns.  cap_ops None: a sizing call first, then room for all; dir_bytes None: a
    call with 0 first, then the needed bytes -> a dict as `expected` makes it."""
    import torch
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()      # noqa: E731
    U, R, total = b["offsets"].size - 1, b["rows"].shape[0], int(b["chain_offsets"][-1])
    cap = total if cap is None else cap
    C_ = min(total, cap)
    N = b["read_offsets"].size - 1
    lens = np.diff(b["read_offsets"])
    bs, ro, of, co = dev(b["bases"]), dev(b["read_offsets"]), dev(b["offsets"]), dev(b["chain_offsets"])
    rw, ac, ap = dev(b["rows"]), dev(b["anchor_chain"]), dev(b["anchor_pred"])
    held = np.zeros((max(cap, 1), 8), np.int32)
    held[:C_] = b["chains"][:C_]
    ch = dev(held)
    al_np = np.zeros((max(cap, 1), 8), np.int32)
    al_np[:C_] = aln[:C_]
    al = dev(al_np)
    tab = dev(np.asarray(ctg_off, np.int64)) if ctg_off is not None else None
    nc = len(ctg_off) - 1 if ctg_off is not None else 0
    n = C_ if sel is None else len(sel)
    sl = dev(np.asarray(sel, np.int64)) if sel is not None and len(sel) else None
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    spare = 3

    def one(cap_ops_, dir_bytes_, with_cigar):
        ws_bytes = lib.genie_chain_cigars_workspace_bytes(U, cap, n if sel is not None else cap, dir_bytes_)
        assert ws_bytes >= 0 and ws_bytes % 256 == 0
        ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device="cuda")
        offs = torch.full((n + 1 + spare,), fill, dtype=torch.int64, device="cuda")
        cg = torch.full((cap_ops_ + spare,), POISON, dtype=torch.int32, device="cuda") if with_cigar else None
        info = torch.full((n + spare, 8), fill, dtype=torch.int32, device="cuda")
        need = torch.full((n + spare,), fill, dtype=torch.int64, device="cuda")
        tt = torch.full((3,), fill, dtype=torch.int64, device="cuda")
        rc_ = lib.genie_chain_cigars(ix._h, _p(tab), nc, AU.BOTH if b["S"] == 2 else 0, _p(bs), _p(ro), N, int(b["bases"].size),
                                     int(lens.max()) if N else 0, _p(of), _p(rw), U, R, _p(ac), _p(ap), _p(co), _p(ch), cap,
                                     *[int(v) for v in p], _p(al), C.c_void_p(sl.data_ptr() if sl is not None else (8 if sel is not None else 0)),
                                     len(sel) if sel is not None else 0, _p(offs), C.c_void_p(cg.data_ptr() if cg is not None else 0),
                                     cap_ops_, _p(info), _p(need), _p(tt), dir_bytes_, _p(ws), ws_bytes, stream)
        torch.cuda.synchronize()
        assert rc_ == want_rc, rc_
        if rc_:
            return None
        offs_, info_, need_ = offs.cpu().numpy(), info.cpu().numpy(), need.cpu().numpy()
        assert (offs_[n + 1:] == fill).all() and (info_[n:] == fill).all() and (need_[n:] == fill).all(), "written past n_sel"
        res = {"offsets": offs_[:n + 1], "info": info_[:n], "need": need_[:n], "totals": tt.cpu().numpy(), "cigar": None}
        if cg is not None:
            cg_ = cg.cpu().numpy()
            used = min(int(offs_[n]), cap_ops_)
            assert (cg_[used:] == POISON).all(), "written past the ops"
            res["cigar"] = cg_[:used].view(np.uint32)
        return res

    if sizing:
        return one(0, 0 if dir_bytes is None else dir_bytes, False)
    if dir_bytes is None:
        first = one(0, 0, False)
        if first is None:
            return None
        dir_bytes = int(first["totals"][2])
    if cap_ops is None:
        sized = one(0, dir_bytes, False)
        cap_ops = int(sized["offsets"][n])
    return one(cap_ops, dir_bytes, True)


def agrees(got, want):
    for key in ("offsets", "info", "need", "totals", "cigar"):
        if got[key] is None:
            continue
        assert got[key].shape == want[key].shape and np.array_equal(got[key], want[key]), \
            (key, got[key][:40], want[key][:40], cigar_strings(got["offsets"], got["cigar"])[:4] if got["cigar"] is not None else None,
             cigar_strings(want["offsets"], want["cigar"])[:4])


def guarded_call(lib, ix, a, s, b, p, aln, ctg_off, cap, sel=None, cap_ops=0, dir_bytes=0, want_rc=0, extras=True):
    """The call on the guarded buffers of tests/guarded.py, as align_util.guarded_call makes its own: inputs (d_aln and d_sel
    among them) frozen, every output and the workspace cut from the arena `a` with exactly the declared bytes and the weakest
    alignment the header allows, ONE call on stream `s` without synchronising -> a contract_calls.Call.  cap_ops == 0: the
    sizing call (d_cigar NULL); extras: d_dir_need and d_totals are given."""
    import contract_calls as CC
    from guarded import as_numpy
    U, R, total = b["offsets"].size - 1, b["rows"].shape[0], max(0, int(b["chain_offsets"][-1]))
    N = b["read_offsets"].size - 1
    C_ = min(total, cap)
    n = C_ if sel is None else len(sel)
    held = np.zeros((cap, 8), np.int32)
    held[:C_] = b["chains"][:C_]
    al_np = np.zeros((max(cap, 1), 8), np.int32)
    al_np[:min(C_, len(aln))] = aln[:C_]
    pb = CC._inp(a, "bases", b["bases"], 1) if b["bases"].size else 0
    pro, po, pco = (CC._inp(a, nm, b[nm], 8) for nm in ("read_offsets", "offsets", "chain_offsets"))
    pr = CC._inp(a, "rows", b["rows"], 16) if R else 0
    pac = CC._inp(a, "anchor_chain", b["anchor_chain"], 4) if R else 0
    pap = CC._inp(a, "anchor_pred", b["anchor_pred"], 4) if R else 0
    pch = CC._inp(a, "chains", held, 16) if cap else 0
    pal = CC._inp(a, "aln", al_np, 16)
    psl = 0 if sel is None else (CC._inp(a, "sel", np.asarray(sel, np.int64), 8) if len(sel) else 8)
    nc = len(ctg_off) - 1 if ctg_off is not None else 0
    pt = CC._inp(a, "table", np.asarray(ctg_off, np.int64), 8) if ctg_off is not None else 0
    co = a.alloc("cigar_offsets", (n + 1) * 8, 8)
    cg = a.alloc("cigar", cap_ops * 4, 4) if cap_ops else None
    info = a.alloc("info", n * 32, 16) if n else None
    need = a.alloc("dir_need", n * 8, 8) if extras and n else None
    tt = a.alloc("totals", 24, 8) if extras else None
    w, wb = CC._workspace(a, lib.genie_chain_cigars_workspace_bytes(U, cap, n if sel is not None else cap, dir_bytes), None)
    lens = np.diff(b["read_offsets"])
    adr = lambda t, name: CC._vp(a.addr(name) if t is not None else 0)      # noqa: E731
    rc_ = lib.genie_chain_cigars(ix._h, CC._vp(pt), nc, AU.BOTH if b["S"] == 2 else 0, CC._vp(pb), CC._vp(pro), N, int(b["bases"].size),
                                 int(lens.max()) if N else 0, CC._vp(po), CC._vp(pr), U, R, CC._vp(pac), CC._vp(pap), CC._vp(pco),
                                 CC._vp(pch), cap, *[int(v) for v in p], CC._vp(pal), CC._vp(psl), 0 if sel is None else len(sel),
                                 adr(co, "cigar_offsets"), adr(cg, "cigar"), cap_ops, CC._vp(a.addr("info") if n else 16), adr(need, "dir_need"),
                                 adr(tt, "totals"), dir_bytes, CC._vp(w), wb, CC._vp(s))

    def collect():
        res = {"offsets": as_numpy(co, np.int64), "info": as_numpy(info, np.int32, (n, 8)) if n else np.zeros((0, 8), np.int32)}
        ops = int(res["offsets"][n])
        assert 0 <= ops and (np.diff(res["offsets"]) >= 0).all()
        if cg is not None:
            used = min(ops, cap_ops)
            res["cigar"] = as_numpy(cg, np.uint32)[:used]
            assert a.holds_poison(cg[used * 4:]), "ops past the total were written"
        if extras:
            res["need"] = as_numpy(need, np.int64) if n else np.zeros(0, np.int64)
            res["totals"] = as_numpy(tt, np.int64)
        return res
    return CC.Call("chain_cigars", rc_, collect, want_rc)
