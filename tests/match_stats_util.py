"""The specification of genie_match_stats restated in Python, on the brute force of tests/smem_util.py (matching
statistics by substring membership) and tests/lookup_util.py (intervals by bisecting the sorted suffix strings), for the
references of lookup_util.family() (at most 4096 bases).  Nothing here comes from the library under test.  Also the raw
ctypes call the GPU tests make, and the read batches they share.

Layout: S = 2 with both strands, else 1; strand-read S i + s is read i (s = 0) or its reverse complement (s = 1); position
p of it is element S off[i] + s L_i + p of ms and lohi, off[] being the caller's read offsets.
Values, for a strand-read that is not flagged: ms = the largest l >= 0 such that the l bases from p on hold no break and
occur in the reference, lohi = lookup_util.interval of those bases, (-1, -1) for l == 0.  A break is a code > 3, with
split_breaks also a base the reference lacks.  Without split_breaks a strand-read with a code > 3 is flagged
GENIE_READ_BAD_BASE and holds -1 and (-1, -1) throughout; one with a base the reference lacks is flagged
GENIE_READ_ABSENT_BASE and keeps its values."""
import ctypes as C

import numpy as np

import lookup_util as U
import smem_util as SM

BOTH, SPLIT = 1, 2
READ_OK, READ_BAD_BASE, READ_ABSENT_BASE = SM.READ_OK, SM.READ_BAD_BASE, SM.READ_ABSENT_BASE
_ONE = {}           # (reference bytes, strand-read bytes, split) -> (ms, lohi, status)


def rc(read):
    """The reverse complement: reversed, code c -> 3 - c, a code > 3 stays what it is."""
    out = np.asarray(read, np.uint8)[::-1].copy()
    out[out < 4] ^= 3
    return out


def strand_reads(reads, strands):
    """[r0, rc(r0), r1, rc(r1), ...] for two strands, the reads themselves for one."""
    out = []
    for r in reads:
        out.append(np.asarray(r, np.uint8))
        if strands == 2:
            out.append(rc(r))
    return out


def _run_stats(ref, rows, run):
    """(ms, lohi) of a run of bases without a code > 3."""
    fwd = SM.matching_stats(ref, run)
    ms = (fwd - np.arange(len(run))).astype(np.int32)
    lohi = np.full((len(run), 2), -1, np.int32)
    for p, l in enumerate(ms.tolist()):
        if l > 0:
            lohi[p] = U.interval(ref, rows, run[p:p + l])
            assert 0 <= lohi[p, 0] <= lohi[p, 1]
    return ms, lohi


def expected_one(ref, read, split):
    """(ms int32 [L], lohi int32 [L, 2], status) of one strand-read, remembered."""
    read = np.asarray(read, np.uint8)
    key = (U._bytes(ref), U._bytes(read), bool(split))
    if key in _ONE:
        return _ONE[key]
    L, rows = len(read), U.suffix_rows(ref)
    lacks = ~np.isin(read, np.unique(ref)) & (read < 4)
    if not split and (read > 3).any():
        res = (np.full(L, -1, np.int32), np.full((L, 2), -1, np.int32), READ_BAD_BASE)
    elif not split:                                              # a base the reference lacks occurs nowhere: ms = 0 there
        res = _run_stats(ref, rows, read) + (READ_ABSENT_BASE if lacks.any() else READ_OK,)
    else:
        ms, lohi = np.zeros(L, np.int32), np.full((L, 2), -1, np.int32)
        good = (read < 4) & ~lacks
        edges = np.flatnonzero(np.diff(np.concatenate([[0], good.astype(np.int8), [0]])))
        for a, b in zip(edges[::2], edges[1::2]):
            ms[a:b], lohi[a:b] = _run_stats(ref, rows, read[a:b])
        res = (ms, lohi, READ_OK)
    _ONE[key] = res
    return res


def expected(ref, reads, flags, lead=0, tail=0):
    """What the call returns for `reads` given as CSR with `lead` bases in front of the first read and `tail` behind the last
    one (they belong to no read: 0 and (-1, -1)) -> (ms [S total], lohi [S total, 2], status [S N])."""
    strands, split = (2 if flags & BOTH else 1), bool(flags & SPLIT)
    res = [expected_one(ref, r, split) for r in strand_reads(reads, strands)]
    pad = lambda n: (np.zeros(strands * n, np.int32), np.full((strands * n, 2), -1, np.int32))      # noqa: E731
    ms = np.concatenate([pad(lead)[0]] + [r[0] for r in res] + [pad(tail)[0]]).astype(np.int32)
    lohi = np.concatenate([pad(lead)[1]] + [r[1] for r in res] + [pad(tail)[1]]).astype(np.int32).reshape(-1, 2)
    return ms, lohi, np.asarray([r[2] for r in res], np.int32)


def rows_from_lengths(ms):
    """The (start, end) of the SMEMs that the traversal of smem_util.smems derives from the lengths of one strand-read
    (every ms > 0)."""
    ms = np.asarray(ms, np.int64)
    fwd = ms + np.arange(len(ms))
    out, i = [], 0
    while i < len(ms):
        s0 = int(np.searchsorted(fwd, i, side="right"))
        s = s0 + int(np.argmax(ms[s0:i + 1]))
        out.append((s, int(fwd[s])))
        i = int(fwd[s])
    return out


# ------------------------------------------------------------------ the read batches
def window_reads(ref):
    """Reads of 255 .. 513 bases cut from the reference (random bases where it has ended): a match crosses a boundary of
    the 256-position windows, and ends exactly at one."""
    rng = np.random.default_rng(len(ref))
    present = np.unique(ref)
    out = []
    for L in (255, 256, 257, 511, 512, 513):
        s = int(rng.integers(0, max(len(ref) - L, 0) + 1))
        p = ref[s:s + L]
        out.append(np.concatenate([p, present[rng.integers(0, len(present), L - len(p))]]).astype(np.uint8))
    return out


def break_reads(ref):
    """Reads with a code 7, and with a base the reference lacks (where it lacks one; else a second break code), at position
    0, at position L - 1, as an adjacent pair and on either side of a window boundary; one clean read and an empty one."""
    rng = np.random.default_rng(len(ref) + 1)
    present = np.unique(ref)
    lacks = np.setdiff1d(np.arange(4, dtype=np.uint8), present)
    odd = int(lacks[-1]) if len(lacks) else 200

    def clean(L):
        s = int(rng.integers(0, max(len(ref) - L, 0) + 1))
        p = ref[s:s + L]
        return np.concatenate([p, present[rng.integers(0, len(present), L - len(p))]]).astype(np.uint8)

    out = [clean(300), np.zeros(0, np.uint8)]
    for code in (7, odd):
        for L, at in ((40, (0,)), (40, (39,)), (40, (17, 18)), (600, (255,)), (600, (256,)), (600, (255, 256)), (600, (0, 511, 512, 599)),
                      (1, (0,)), (2, (0, 1))):
            r = clean(L)
            r[list(at)] = code
            out.append(r)
    mixed = clean(700)
    mixed[[3, 256, 300]] = 7
    mixed[[100, 257]] = odd
    out.append(mixed)
    return out


def csr(reads, lead=0, tail=0, fill=9):
    """Reads -> (uint8 bases, int64 [N + 1] offsets) with `lead` / `tail` bytes of `fill` around them."""
    off = np.zeros(len(reads) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in reads])
    parts = [np.full(lead, fill, np.uint8)] + [np.asarray(r, np.uint8) for r in reads] + [np.full(tail, fill, np.uint8)]
    return np.concatenate(parts).astype(np.uint8), off + lead


# ------------------------------------------------------------------ the raw call
def call(lib, ix, flags, bases, offs, max_len=None, intervals=True, status=True, ws_mult=1, fill=-7, want_rc=0):
    """One raw genie_match_stats on torch buffers of exactly the declared sizes, the workspace exactly what its size
    function returns (times ws_mult), every output filled with `fill` first -> (ms, lohi or None, status or None) as numpy."""
    import torch
    bases, offs = np.asarray(bases, np.uint8), np.asarray(offs, np.int64)
    n, total = offs.size - 1, int(bases.size)
    strands = 2 if flags & BOTH else 1
    if max_len is None:
        max_len = int(np.diff(offs).max()) if n else 0
    b = torch.as_tensor(bases if total else np.zeros(1, np.uint8)).cuda()
    of = torch.as_tensor(offs).cuda()
    ws_bytes = lib.genie_match_stats_workspace_bytes(n, total, max_len, flags)
    assert ws_bytes >= 0
    assert ws_bytes <= lib.genie_find_smems_long_ex_workspace_bytes(n, total, max_len, flags)
    ws_bytes *= ws_mult
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device="cuda")
    ms = torch.full((strands * total,), fill, dtype=torch.int32, device="cuda")
    lohi = torch.full((strands * total, 2), fill, dtype=torch.int32, device="cuda") if intervals else None
    st = torch.full((strands * n,), fill, dtype=torch.int32, device="cuda") if status else None
    p = lambda t: C.c_void_p(t.data_ptr() if t is not None and t.numel() else 0)      # noqa: E731
    rc_ = lib.genie_match_stats(ix._h, flags, p(b), p(of), n, total, max_len, p(ms), p(lohi), p(st), p(ws), ws_bytes,
                                C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc_ == want_rc, rc_
    if rc_:
        return None
    return ms.cpu().numpy(), (lohi.cpu().numpy() if intervals else None), (st.cpu().numpy() if status else None)


def guarded_call(lib, ix, a, s, flags, reads, lead=0, tail=0, intervals=True, status=True):
    """The call on the guarded buffers of tests/guarded.py, as tests/contract_calls.py makes the others: inputs frozen,
    every output and the workspace cut from the arena `a` with exactly the declared bytes and the weakest alignment the
    header allows, ONE call on stream `s` without synchronising -> a contract_calls.Call."""
    import contract_calls as CC
    from guarded import as_numpy
    bases, offs = csr(reads, lead, tail, fill=3)
    n, total = len(reads), int(bases.size)
    strands = 2 if flags & BOTH else 1
    max_len = max([len(r) for r in reads] + [0])
    p = CC._inp(a, "bases", bases)
    po = CC._inp(a, "read_offsets", offs, 8)
    ms = a.alloc("ms", strands * total * 4, 4)
    lohi = a.alloc("lohi", strands * total * 8, 8) if intervals else None
    st = a.alloc("status", strands * n * 4, 4) if status else None
    w, wb = CC._workspace(a, lib.genie_match_stats_workspace_bytes(n, total, max_len, flags), None)
    rc_ = lib.genie_match_stats(ix._h, flags, CC._vp(p), CC._vp(po), n, total, max_len, CC._vp(a.addr("ms")),
                                CC._vp(a.addr("lohi") if intervals else 0), CC._vp(a.addr("status") if status else 0), CC._vp(w), wb,
                                CC._vp(s))

    def collect():
        res = {"ms": as_numpy(ms, np.int32)}
        if intervals:
            res["lohi"] = as_numpy(lohi, np.int32, (strands * total, 2))
        if status:
            res["status"] = as_numpy(st, np.int32)
        return res
    return CC.Call("match_stats", rc_, collect)
