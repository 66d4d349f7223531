"""The specification of the contig calls (genie_find_mems_contigs, genie_locate_contigs, genie_contig_coords) restated in
Python by brute force, on references of at most 4096 bases cut from lookup_util.family().  Nothing here comes from the
library under test.

A contig table `off` (n_contigs + 1 int64: 0 = off[0] <= ... <= off[n_contigs] = n) cuts the reference T into contigs
T[off[c] .. off[c+1]), some of them empty.  The contig of t < n is the last c with off[c] <= t, room(t) = off[c+1] - t.
The MEMs of a strand-read against the set are restated twice, independently:

  per contig    mems_util.maximal_runs(contig c, read) for every c, the starts shifted by off[c];
  by clipping   the maximal runs along the diagonals of the concatenation, cut at every boundary they cross.

Rows are (p, p + l, t + 1, r), r the row of suffix t of the concatenation (lookup_util.suffix_rows), ordered by (p, r);
status and the positions max_occ skips are those of the concatenation (mems_util).  Also the brute force of
genie_locate_contigs and genie_contig_coords, the cases the host and GPU tests share, and the raw ctypes calls on buffers
of exactly the declared sizes, prefilled, as mems_util.call makes them."""
import ctypes as C

import numpy as np

import lookup_util as U
import match_stats_util as MS
import mems_util as MM

BOTH, SPLIT = MM.BOTH, MM.SPLIT
FLAGS = (0, BOTH, SPLIT, BOTH | SPLIT)
OK, INVALID = 0, -1
_PER = {}               # (contig bytes, strand-read bytes, m) -> its maximal runs of at least m bases
LDS_SAMPLES = 1024      # coords and locate stage at most this many table values per block: more contigs take the second level
WALK_SAMPLES = 12288    # ... and the MEM walks this many


def contig_of(off, t):
    """The contig of every position of t (all below n): the last c with off[c] <= t."""
    off = np.asarray(off, np.int64)
    return np.minimum(np.searchsorted(off, t, side="right") - 1, len(off) - 2)


# ------------------------------------------------------------------ MEMs, twice
def _status(ref, read, split):
    if not split and (read > 3).any():
        return MM.READ_BAD_BASE
    lacks = bool((~np.isin(read, np.unique(ref)) & (read < 4)).any())
    return MM.READ_OK if split or not lacks else MM.READ_ABSENT_BASE


def _finish(ref, read, m, split, max_occ, p, t, l, status):
    skip = MM.skipped_positions(ref, read, m, split, max_occ)
    keep = l >= m
    if skip.size:
        keep &= ~np.isin(p, skip)
    p, t, l = p[keep], t[keep], l[keep]
    r = MM._inverse_rows(ref)[t]
    order = np.lexsort((r, p))
    return np.stack([p, p + l, t + 1, r], 1)[order].astype(np.int32).reshape(-1, 4), status, int(skip.size)


def per_contig_one(ref, off, read, m, split, max_occ=0):
    """(rows, status, skipped) of one strand-read: the union over the contigs of its MEMs against each alone."""
    ref, read, off = np.asarray(ref, np.uint8), np.asarray(read, np.uint8), np.asarray(off, np.int64)
    status = _status(ref, read, split)
    z = np.zeros(0, np.int64)
    if status == MM.READ_BAD_BASE:
        return np.zeros((0, 4), np.int32), status, 0
    ps, ts, ls = [z], [z], [z]
    for c in range(len(off) - 1):
        a, b = int(off[c]), int(off[c + 1])
        if b - a < m:                                               # no match of m bases fits
            continue
        key = (U._bytes(ref[a:b]), U._bytes(read), m)
        if key not in _PER:
            _PER[key] = MM.maximal_runs(ref[a:b], read, m)
        p, t, l = _PER[key]
        ps.append(p)
        ts.append(t + a)
        ls.append(l)
    return _finish(ref, read, m, split, max_occ, np.concatenate(ps), np.concatenate(ts), np.concatenate(ls), status)


def clipped_one(ref, off, read, m, split, max_occ=0):
    """The same by clipping the runs of the concatenation at the boundaries."""
    ref, read, off = np.asarray(ref, np.uint8), np.asarray(read, np.uint8), np.asarray(off, np.int64)
    status = _status(ref, read, split)
    if status == MM.READ_BAD_BASE:
        return np.zeros((0, 4), np.int32), status, 0
    cuts = np.unique(off)
    ps, ts, ls = [], [], []
    p0, t0, l0 = MM._runs(ref, read, m)
    for p, t, l in zip(p0.tolist(), t0.tolist(), l0.tolist()):
        if l < m:
            continue
        inner = cuts[(cuts > t) & (cuts < t + l)].tolist()
        edges = [t] + inner + [t + l]
        for a, b in zip(edges[:-1], edges[1:]):
            ps.append(p + a - t)
            ts.append(a)
            ls.append(b - a)
    arr = lambda x: np.asarray(x, np.int64)      # noqa: E731
    return _finish(ref, read, m, split, max_occ, arr(ps), arr(ts), arr(ls), status)


def expected(ref, off, reads, flags, m, max_occ=0, one=clipped_one):
    """What genie_find_mems_contigs returns -> (offsets int64 [S N + 1], rows int32 [R, 4], status int32 [S N], skipped)."""
    strands, split = (2 if flags & BOTH else 1), bool(flags & SPLIT)
    res = [one(ref, off, r, m, split, max_occ) for r in MS.strand_reads(reads, strands)]
    offs = np.zeros(len(res) + 1, np.int64)
    offs[1:] = np.cumsum([x[0].shape[0] for x in res])
    rows = np.concatenate([x[0] for x in res] + [np.zeros((0, 4), np.int32)]).astype(np.int32).reshape(-1, 4)
    return offs, rows, np.asarray([x[1] for x in res], np.int32), sum(x[2] for x in res)


# ------------------------------------------------------------------ locate and coordinates
def coords_expected(off, n, pos):
    """(contig, 1-based offset) of 1-based concatenation positions; (-1, -1) outside [1, n]."""
    off, pos = np.asarray(off, np.int64), np.asarray(pos, np.int64)
    out = np.full((pos.size, 2), -1, np.int32)
    ok = (pos >= 1) & (pos <= n)
    c = contig_of(off, pos[ok] - 1)
    out[ok, 0] = c
    out[ok, 1] = pos[ok] - off[c]
    return out


def locate_expected(ref, off, rows):
    """genie_locate_contigs by brute force -> (hit_offsets int64 [S + 1], hits int32 [T, 2], dropped)."""
    off, sa, n = np.asarray(off, np.int64), U.suffix_rows(ref), len(ref)
    hits, counts, dropped = [], [], 0
    for s, e, lo, hi in np.asarray(rows, np.int64).reshape(-1, 4).tolist():
        k = 0
        if lo >= 0 and hi >= lo:
            for r in range(lo, hi + 1):
                t = int(sa[r])
                if t >= n:
                    continue                                        # the $ suffix belongs to no contig
                c = int(contig_of(off, t))
                if e - s <= off[c + 1] - t:
                    hits.append((c, t - int(off[c]) + 1))
                    k += 1
                else:
                    dropped += 1
        counts.append(k)
    ho = np.zeros(len(counts) + 1, np.int64)
    ho[1:] = np.cumsum(counts)
    return ho, np.asarray(hits, np.int32).reshape(-1, 2), dropped


# ------------------------------------------------------------------ the shared cases
class Case:
    def __init__(self, ref, off, reads, m, bridge=None, dir_bits=7):
        self.ref, self.off, self.reads, self.m, self.dir_bits = np.asarray(ref, np.uint8), np.asarray(off, np.int64), reads, m, dir_bits
        self.bridge = bridge                                        # a read all of whose occurrences lie across a boundary
        assert self.off[0] == 0 and self.off[-1] == len(self.ref) <= U.MAX_N and (np.diff(self.off) >= 0).all()

    @property
    def n_contigs(self):
        return len(self.off) - 1


def _offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def _other(code):
    return np.uint8((int(code) + 1) & 3)


def _edge_case(m):
    """Contigs of 0, 1, m - 1, m and m + 1 bases, an empty first and an empty last contig, an empty one between two long
    ones.  Reads: across the short contigs; the tail of one contig and the head of the next (one bridging MEM of the
    concatenation, two clipped rows); a read whose base in front of a contig start is the previous contig's last base
    (left-maximal by the contig start alone); a break next to a boundary; breaks and windows from match_stats_util."""
    lens = [0, 1, m - 1, m, m + 1, 300, 0, 50, 700, 0]
    off = _offsets(lens)
    ref = U.family()["rand4096"][:int(off[-1])]
    b5, b7, b8 = int(off[6]), int(off[7]), int(off[8])             # the end of contig 5 = the start of 7 (6 is empty); of 8
    assert b5 == b7
    bridge = ref[b5 - m - 8:b7 + m + 8].copy()
    left = np.concatenate([[_other(ref[b8 - 2])], ref[b8 - 1:b8 + 2 * m + 3]]).astype(np.uint8)
    broken = ref[b8 - 2 * m:b8 + 2 * m].copy()
    broken[2 * m - 1] = 7                                           # the break sits on the last base of contig 7
    reads = [ref[:int(off[5]) + 3 * m].copy(), bridge, left, broken, ref[b8 + 600:].copy(), np.zeros(0, np.uint8)]
    return Case(ref, off, reads + MS.break_reads(ref)[2:8] + MS.window_reads(ref)[:2], m, bridge)


def _wave_case(m, n_contigs=0, repeat=1):
    """41 copies of a 50-base unit; 40 of them are contigs, the one in the middle is cut into contigs of 35 and 15 bases.
    Every seed has more than 32 rows (the whole-wave path), and the occurrences that cross the cut or lie in the 15-base
    contig have room < m: rows dropped in the middle of a wave's mask."""
    unit = U.family()["rand4096"][100:150]
    lens = [50] * 20 + [35, 15] + [50] * 20
    reads = [unit.copy(), unit[5:48].copy(), np.concatenate([[_other(unit[9])], unit[10:]]).astype(np.uint8),
             np.concatenate([unit[20:], unit[:30]]).astype(np.uint8)]
    off = _offsets(lens)
    if n_contigs:
        off = np.sort(np.concatenate([off, np.random.default_rng(n_contigs).choice(off, n_contigs + 1 - off.size)]))
    return Case(np.tile(unit, 41), off, reads * repeat, m, reads[3])


def _table_case(n_contigs, seed):
    """2000 bases in n_contigs contigs: up to 70 non-empty ones at random cuts, the rest empty ones at those cuts."""
    ref = U.family()["rand4096"][1000:3000]
    rng = np.random.default_rng(seed)
    inner = np.sort(rng.choice(np.arange(1, 2000), min(n_contigs, 71) - 1, replace=False))
    cuts = np.concatenate([inner, rng.choice(np.concatenate([inner, [0, 2000]]), n_contigs - 1 - inner.size)]) if n_contigs > 1 else inner
    off = np.concatenate([[0], np.sort(cuts), [2000]]).astype(np.int64)
    reads = [ref[s:s + L].copy() for s, L in ((0, 90), (950, 120), (1880, 120))]
    if n_contigs > 1:
        b = int(inner[inner.size // 2])
        reads.append(ref[b - 20:b + 20].copy())
    return Case(ref, off, reads + MS.break_reads(ref)[2:6], 12, reads[3] if n_contigs > 1 else None)


def cases():
    """name -> Case: every shape the GPU tests run, checked on the host first (tests/test_contigs_host.py)."""
    out = {"edges5": _edge_case(5), "edges12": _edge_case(12), "edges45": _edge_case(45),      # dir_bits 7: <= 7, (7, 39], > 39
           "wave20": _wave_case(20), "wave5": _wave_case(5),
           # one block of the walks with more seed rows than the table has samples: the large staging, whole and sampled
           "wave5_2600": _wave_case(5, 2600, 3), "wave5_13000": _wave_case(5, 13000, 3)}
    # 1500 and 2600: one and two levels below the samples of coords and locate; 13000 and 30000: below those of the walks
    for nc in (1, 2, 3, 5, 64, 65, LDS_SAMPLES - 1, LDS_SAMPLES, 1500, 2600, WALK_SAMPLES - 1, 13000, 30000):
        out[f"table{nc}"] = _table_case(nc, nc)
    return out


_CASES = None


def case(name):
    global _CASES
    if _CASES is None:
        _CASES = cases()
    return _CASES[name]


# ------------------------------------------------------------------ the raw calls
def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _p(t):
    return C.c_void_p(t.data_ptr() if t is not None and t.numel() else 0)


def validate(lib, ix, off):
    import torch
    t = _dev(np.asarray(off, np.int64))
    rc_ = lib.genie_contigs_validate(ix._h, _p(t), t.numel() - 1, _stream())
    torch.cuda.synchronize()
    return rc_


def call(lib, ix, off, flags, bases, offs, m, max_occ=0, cap=0, rows=True, status=True, totals=True, fill=-7, want_rc=0, spare=0):
    """One raw genie_find_mems_contigs on torch buffers of exactly the declared sizes (d_rows: cap + spare rows, of which the
    call is told cap; rows=False: NULL), the workspace exactly what its size function returns, every output filled with
    `fill` first -> (offsets, rows or None, status or None, totals or None) as numpy."""
    import torch
    bases, offs, off = np.asarray(bases, np.uint8), np.asarray(offs, np.int64), np.asarray(off, np.int64)
    n, total = offs.size - 1, int(bases.size)
    strands = 2 if flags & BOTH else 1
    max_len = int(np.diff(offs).max()) if n else 0
    b = _dev(bases if total else np.zeros(1, np.uint8))
    of, tab = _dev(offs), _dev(off)
    ws_bytes = lib.genie_find_mems_contigs_workspace_bytes(n, total, max_len, flags, off.size - 1)
    assert ws_bytes >= lib.genie_find_mems_workspace_bytes(n, total, max_len, flags) >= 0
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device="cuda")
    out = torch.full((strands * n + 1,), fill, dtype=torch.int64, device="cuda")
    rw = torch.full((max(cap + spare, 1), 4), fill, dtype=torch.int32, device="cuda") if rows else None
    st = torch.full((strands * n,), fill, dtype=torch.int32, device="cuda") if status else None
    tt = torch.full((2,), fill, dtype=torch.int64, device="cuda") if totals else None
    rc_ = lib.genie_find_mems_contigs(ix._h, _p(tab), off.size - 1, flags, _p(b), _p(of), n, total, max_len, m, max_occ, _p(out), _p(rw),
                                      cap, _p(st), _p(tt), _p(ws), ws_bytes, _stream())
    torch.cuda.synchronize()
    assert rc_ == want_rc, rc_
    if rc_:
        return None
    return (out.cpu().numpy(), rw.cpu().numpy()[:cap + spare] if rows else None, st.cpu().numpy() if status else None,
            tt.cpu().numpy() if totals else None)


def sized_call(lib, ix, off, flags, bases, offs, m, max_occ=0):
    """The sizing call (d_rows NULL), then the call with exactly that room -> (offsets, rows, status, totals)."""
    off0, none, st0, tt0 = call(lib, ix, off, flags, bases, offs, m, max_occ, rows=False)
    assert none is None and tt0[0] == off0[-1]
    o, rows, st, tt = call(lib, ix, off, flags, bases, offs, m, max_occ, cap=int(off0[-1]))
    assert np.array_equal(o, off0) and np.array_equal(st, st0) and np.array_equal(tt, tt0)
    return o, rows, st, tt


def locate_call(lib, ix, off, rows, cap=0, hits=True, totals=True, fill=-7, spare=0):
    """One raw genie_locate_contigs -> (hit_offsets, hits [cap + spare, 2] or None, totals or None) as numpy."""
    import torch
    rows, off = np.asarray(rows, np.int32).reshape(-1, 4), np.asarray(off, np.int64)
    S = rows.shape[0]
    r, tab = _dev(rows if S else np.zeros((1, 4), np.int32)), _dev(off)
    tmp_bytes = lib.genie_locate_contigs_tmp_bytes(S)
    assert tmp_bytes >= 0 and tmp_bytes % 256 == 0
    tmp = torch.empty(max(tmp_bytes, 1), dtype=torch.uint8, device="cuda")
    ho = torch.full((S + 1,), fill, dtype=torch.int64, device="cuda")
    hh = torch.full((max(cap + spare, 1), 2), fill, dtype=torch.int32, device="cuda") if hits else None
    tt = torch.full((2,), fill, dtype=torch.int64, device="cuda") if totals else None
    rc_ = lib.genie_locate_contigs(ix._h, _p(tab), off.size - 1, _p(r), S, _p(ho), _p(hh), cap, _p(tt), _p(tmp), tmp_bytes, _stream())
    torch.cuda.synchronize()
    assert rc_ == 0, rc_
    return ho.cpu().numpy(), hh.cpu().numpy()[:cap + spare] if hits else None, tt.cpu().numpy() if totals else None


def coords_call(lib, ix, off, pos, stride=1, fill=-7):
    """One raw genie_contig_coords on `pos` (int32, flat; every stride-th element is a position) -> int32 [count, 2]."""
    import torch
    pos, off = np.asarray(pos, np.int32).reshape(-1), np.asarray(off, np.int64)
    count = (pos.size + stride - 1) // stride
    p, tab = _dev(pos if pos.size else np.zeros(1, np.int32)), _dev(off)
    out = torch.full((max(count, 1), 2), fill, dtype=torch.int32, device="cuda")
    rc_ = lib.genie_contig_coords(ix._h, _p(tab), off.size - 1, _p(p), stride, count, _p(out), _stream())
    torch.cuda.synchronize()
    assert rc_ == 0, rc_
    return out.cpu().numpy()[:count]


def guarded_calls(lib, ix, a, s, off, flags, reads, m, cap, smem_rows, cap_hits, pos):
    """The three hot calls on the guarded buffers of tests/guarded.py (inputs frozen, outputs and scratch cut from the arena
    `a` with exactly the declared bytes and the weakest alignment the header allows), on stream `s`, not synchronised ->
    their three statuses.  Used with tables that genie_contigs_validate refuses: only the guards are looked at."""
    import contract_calls as CC
    off = np.asarray(off, np.int64)
    nc = off.size - 1
    bases, offs = MS.csr(reads, 5, 3, fill=3)
    n, total = len(reads), int(bases.size)
    strands = 2 if flags & BOTH else 1
    max_len = max([len(r) for r in reads] + [0])
    tab = CC._inp(a, "contig_offsets", off, 8)
    p = CC._inp(a, "bases", bases)
    po = CC._inp(a, "read_offsets", offs, 8)
    a.alloc("offsets", (strands * n + 1) * 8, 8)
    a.alloc("rows", cap * 16, 16)
    a.alloc("status", strands * n * 4, 4)
    a.alloc("totals", 16, 8)
    w, wb = CC._workspace(a, lib.genie_find_mems_contigs_workspace_bytes(n, total, max_len, flags, nc), None)
    rcs = [lib.genie_find_mems_contigs(ix._h, CC._vp(tab), nc, flags, CC._vp(p), CC._vp(po), n, total, max_len, m, 0,
                                       CC._vp(a.addr("offsets")), CC._vp(a.addr("rows")), cap, CC._vp(a.addr("status")),
                                       CC._vp(a.addr("totals")), CC._vp(w), wb, CC._vp(s))]
    smem_rows = np.asarray(smem_rows, np.int32).reshape(-1, 4)
    S = smem_rows.shape[0]
    pr = CC._inp(a, "smem_rows", smem_rows, 16)
    a.alloc("hit_offsets", (S + 1) * 8, 8)
    a.alloc("hits", cap_hits * 8, 8)
    a.alloc("hit_totals", 16, 8)
    tb = lib.genie_locate_contigs_tmp_bytes(S)
    a.alloc("locate_tmp", tb, 256)
    rcs.append(lib.genie_locate_contigs(ix._h, CC._vp(tab), nc, CC._vp(pr), S, CC._vp(a.addr("hit_offsets")), CC._vp(a.addr("hits")),
                                        cap_hits, CC._vp(a.addr("hit_totals")), CC._vp(a.addr("locate_tmp")), tb, CC._vp(s)))
    pos = np.asarray(pos, np.int32)
    pp = CC._inp(a, "pos", pos, 4)
    a.alloc("coords", pos.size * 8, 4)
    rcs.append(lib.genie_contig_coords(ix._h, CC._vp(tab), nc, CC._vp(pp), 1, pos.size, CC._vp(a.addr("coords")), CC._vp(s)))
    return rcs
