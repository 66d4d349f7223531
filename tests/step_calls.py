"""The raw ctypes calls of the call pairs with a step -- genie_match_stats_X and genie_find_smems_X, X = contigs or min_occ --
on buffers of exactly the declared sizes.  A Pair describes what tells one pair from another; contig_stats_util and
min_occ_util bind these functions to theirs."""
import numpy as np

import contig_util as CU
import match_stats_util as MS

BOTH = CU.BOTH


class Pair:
    """genie_match_stats_<suffix> and genie_find_smems_<suffix>.  table: the contig offsets (int64 [C + 1]) of a pair that
    takes (d_contig_offsets, n_contigs) in front of the flags and n_contigs behind the size functions' flags, else None.
    extra: the arguments behind the flags (statistics) or behind min_len (SMEMs)."""

    def __init__(self, suffix, table=None, extra=()):
        self.ms, self.smems = "genie_match_stats_" + suffix, "genie_find_smems_" + suffix
        self.table = None if table is None else np.asarray(table, np.int64)
        self.extra = tuple(extra)
        self.size_tail = () if table is None else (self.table.size - 1,)

    def head(self, pointer):
        """The arguments in front of the flags, `pointer` the table's address as the caller passes pointers."""
        return () if self.table is None else (pointer, self.table.size - 1)

    def size(self, lib, name, parent, n, total, max_len, flags):
        """What the size function of `name` returns: a multiple of 256, no less than the parent's."""
        ws_bytes = getattr(lib, name + "_workspace_bytes")(n, total, max_len, flags, *self.size_tail)
        assert ws_bytes >= getattr(lib, parent)(n, total, max_len, flags) >= 0 and ws_bytes % 256 == 0
        return ws_bytes


def _setup(pair, bases, offs, flags):
    bases, offs = np.asarray(bases, np.uint8), np.asarray(offs, np.int64)
    n, total = offs.size - 1, int(bases.size)
    max_len = int(np.diff(offs).max()) if n else 0
    tab = None if pair.table is None else CU._dev(pair.table)
    return CU._dev(bases if total else np.zeros(1, np.uint8)), CU._dev(offs), tab, n, total, max_len, 2 if flags & BOTH else 1


def ms_call(pair, lib, ix, flags, bases, offs, intervals=True, status=True, totals=True, fill=-7, want_rc=0):
    """One raw statistics call on torch buffers of exactly the declared sizes, the workspace exactly what its size function
    returns, every output filled with `fill` first -> (ms, lohi or None, status or None, total or None)."""
    import torch
    b, of, tab, n, total, max_len, strands = _setup(pair, bases, offs, flags)
    ws_bytes = pair.size(lib, pair.ms, "genie_match_stats_workspace_bytes", n, total, max_len, flags)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device="cuda")
    ms = torch.full((strands * total,), fill, dtype=torch.int32, device="cuda")
    lohi = torch.full((strands * total, 2), fill, dtype=torch.int32, device="cuda") if intervals else None
    st = torch.full((strands * n,), fill, dtype=torch.int32, device="cuda") if status else None
    tt = torch.full((1,), fill, dtype=torch.int64, device="cuda") if totals else None
    p = CU._p
    rc_ = getattr(lib, pair.ms)(ix._h, *pair.head(p(tab)), flags, *pair.extra, p(b), p(of), n, total, max_len, p(ms), p(lohi), p(st),
                                p(tt), p(ws), ws_bytes, CU._stream())
    torch.cuda.synchronize()
    assert rc_ == want_rc, rc_
    if rc_:
        return None
    return (ms.cpu().numpy(), lohi.cpu().numpy() if intervals else None, st.cpu().numpy() if status else None,
            int(tt.item()) if totals else None)


def smem_call(pair, lib, ix, flags, bases, offs, mode=0, min_len=1, cap=0, status=True, totals=True, fill=-7, want_rc=0, spare=0):
    """One raw SMEM call (d_rows: cap + spare rows, of which the call is told cap) -> (offsets, rows, status or None, total or
    None)."""
    import torch
    b, of, tab, n, total, max_len, strands = _setup(pair, bases, offs, flags)
    ws_bytes = pair.size(lib, pair.smems, "genie_find_smems_long_ex_workspace_bytes", n, total, max_len, flags)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device="cuda")
    out = torch.full((strands * n + 1,), fill, dtype=torch.int64, device="cuda")
    rw = torch.full((max(cap + spare, 1), 4), fill, dtype=torch.int32, device="cuda")
    st = torch.full((strands * n,), fill, dtype=torch.int32, device="cuda") if status else None
    tt = torch.full((1,), fill, dtype=torch.int64, device="cuda") if totals else None
    p = CU._p
    rc_ = getattr(lib, pair.smems)(ix._h, *pair.head(p(tab)), mode, flags, p(b), p(of), n, total, max_len, min_len, *pair.extra, p(out),
                                   p(rw), cap, p(st), p(tt), p(ws), ws_bytes, CU._stream())
    torch.cuda.synchronize()
    assert rc_ == want_rc, rc_
    if rc_:
        return None
    return (out.cpu().numpy(), rw.cpu().numpy()[:cap + spare], st.cpu().numpy() if status else None,
            int(tt.item()) if totals else None)


def sized_smem_call(pair, lib, ix, flags, bases, offs, mode=0, min_len=1, **kw):
    """The sizing call (out_cap_rows = 0), then the call with exactly that room -> (offsets, rows, status, total)."""
    first = smem_call(pair, lib, ix, flags, bases, offs, mode, min_len, cap=0, spare=2, **kw)
    assert (first[1] == -7).all(), "the sizing call wrote rows"
    got = smem_call(pair, lib, ix, flags, bases, offs, mode, min_len, cap=int(first[0][-1]), **kw)
    assert np.array_equal(got[0], first[0]) and got[3] == first[3]
    return got


def guarded_calls(pair, lib, ix, a, s, flags, reads, cap):
    """Both calls on the guarded buffers of tests/guarded.py (inputs frozen, the table among them; outputs and workspaces cut
    from the arena `a` with exactly the declared bytes and the weakest alignment the header allows), on stream `s`, not
    synchronised -> their statuses and a function that collects the outputs."""
    import contract_calls as CC
    from guarded import as_numpy
    bases, offs = MS.csr(reads, 5, 3, fill=3)
    n, total = len(reads), int(bases.size)
    strands = 2 if flags & BOTH else 1
    max_len = max([len(r) for r in reads] + [0])
    head = pair.head(None if pair.table is None else CC._vp(CC._inp(a, "contig_offsets", pair.table, 8)))
    p = CC._inp(a, "bases", bases)
    po = CC._inp(a, "read_offsets", offs, 8)
    ms = a.alloc("ms", strands * total * 4, 4)
    lohi = a.alloc("lohi", strands * total * 8, 8)
    st = a.alloc("ms_status", strands * n * 4, 4)
    tt = a.alloc("ms_totals", 8, 8)
    wb = pair.size(lib, pair.ms, "genie_match_stats_workspace_bytes", n, total, max_len, flags)
    a.alloc("ms_workspace", wb, 256)
    rcs = [getattr(lib, pair.ms)(ix._h, *head, flags, *pair.extra, CC._vp(p), CC._vp(po), n, total, max_len, CC._vp(a.addr("ms")),
                                 CC._vp(a.addr("lohi")), CC._vp(a.addr("ms_status")), CC._vp(a.addr("ms_totals")),
                                 CC._vp(a.addr("ms_workspace")), wb, CC._vp(s))]
    offsets = a.alloc("offsets", (strands * n + 1) * 8, 8)
    rows = a.alloc("rows", cap * 16, 16)
    st2 = a.alloc("status", strands * n * 4, 4)
    tt2 = a.alloc("totals", 8, 8)
    wb2 = pair.size(lib, pair.smems, "genie_find_smems_long_ex_workspace_bytes", n, total, max_len, flags)
    a.alloc("workspace", wb2, 256)
    rcs.append(getattr(lib, pair.smems)(ix._h, *head, 0, flags, CC._vp(p), CC._vp(po), n, total, max_len, 1, *pair.extra,
                                        CC._vp(a.addr("offsets")), CC._vp(a.addr("rows")), cap, CC._vp(a.addr("status")),
                                        CC._vp(a.addr("totals")), CC._vp(a.addr("workspace")), wb2, CC._vp(s)))

    def collect():
        o = as_numpy(offsets, np.int64)
        got = min(max(int(o[-1]), 0), cap)
        assert a.holds_poison(rows[got * 16:]), "rows beyond the total were written"
        return {"ms": as_numpy(ms, np.int32), "lohi": as_numpy(lohi, np.int32, (strands * total, 2)), "ms_status": as_numpy(st, np.int32),
                "ms_totals": as_numpy(tt, np.int64), "offsets": o, "rows": as_numpy(rows, np.int32, (cap, 4))[:got],
                "status": as_numpy(st2, np.int32), "totals": as_numpy(tt2, np.int64)}
    return rcs, collect
