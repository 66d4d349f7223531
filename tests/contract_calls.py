"""Raw calls of the C ABI on guarded buffers (tests/guarded.py), for the memory-contract and stream tests.

Every function here puts its inputs into the arena and freezes them, cuts every output and scratch buffer from the arena
with exactly the bytes the header asks for and the weakest alignment it allows, makes ONE call on the given stream without
synchronising, and returns a Call.  After the stream is synchronised, Call.result() gives the outputs the header defines,
as a dict of numpy arrays, having checked that the status is the expected one and that whatever the header says is dropped
still holds the arena's poison.  Nothing is cleared for the library: the Python wrapper's torch.zeros are bypassed."""
import ctypes as C

import numpy as np

from guarded import as_numpy

MODES = {"bwa": 0, "lut": 1, "rmi": 2}
BOTH, SPLIT = 1, 2


class Call:
    def __init__(self, name, rc, collect, want_rc=0):
        self.name, self.rc, self.want_rc, self._collect = name, rc, want_rc, collect

    def result(self):
        assert self.rc == self.want_rc, (self.name, self.rc)
        return self._collect()


def _vp(addr):
    return C.c_void_p(int(addr))


def _inp(a, name, array, align=1):
    """A frozen input; returns its address (0 for None)."""
    if array is None:
        return 0
    a.freeze(a.put(name, array, align), name)
    return a.addr(name)


def _workspace(a, nbytes, ws):
    """(address, bytes) of the workspace: a fresh piece of the arena of exactly `nbytes`, or the caller's (address, bytes)."""
    assert nbytes >= 0
    if ws is not None:
        assert ws[1] >= nbytes
        return ws[0], nbytes
    a.alloc("workspace", nbytes, 256)
    return a.addr("workspace"), nbytes


def same(x, y):
    """Two results are the same: the same keys, and every array equal in dtype, shape and value."""
    assert x.keys() == y.keys()
    for k in x:
        assert x[k].dtype == y[k].dtype and x[k].shape == y[k].shape and np.array_equal(x[k], y[k]), k


# ------------------------------------------------------------------ intervals and seeds
def sa_interval(lib, ix, a, s, pats, lens, fixed_len):
    n, stride = pats.shape
    p = _inp(a, "pats", pats)
    ln = _inp(a, "lens", None if lens is None else np.asarray(lens, np.int32), 4)
    out = a.alloc("lohi", n * 8, 4)
    rc = lib.genie_sa_interval(ix._h, _vp(p), _vp(ln), n, stride, fixed_len, _vp(a.addr("lohi")), _vp(s))
    return Call("sa_interval", rc, lambda: {"lohi": as_numpy(out, np.int32, (n, 2))})


def seed_lookup(lib, ix, a, s, mode, kmers, want_pred):
    n = kmers.shape[0]
    p = _inp(a, "kmers", kmers)
    out = a.alloc("lohi", n * 8, 4)
    pred = a.alloc("pred", n * 8, 8) if want_pred else None
    rc = lib.genie_seed_lookup(ix._h, MODES[mode], _vp(p), n, _vp(a.addr("lohi")), _vp(a.addr("pred") if want_pred else 0), _vp(s))

    def collect():
        res = {"lohi": as_numpy(out, np.int32, (n, 2))}
        if want_pred:
            res["pred"] = as_numpy(pred, np.float64)
        return res
    return Call("seed_lookup", rc, collect)


# ------------------------------------------------------------------ slots and compaction
def find_slots(lib, ix, a, s, mode, reads, lens, fixed_len, min_len, cap, with_status=True, ws=None):
    n, stride = reads.shape
    p = _inp(a, "reads", reads)
    ln = _inp(a, "lens", None if lens is None else np.asarray(lens, np.int32), 4)
    counts = a.alloc("counts", n * 4, 4)
    slots = a.alloc("slots", n * cap * 16, 16)
    status = a.alloc("status", n * 4, 4) if with_status else None
    w, wb = _workspace(a, lib.genie_find_smems_workspace_bytes(n, fixed_len), ws)
    rc = lib.genie_find_smems(ix._h, MODES[mode], _vp(p), _vp(ln), n, stride, fixed_len, min_len, _vp(a.addr("counts")),
                              _vp(a.addr("slots")), cap, _vp(a.addr("status") if with_status else 0), _vp(w), wb, _vp(s))

    def collect():
        c = as_numpy(counts, np.int32)
        sl = as_numpy(slots, np.int32, (n, cap, 4))
        # the defined slots: [r, 0:min(count, cap))
        rows = [sl[r, :min(max(int(c[r]), 0), cap)] for r in range(n)]
        res = {"counts": c, "slots": np.concatenate(rows) if rows else np.zeros((0, 4), np.int32)}
        if with_status:
            res["status"] = as_numpy(status, np.int32)
        return res
    return Call("find_smems", rc, collect)


def compact(lib, a, s, counts, slots, out_cap):
    """out_cap None: d_out null (the sizing call)."""
    n, cap = slots.shape[0], slots.shape[1]
    pc = _inp(a, "counts", np.asarray(counts, np.int32), 4)
    ps = _inp(a, "slots", np.asarray(slots, np.int32), 16)
    offsets = a.alloc("offsets", (n + 1) * 8, 8)
    rows = a.alloc("rows", out_cap * 16, 16) if out_cap is not None else None
    a.alloc("tmp", lib.genie_compact_tmp_bytes(n), 8)
    rc = lib.genie_compact_smems(_vp(pc), _vp(ps), n, cap, _vp(a.addr("offsets")), _vp(a.addr("rows") if rows is not None else 0),
                                 out_cap or 0, _vp(a.addr("tmp")), _vp(s))

    def collect():
        off = as_numpy(offsets, np.int64)
        res = {"offsets": off}
        if rows is not None:
            got = min(int(off[-1]), out_cap)
            res["rows"] = as_numpy(rows, np.int32, (out_cap, 4))[:got]
            assert a.holds_poison(rows[got * 16:]), "rows beyond the total were written"
        return res
    return Call("compact_smems", rc, collect)


# ------------------------------------------------------------------ CSR output
def _csr_result(a, offsets, rows, status, cap_rows, n_out):
    def collect():
        off = as_numpy(offsets, np.int64)
        got = min(max(int(off[-1]), 0), cap_rows)
        res = {"offsets": off, "rows": as_numpy(rows, np.int32, (cap_rows, 4))[:got]}
        assert a.holds_poison(rows[got * 16:]), "rows beyond the total were written"
        if status is not None:
            res["status"] = as_numpy(status, np.int32)
            assert res["status"].shape == (n_out,)
        return res
    return collect


def find_csr(lib, ix, a, s, kind, mode, reads, lens, fixed_len, min_len, cap_rows, with_status=True, ws=None):
    """kind: "csr", "both" or "split" (which has no mode)."""
    n, stride = reads.shape
    n_out = 2 * n if kind == "both" else n
    p = _inp(a, "reads", reads)
    ln = _inp(a, "lens", None if lens is None else np.asarray(lens, np.int32), 4)
    offsets = a.alloc("offsets", (n_out + 1) * 8, 8)
    rows = a.alloc("rows", cap_rows * 16, 16)
    status = a.alloc("status", n_out * 4, 4) if with_status else None
    size_fn = {"csr": lib.genie_find_smems_workspace_bytes, "both": lib.genie_find_smems_both_workspace_bytes,
               "split": lib.genie_find_smems_split_workspace_bytes}[kind]
    w, wb = _workspace(a, size_fn(n, fixed_len), ws)
    tail = (_vp(a.addr("offsets")), _vp(a.addr("rows")), cap_rows, _vp(a.addr("status") if with_status else 0), _vp(w), wb, _vp(s))
    if kind == "split":
        rc = lib.genie_find_smems_split(ix._h, _vp(p), _vp(ln), n, stride, fixed_len, min_len, *tail)
    else:
        fn = lib.genie_find_smems_csr if kind == "csr" else lib.genie_find_smems_both
        rc = fn(ix._h, MODES[mode], _vp(p), _vp(ln), n, stride, fixed_len, min_len, *tail)
    return Call("find_smems_" + kind, rc, _csr_result(a, offsets, rows, status, cap_rows, n_out))


def find_long(lib, ix, a, s, flags, mode, reads, min_len, cap_rows, first=0, slack=0, with_status=True, ws=None):
    """flags None: genie_find_smems_long; else genie_find_smems_long_ex.  reads: a list of uint8 arrays; `first` unused
    bases in front of the first read (a nonzero first offset) and `slack` more behind the last (total_bases beyond the
    last offset)."""
    n = len(reads)
    lens = [len(r) for r in reads]
    offs = np.zeros(n + 1, np.int64)
    offs[0] = first
    offs[1:] = first + np.cumsum(lens)
    bases = np.concatenate([np.full(first, 3, np.uint8)] + [np.asarray(r, np.uint8) for r in reads] + [np.full(slack, 2, np.uint8)])
    total, max_len = int(bases.size), max(lens + [0])
    n_out = 2 * n if (flags or 0) & BOTH else n
    p = _inp(a, "bases", bases)
    po = _inp(a, "read_offsets", offs, 8)
    offsets = a.alloc("offsets", (n_out + 1) * 8, 8)
    rows = a.alloc("rows", cap_rows * 16, 16)
    status = a.alloc("status", n_out * 4, 4) if with_status else None
    if flags is None:
        need = lib.genie_find_smems_long_workspace_bytes(n, total, max_len)
    else:
        need = lib.genie_find_smems_long_ex_workspace_bytes(n, total, max_len, flags)
    w, wb = _workspace(a, need, ws)
    tail = (_vp(p), _vp(po), n, total, max_len, min_len, _vp(a.addr("offsets")), _vp(a.addr("rows")), cap_rows,
            _vp(a.addr("status") if with_status else 0), _vp(w), wb, _vp(s))
    if flags is None:
        rc = lib.genie_find_smems_long(ix._h, MODES[mode], *tail)
    else:
        rc = lib.genie_find_smems_long_ex(ix._h, MODES[mode], flags, *tail)
    return Call("find_smems_long", rc, _csr_result(a, offsets, rows, status, cap_rows, n_out))


# ------------------------------------------------------------------ packed reads, compact rows
def find_packed(lib, ix, a, s, row_bytes, mode, codes, lens, min_len, cap_rows, cap_escapes, ws=None, calls=1):
    """cap_escapes None: a null escape list with capacity 0.  calls = 2: the same call again on the same buffers with
    nothing cleared in between (the rerun loop of the Python wrapper); the caller compares with a single call's result."""
    from genie_smem_amd import packing
    n, L = codes.shape
    packed = packing.pack_reads(codes)
    p = _inp(a, "reads2bit", packed, 4)
    ln = _inp(a, "lens", None if lens is None else np.asarray(lens, np.int32), 4)
    counts8 = a.alloc("counts8", n, 1)
    status8 = a.alloc("status8", n, 1)
    rows = a.alloc("rows", cap_rows * row_bytes, 8 if row_bytes == 8 else 2)
    totals = a.alloc("totals", 16, 8)
    esc = a.alloc("escapes", cap_escapes * 16, 8) if cap_escapes is not None else None
    w, wb = _workspace(a, lib.genie_find_smems_workspace_bytes(n, L), ws)
    fn = lib.genie_find_smems_packed if row_bytes == 8 else lib.genie_find_smems_packed6
    rc = 0
    for _ in range(calls):
        rc = rc or fn(ix._h, MODES[mode], _vp(p), _vp(ln), n, packed.shape[1], L, min_len, _vp(a.addr("counts8")),
                      _vp(a.addr("status8")), _vp(a.addr("rows")), cap_rows, _vp(a.addr("totals")),
                      _vp(a.addr("escapes") if esc is not None else 0), cap_escapes or 0, _vp(w), wb, _vp(s))

    def collect():
        tot = as_numpy(totals, np.int64)
        got = min(max(int(tot[0]), 0), cap_rows)
        res = {"counts8": as_numpy(counts8, np.uint8), "status8": as_numpy(status8, np.uint8), "totals": tot,
               "rows": as_numpy(rows, np.uint8, (cap_rows, row_bytes))[:got]}
        assert a.holds_poison(rows[got * row_bytes:]), "rows beyond the total were written"
        if esc is not None:
            kept = min(max(int(tot[1]), 0), cap_escapes)
            e = as_numpy(esc, np.int64, (cap_escapes, 2))[:kept]
            res["escapes"] = e[np.lexsort((e[:, 1], e[:, 0]))]          # unordered by contract: compared as a set
            assert len({tuple(x) for x in e.tolist()}) == kept, "an escape was listed twice"
            assert a.holds_poison(esc[kept * 16:]), "escapes beyond the total were written"
        return res
    return Call("find_smems_packed", rc, collect)


# ------------------------------------------------------------------ positions
def locate(lib, ix, a, s, lohi, cap):
    """lohi: int32 [S, stride] with (lo, hi) in the first two columns; cap None: d_positions null (the sizing call)."""
    S, stride = lohi.shape
    p = _inp(a, "lohi", np.asarray(lohi, np.int32), 4)
    offsets = a.alloc("pos_offsets", (S + 1) * 8, 8)
    pos = a.alloc("positions", cap * 4, 4) if cap is not None else None
    need = lib.genie_locate_tmp_bytes(S)
    a.alloc("tmp", need, 256)
    rc = lib.genie_locate(ix._h, _vp(p), stride, S, _vp(a.addr("pos_offsets")), _vp(a.addr("positions") if pos is not None else 0),
                          cap or 0, _vp(a.addr("tmp")), need, _vp(s))

    def collect():
        off = as_numpy(offsets, np.int64)
        res = {"pos_offsets": off}
        if pos is not None:
            got = min(int(off[-1]), cap)
            res["positions"] = as_numpy(pos, np.int32)[:got]
            assert a.holds_poison(pos[got * 4:]), "positions beyond the total were written"
        return res
    return Call("locate", rc, collect)
