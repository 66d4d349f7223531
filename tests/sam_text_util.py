"""The brute force of genie_sam_text (include/genie_smem.h) in plain Python -- every line field by field, straight from the
definition -- with the raw ctypes call, the call on the guarded buffers of tests/guarded.py, and builders of synthetic batches
that need no pipeline: the call itself needs the index only for the reference letters of MD.

A batch is a dict: bases uint8, read_offsets int64[N+1], quals uint8 or None, sel_offsets int64[N+1], records int32[T, 12], sam
int32[T, 4] or None (single-end mode), info int32[T, 8], cigar_offsets int64[T+1], cigar uint32, names and contig_names lists of
bytes, contig_offsets int64[nc+1] or None."""
import ctypes as C

import numpy as np

import pair_util as PU

NM, AS, MD, MC, MQ = 1, 2, 4, 8, 16
NO_SEQ = 1
I, D, S, EQ, X = 1, 2, 4, 7, 8
OP_LETTERS = "MIDNSHP=X"
INVALID, NO_DEVICE, CAPACITY, TOO_LONG = -1, -4, -10, -6
clamp = PU.clamp


def op(length, code):
    return (length << 4) | code


def cigar_text(ops):
    return "".join(f"{int(v) >> 4}{OP_LETTERS[int(v) & 15] if int(v) & 15 < 9 else '?'}" for v in ops)


def md_text(ops, T, t):
    """MD of ops whose first reference position is t (0-based in the concatenation T), by the definition's serial walk."""
    out, c = [], 0
    letter = lambda p: "ACGT"[int(T[clamp(p, 0, len(T) - 1)]) & 3]      # noqa: E731
    for v in ops:
        code, n = int(v) & 15, int(v) >> 4
        if code == EQ:
            c += n
            t += n
        elif code == X:
            for _ in range(n):
                out.append(f"{c}{letter(t)}")
                c = 0
                t += 1
        elif code == D:
            out.append(f"{c}^" + "".join(letter(t + i) for i in range(n)))
            c = 0
            t += n
    return "".join(out) + str(c)


def seq_text(codes, turned):
    if turned:
        codes = [3 - int(c) if c < 4 else int(c) for c in codes[::-1]]
    return "".join("ACGT"[int(c)] if c < 4 else "N" for c in codes)


def expected(b, T, tags=NM | AS, flags=0, n_records=None):
    """-> {"text": uint8[bytes], "line_offsets": int64[n_lines + 1], "totals": int64[3]}."""
    so, rec, sam, info, co, cg = b["sel_offsets"], b["records"], b["sam"], b["info"], b["cigar_offsets"], b["cigar"]
    N = so.size - 1
    n_records = rec.shape[0] if n_records is None else n_records
    R = clamp(int(so[N]), 0, n_records)
    names = [bytes(x).decode("latin-1") for x in b["names"]]
    cnames = [bytes(x).decode("latin-1") for x in b["contig_names"]]
    table = b.get("contig_offsets")
    nc = table.size - 1 if table is not None else 1                  # names there are: max(n_contigs, 1)
    cname = lambda c: cnames[clamp(int(c), 0, nc - 1)]               # noqa: E731
    ops_of = lambda j: cg[int(co[j]):int(co[j + 1])]                 # noqa: E731

    def seq_qual(r, turned):
        if flags & NO_SEQ:
            return ["*", "*"]
        lo, hi = int(b["read_offsets"][r]), int(b["read_offsets"][r + 1])
        qual = "*"
        if b["quals"] is not None:
            q = b["quals"][lo:hi]
            qual = bytes(q[::-1] if turned else q).decode("latin-1")
        return [seq_text(b["bases"][lo:hi], turned), qual]

    def mate_tags(m):
        out = []
        if m is not None:
            if tags & MC and len(ops_of(m)):
                out.append("MC:Z:" + cigar_text(ops_of(m)))
            if tags & MQ:
                out.append(f"MQ:i:{int(sam[m][1])}")
        return out

    lines, unmapped = [], 0
    for r in range(N):
        lo, hi = PU.read_records(b, r, R)
        for j in range(lo, hi):
            _, _, kind, strand, contig, offset, _, _, _, score, _, own = (int(v) for v in rec[j])
            mate = None
            if sam is not None:
                flag, mapq, m, tlen = (int(v) for v in sam[j])
                mate = m if 0 <= m < R else None
            else:
                flag, mapq, tlen = (0x10 if strand else 0) | (0x800 if kind == 1 else 0) | (0x100 if kind == 2 else 0), own, 0
            rnext, pnext = "*", 0
            if mate is not None:
                rnext, pnext = "=" if int(rec[mate][4]) == contig else cname(rec[mate][4]), int(rec[mate][5])
            ops = ops_of(j)
            cols = [names[r], flag, cname(contig), offset, mapq, cigar_text(ops) or "*", rnext, pnext, tlen] + seq_qual(r, strand != 0)
            if tags & NM:
                cols.append(f"NM:i:{int(info[j][3])}")
            if tags & AS:
                cols.append(f"AS:i:{score}")
            if tags & MD and len(ops):
                start = int(table[clamp(contig, 0, len(table) - 2)]) if table is not None else 0
                cols.append("MD:Z:" + md_text(ops, T, clamp(start, 0, len(T)) + offset - 1))
            lines.append("\t".join(str(c) for c in cols + mate_tags(mate)))
        if lo == hi:
            unmapped += 1
            if sam is None:
                cols = [names[r], 4, "*", 0, 0, "*", "*", 0, 0] + seq_qual(r, False)
                lines.append("\t".join(str(c) for c in cols))
                continue
            flag, rname, pos, rnext, mate = 0x1 | 0x4 | (0x80 if r & 1 else 0x40), "*", 0, "*", None
            mlo, mhi = PU.read_records(b, r ^ 1, R)
            for j in range(mlo, mhi):
                if not int(sam[j][0]) & 0x900:
                    mate = j
            if mate is None:
                flag |= 0x8
            else:
                flag |= 0x20 if int(rec[mate][3]) else 0
                rname, pos, rnext = cname(rec[mate][4]), int(rec[mate][5]), "="
            cols = [names[r], flag, rname, pos, 0, "*", rnext, pos, 0] + seq_qual(r, False)
            lines.append("\t".join(str(c) for c in cols + mate_tags(mate)))
    raw = [(ln + "\n").encode("latin-1") for ln in lines]
    off = np.zeros(len(raw) + 1, np.int64)
    if raw:
        off[1:] = np.cumsum([len(x) for x in raw])
    return {"text": np.frombuffer(b"".join(raw), np.uint8).copy(), "line_offsets": off,
            "totals": np.array([len(raw), int(off[-1]), unmapped], np.int64)}


def agrees(got, want, cap_text=None):
    assert np.array_equal(got["line_offsets"], want["line_offsets"]), (got["line_offsets"][:8], want["line_offsets"][:8])
    if "totals" in got:
        assert got["totals"].tolist() == want["totals"].tolist()
    if "text" in got:
        w = want["text"] if cap_text is None else want["text"][:cap_text]
        assert got["text"].size == w.size, (got["text"].size, w.size)
        bad = np.flatnonzero(got["text"] != w)
        if bad.size:
            at = int(bad[0])
            line = int(np.searchsorted(want["line_offsets"], at, side="right")) - 1
            lo, hi = int(want["line_offsets"][line]), int(want["line_offsets"][line + 1])
            raise AssertionError((f"byte {at}, line {line}, column {at - lo}", bytes(got["text"][lo:hi][:400]), bytes(w[lo:hi][:400])))


# ------------------------------------------------------------------ batches
def make_batch(rng, reads, names=None, contig_names=(b"a", b"b", b"c"), contig_offsets=None, quals=True, single=False, pair=None,
               code4=0.02):
    """reads: per read (length, [record, ...]), a record a dict with ops (a list of op()) and any of kind, parent, strand, contig,
    offset, score, mapq, nm.  r_span is what the ops cover of the reference.  sam comes from pair_util's brute force over the
    records (pair: its parameters), so flags, mates and TLEN are those of a real pairing; single: sam is None."""
    rows = []
    for _, recs in reads:
        rows.append([(q.get("kind", 0 if i == 0 else 2), q.get("parent", 0), q.get("strand", 0), q.get("contig", 0), q.get("offset", 1),
                      sum(int(v) >> 4 for v in q["ops"] if int(v) & 15 in (D, EQ, X)), q.get("score", 60), q.get("mapq", 30))
                     for i, q in enumerate(recs)])
    pad = len(rows) % 2 if single else 0
    b = PU.make_batch(rows + [[]] * pad)
    if pad:
        b["sel_offsets"] = b["sel_offsets"][:-1]
    b["sam"] = None if single else PU.expected(b, pair or PU.DEFAULTS._replace(orient=7))["sam"]
    flat = [q for _, recs in reads for q in recs]
    b["info"] = np.zeros((len(flat), 8), np.int32)
    b["info"][:, 3] = [q.get("nm", sum(int(v) >> 4 for v in q["ops"] if int(v) & 15 in (I, D, X)) & 0x7fffffff) for q in flat]
    b["cigar_offsets"] = np.zeros(len(flat) + 1, np.int64)
    if flat:
        b["cigar_offsets"][1:] = np.cumsum([len(q["ops"]) for q in flat])
    b["cigar"] = np.array([v for q in flat for v in q["ops"]], np.uint32)
    lens = [n for n, _ in reads]
    b["read_offsets"] = np.zeros(len(reads) + 1, np.int64)
    b["read_offsets"][1:] = np.cumsum(lens)
    total = int(b["read_offsets"][-1])
    b["bases"] = np.where(rng.random(total) < code4, 4, rng.integers(0, 4, total)).astype(np.uint8)
    b["quals"] = rng.integers(33, 127, total).astype(np.uint8) if quals else None
    b["names"] = [f"read{r // 2}".encode() for r in range(len(reads))] if names is None else [bytes(x) for x in names]
    b["contig_names"] = [bytes(x) for x in contig_names]
    b["contig_offsets"] = None if contig_offsets is None else np.asarray(contig_offsets, np.int64)
    return b


def random_ops(rng, n_ops, clips=True):
    """n_ops ops of an alignment in CIGAR order: = runs with X, I and D between them, S at the ends."""
    if n_ops == 0:
        return []
    body = n_ops - (2 if clips and n_ops >= 3 else 0)
    ops = []
    for i in range(body):
        if i % 2 == 0:
            ops.append(op(int(rng.integers(1, 40)), EQ))
        else:
            ops.append(op(int(rng.integers(1, 4)), int(rng.choice([X, X, I, D]))))
    if body < n_ops:
        ops = [op(int(rng.integers(1, 20)), S)] + ops + [op(int(rng.integers(1, 20)), S)]
    return ops


def query_length(ops):
    return sum(int(v) >> 4 for v in ops if int(v) & 15 in (I, S, EQ, X))


def random_reads(rng, counts, table, max_ops=9):
    """One read per entry of counts with that many records, placed so that every alignment lies inside its contig."""
    reads = []
    for n in counts:
        recs, length = [], int(rng.integers(0, 200))
        for i in range(n):
            ops = random_ops(rng, int(rng.integers(0, max_ops + 1)))
            if i == 0 and ops:
                length = query_length(ops)
            c = int(rng.integers(0, len(table) - 1))
            room = int(table[c + 1] - table[c]) - sum(int(v) >> 4 for v in ops if int(v) & 15 in (D, EQ, X))
            recs.append(dict(ops=ops, kind=0 if i == 0 else int(rng.choice([1, 2, 2])), strand=int(rng.integers(0, 2)), contig=c,
                             offset=1 + int(rng.integers(0, max(room, 1))), score=int(rng.integers(20, 200)), mapq=int(rng.integers(0, 61))))
        reads.append((length, recs))
    return reads


def csr(names):
    off = np.zeros(len(names) + 1, np.int64)
    if names:
        off[1:] = np.cumsum([len(x) for x in names])
    return np.frombuffer(b"".join(names), np.uint8).copy(), off


# ------------------------------------------------------------------ the call
def _arrays(b, n_records):
    """The inputs as the call takes them, in its argument order, each (name, array or None, alignment)."""
    rec = b["records"]
    n_records = rec.shape[0] if n_records is None else n_records
    held = lambda a: np.ascontiguousarray(a[:n_records]) if a is not None else None      # noqa: E731
    nb, no = csr(b["names"])
    cb, cno = csr(b["contig_names"])
    return n_records, {"contig_offsets": (b.get("contig_offsets"), 8), "bases": (b["bases"], 1), "read_offsets": (b["read_offsets"], 8),
                       "quals": (b["quals"], 1), "sel_offsets": (b["sel_offsets"], 8), "records": (held(rec), 16),
                       "sam": (held(b["sam"]), 16), "info": (held(b["info"]), 16), "cigar_offsets": (b["cigar_offsets"], 8),
                       "cigar": (b["cigar"], 4), "names": (nb, 1), "name_offsets": (no, 8), "contig_names": (cb, 1),
                       "contig_name_offsets": (cno, 8)}


def _invoke(lib, ix, b, n_records, ptr, tags, flags, line_offsets, text, cap_text, totals, ws, ws_bytes, stream):
    """ptr: name -> address (0 for an input that is None or, unless it stands for a mode, empty)."""
    table = b.get("contig_offsets")
    vp = C.c_void_p
    return lib.genie_sam_text(ix._h, vp(ptr("contig_offsets")), 0 if table is None else table.size - 1, vp(ptr("bases")),
                              vp(ptr("read_offsets")), b["read_offsets"].size - 1, b["bases"].size, vp(ptr("quals")),
                              vp(ptr("sel_offsets")), vp(ptr("records")), n_records, vp(ptr("sam")), vp(ptr("info")),
                              vp(ptr("cigar_offsets")), vp(ptr("cigar")), b["cigar"].size, vp(ptr("names")), vp(ptr("name_offsets")),
                              sum(len(x) for x in b["names"]), vp(ptr("contig_names")), vp(ptr("contig_name_offsets")),
                              sum(len(x) for x in b["contig_names"]), tags, flags, vp(line_offsets), vp(text), cap_text, vp(totals),
                              vp(ws), ws_bytes, vp(stream))


def call(lib, ix, b, tags=NM | AS, flags=0, cap_text=None, n_records=None, totals=True, want_rc=0):
    """The raw calls on torch tensors of the current device: the sizing call, then the filling call with room for cap_text
    bytes (default: all) -> text, line_offsets and totals as expected() returns them (text cut to cap_text)."""
    import torch
    dev = "cuda"
    n_records, arrays = _arrays(b, n_records)
    N = b["read_offsets"].size - 1
    held = {}
    for name, (a, _) in arrays.items():
        if a is not None:
            # an address for an empty quals or sam too: NULL there selects a mode
            held[name] = torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).to(dev) if a.size else \
                torch.zeros(16, dtype=torch.uint8, device=dev)
    ptr = lambda name: held[name].data_ptr() if name in held and (arrays[name][0].size or name in ("quals", "sam")) else 0      # noqa: E731
    lo = torch.full((N + n_records + 1 + 2,), -77, dtype=torch.int64, device=dev)
    tt = torch.full((3,), -77, dtype=torch.int64, device=dev) if totals else None
    wsb = lib.genie_sam_text_workspace_bytes(N, n_records)
    ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device=dev)
    tp = tt.data_ptr() if totals else 0
    rc = _invoke(lib, ix, b, n_records, ptr, tags, flags, lo.data_ptr(), 0, 0, tp, ws.data_ptr(), wsb, 0)
    torch.cuda.synchronize()
    assert rc == want_rc, rc
    if want_rc:
        return None
    sized = lo.cpu().numpy()
    n_lines = int(np.flatnonzero(sized == -77)[0]) - 1
    total = int(sized[n_lines])
    cap = total if cap_text is None else cap_text
    text = torch.full((cap + 64,), 0x7e, dtype=torch.uint8, device=dev)
    lo2 = torch.full_like(lo, -77)
    rc = _invoke(lib, ix, b, n_records, ptr, tags, flags, lo2.data_ptr(), text.data_ptr(), cap, tp, ws.data_ptr(), wsb, 0)
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert np.array_equal(lo2.cpu().numpy(), sized), "the sizing call and the filling call disagree about the offsets"
    assert (text[min(cap, total):] == 0x7e).all(), "bytes at or past min(cap_text, total) were written"
    res = {"text": text[:min(cap, total)].cpu().numpy(), "line_offsets": sized[:n_lines + 1]}
    if totals:
        res["totals"] = tt.cpu().numpy()
    return res


def guarded_call(lib, ix, a, s, b, tags=NM | AS, flags=0, cap_text=0, n_records=None, totals=True, fill=True, want_rc=0):
    """ONE call on the guarded buffers of tests/guarded.py: inputs frozen, outputs and workspace cut from the arena `a` with
    exactly the declared bytes and the weakest alignment the header allows, on stream `s` without synchronising -> a
    contract_calls.Call.  fill=False: d_text is NULL, the sizing call."""
    import contract_calls as CC
    from guarded import as_numpy
    n_records, arrays = _arrays(b, n_records)
    N = b["read_offsets"].size - 1
    addr = {}
    for name, (arr, align) in arrays.items():
        if arr is not None:
            addr[name] = CC._inp(a, name, arr, align)
    ptr = lambda name: addr[name] if name in addr and (arrays[name][0].size or name in ("quals", "sam")) else 0      # noqa: E731
    lo = a.alloc("line_offsets", (N + n_records + 1) * 8, 8)
    text = a.alloc("text", cap_text, 1) if fill else None
    tt = a.alloc("totals", 24, 8) if totals else None
    w, wb = CC._workspace(a, lib.genie_sam_text_workspace_bytes(N, n_records), None)
    rc = _invoke(lib, ix, b, n_records, ptr, tags, flags, a.addr("line_offsets"), a.addr("text") if fill else 0, cap_text,
                 a.addr("totals") if totals else 0, w, wb, s)
    R = clamp(int(b["sel_offsets"][N]), 0, n_records)

    def collect():
        off = as_numpy(lo, np.int64)
        so = np.clip(b["sel_offsets"], 0, R)
        n_lines = R + int((np.diff(so) == 0).sum())
        assert a.holds_poison(lo[(n_lines + 1) * 8:]), "line offsets past n_lines were written"
        res = {"line_offsets": off[:n_lines + 1]}
        if fill:
            got = min(max(int(off[n_lines]), 0), cap_text)
            res["text"] = as_numpy(text, np.uint8)[:got]
            assert a.holds_poison(text[got:]), "bytes past the total were written"
        if totals:
            res["totals"] = as_numpy(tt, np.int64)
        return res
    return CC.Call("sam_text", rc, collect, want_rc)
