"""Two independent pieces for genie_bam_records (include/genie_smem.h), in plain Python:

(a) host_bam_records: the brute force -- every record byte by byte, straight from the header's definition -- on the synthetic
    batches of tests/sam_text_util.py, with the raw ctypes call and the call on the guarded buffers of tests/guarded.py in that
    module's patterns;
(b) bam_to_sam: a decoder written from the SAM specification alone (SAMv1 section 4.2), which shares no code with (a) or the
    library.  It turns a stream of records back into SAM lines and checks block_size, the NUL terminators and bin on the way.

(a) through (b) must give the text of sam_text_util.expected: that ties the BAM definition to the SAM one."""
import ctypes as C
import struct

import numpy as np

import pair_util as PU
import sam_text_util as ST

NM, AS, MD, MC, MQ, NO_SEQ = ST.NM, ST.AS, ST.MD, ST.MC, ST.MQ, ST.NO_SEQ
clamp = PU.clamp
REF_CODES = (0, 2, 3, 7, 8)                                          # the ops that cover the reference: M D N = X


def w32(v):
    """v as an int32 that wraps."""
    return ((int(v) + 2**31) % 2**32) - 2**31


def reg2bin(beg, end):
    """SAMv1 section 5.3, on Python's integers (>> is arithmetic)."""
    end -= 1
    if beg >> 14 == end >> 14:
        return ((1 << 15) - 1) // 7 + (beg >> 14)
    if beg >> 17 == end >> 17:
        return ((1 << 12) - 1) // 7 + (beg >> 17)
    if beg >> 20 == end >> 20:
        return ((1 << 9) - 1) // 7 + (beg >> 20)
    if beg >> 23 == end >> 23:
        return ((1 << 6) - 1) // 7 + (beg >> 23)
    if beg >> 26 == end >> 26:
        return ((1 << 3) - 1) // 7 + (beg >> 26)
    return 0


def ref_span(ops):
    ops = np.asarray(ops, np.int64)
    return int((ops >> 4)[np.isin(ops & 15, REF_CODES)].sum()) if ops.size else 0


def encode_record(name, flag, ref_id, pos, mapq, ops, next_id, next_pos, tlen, codes, quals, turned, tag_bytes):
    """One record from its columns: pos and next_pos are BAM's (0-based), codes the read's base codes in read orientation or
    None (no SEQ), quals its quality characters or None (0xFF), tag_bytes the tags but CG, already encoded."""
    ops = np.asarray(ops, np.uint32)
    stored = bytes(name)[:254] or b"*"
    l_seq = 0 if codes is None else len(codes)
    span = ref_span(ops)
    beg = w32(pos)
    big = ops.size > 65535
    cigar = ops.astype("<u4").tobytes()
    tail = b""
    if big:
        tail = b"CGBI" + struct.pack("<i", ops.size) + cigar
        cigar = struct.pack("<II", (l_seq << 4 | 4) & 0xffffffff, min(span, 2**28 - 1) << 4 | 3)
    seq = qual = b""
    if l_seq:
        c = np.asarray(codes, np.uint8)
        if turned:
            c = np.where(c < 4, 3 - c, c)[::-1]
        nib = np.where(c < 4, 1 << np.minimum(c, 3), 15).astype(np.uint8)
        if l_seq & 1:
            nib = np.concatenate([nib, [0]]).astype(np.uint8)
        seq = ((nib[0::2] << 4) | nib[1::2]).astype(np.uint8).tobytes()
        if quals is None:
            qual = b"\xff" * l_seq
        else:
            q = np.maximum(np.asarray(quals, np.int64) - 33, 0).astype(np.uint8)
            qual = (q[::-1] if turned else q).tobytes()
    body = struct.pack("<iiBBHHHiiii", ref_id, beg, len(stored) + 1, clamp(int(mapq), 0, 255),
                       reg2bin(beg, beg + (span or 1)) & 0xffff, 2 if big else ops.size, int(flag) & 0xffff, l_seq, next_id, w32(next_pos),
                       w32(tlen))
    body += stored + b"\0" + cigar + seq + qual + tag_bytes + tail
    return struct.pack("<i", len(body)) + body


def tag_i(name, v):
    return name + b"i" + struct.pack("<i", w32(v))


def tag_z(name, text):
    return name + b"Z" + text.encode("latin-1") + b"\0"


def host_bam_records(b, T, tags=NM | AS, flags=0, n_records=None):
    """-> {"data": uint8[bytes], "record_offsets": int64[n + 1], "totals": int64[3]}."""
    so, rec, sam, info, co, cg = b["sel_offsets"], b["records"], b["sam"], b["info"], b["cigar_offsets"], b["cigar"]
    N = so.size - 1
    n_records = rec.shape[0] if n_records is None else n_records
    R = clamp(int(so[N]), 0, n_records)
    table = b.get("contig_offsets")
    nc = table.size - 1 if table is not None else 1
    cid = lambda c: clamp(int(c), 0, nc - 1)                         # noqa: E731
    ops_of = lambda j: cg[int(co[j]):int(co[j + 1])]                 # noqa: E731

    def read_of(r, turned):
        if flags & NO_SEQ:
            return None, None
        lo, hi = int(b["read_offsets"][r]), int(b["read_offsets"][r + 1])
        return b["bases"][lo:hi], (b["quals"][lo:hi] if b["quals"] is not None else None)

    def mate_tags(m):
        out = b""
        if m is not None:
            if tags & MC and len(ops_of(m)):
                out += tag_z(b"MC", ST.cigar_text(ops_of(m)))
            if tags & MQ:
                out += tag_i(b"MQ", sam[m][1])
        return out

    out, unmapped = [], 0
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
            next_id, pnext = (cid(rec[mate][4]), int(rec[mate][5])) if mate is not None else (-1, 0)
            ops = ops_of(j)
            t = b""
            if tags & NM:
                t += tag_i(b"NM", info[j][3])
            if tags & AS:
                t += tag_i(b"AS", score)
            if tags & MD and len(ops):
                start = int(table[clamp(contig, 0, len(table) - 2)]) if table is not None else 0
                t += tag_z(b"MD", ST.md_text(ops, T, clamp(start, 0, len(T)) + offset - 1))
            codes, quals = read_of(r, strand != 0)
            out.append(encode_record(b["names"][r], flag, cid(contig), offset - 1, mapq, ops, next_id, pnext - 1, tlen, codes, quals,
                                     strand != 0, t + mate_tags(mate)))
        if lo == hi:
            unmapped += 1
            codes, quals = read_of(r, False)
            flag, ref_id, pos, mate = 0x4, -1, 0, None
            if sam is not None:
                flag = 0x1 | 0x4 | (0x80 if r & 1 else 0x40)
                mlo, mhi = PU.read_records(b, r ^ 1, R)
                for j in range(mlo, mhi):
                    if not int(sam[j][0]) & 0x900:
                        mate = j
                if mate is None:
                    flag |= 0x8
                else:
                    flag |= 0x20 if int(rec[mate][3]) else 0
                    ref_id, pos = cid(rec[mate][4]), int(rec[mate][5])
            out.append(encode_record(b["names"][r], flag, ref_id, pos - 1, 0, [], ref_id, pos - 1, 0, codes, quals, False, mate_tags(mate)))
    off = np.zeros(len(out) + 1, np.int64)
    if out:
        off[1:] = np.cumsum([len(x) for x in out])
    return {"data": np.frombuffer(b"".join(out), np.uint8).copy(), "record_offsets": off,
            "totals": np.array([len(out), int(off[-1]), unmapped], np.int64)}


def agrees(got, want, cap_data=None):
    assert np.array_equal(got["record_offsets"], want["record_offsets"]), (got["record_offsets"][:8], want["record_offsets"][:8])
    if "totals" in got:
        assert got["totals"].tolist() == want["totals"].tolist()
    if "data" in got:
        w = want["data"] if cap_data is None else want["data"][:cap_data]
        assert got["data"].size == w.size, (got["data"].size, w.size)
        bad = np.flatnonzero(got["data"] != w)
        if bad.size:
            at = int(bad[0])
            k = int(np.searchsorted(want["record_offsets"], at, side="right")) - 1
            lo, hi = int(want["record_offsets"][k]), int(want["record_offsets"][k + 1])
            raise AssertionError((f"byte {at}, record {k}, byte {at - lo} of {hi - lo}", bytes(got["data"][lo:hi][:120]), bytes(w[lo:hi][:120])))


# ------------------------------------------------------------------ (b) the decoder
SEQ_LETTERS = "=ACMGRSVTWYHKDBN"
CIGAR_LETTERS = "MIDNSHP=X"


def _bin_by_levels(beg, end):
    """The smallest bin that holds [beg, end): the levels from the finest to the coarsest, each with the number of its first
    bin; 0 is the root."""
    end -= 1
    first, shift = 4681, 14
    while shift <= 26:
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
        shift += 3
        first = (first - 1) // 8
    return 0


def _tags(raw):
    """[(name, type letter, value)] of the tag bytes."""
    out, at = [], 0
    sizes = {"c": ("<b", 1), "C": ("<B", 1), "s": ("<h", 2), "S": ("<H", 2), "i": ("<i", 4), "I": ("<I", 4), "f": ("<f", 4)}
    while at < len(raw):
        name, kind = raw[at:at + 2].decode("latin-1"), chr(raw[at + 2])
        at += 3
        if kind == "A":
            out.append((name, "A", chr(raw[at])))
            at += 1
        elif kind in sizes:
            fmt, n = sizes[kind]
            out.append((name, "f" if kind == "f" else "i", struct.unpack_from(fmt, raw, at)[0]))
            at += n
        elif kind in "ZH":
            end = raw.index(b"\0", at)                               # raises without a terminator
            out.append((name, kind, raw[at:end].decode("latin-1")))
            at = end + 1
        elif kind == "B":
            sub, count = chr(raw[at]), struct.unpack_from("<i", raw, at + 1)[0]
            fmt, n = sizes[sub]
            assert count >= 0 and at + 5 + n * count <= len(raw), "a B array past the record's end"
            out.append((name, "B" + sub, np.frombuffer(raw, np.dtype(fmt), count, at + 5)))
            at += 5 + n * count
        else:
            raise AssertionError(f"tag type {kind!r}")
    assert at == len(raw), "the tags do not end with the record"
    return out


def bam_to_sam(data, contig_names):
    """The SAM lines (without line ends) of a stream of BAM alignment records."""
    on_reference = (0, 2, 3, 7, 8)                                   # M D N = X consume the reference (SAMv1 section 1.4)
    data = bytes(data)
    names = [x.decode("latin-1") if isinstance(x, bytes) else x for x in contig_names]
    lines, at = [], 0
    while at < len(data):
        block_size = struct.unpack_from("<i", data, at)[0]
        assert block_size >= 32 and at + 4 + block_size <= len(data), ("block_size", at, block_size)
        ref_id, pos, l_name, mapq, bin_, n_ops, flag, l_seq, next_id, next_pos, tlen = struct.unpack_from("<iiBBHHHiiii", data, at + 4)
        p = at + 36
        end = at + 4 + block_size
        assert l_name >= 2 and data[p + l_name - 1] == 0 and 0 not in data[p:p + l_name - 1], "read_name and its NUL"
        qname = data[p:p + l_name - 1].decode("latin-1")
        p += l_name
        ops = np.frombuffer(data, "<u4", n_ops, p)
        p += 4 * n_ops
        assert l_seq >= 0 and p + (l_seq + 1) // 2 + l_seq <= end, "SEQ and QUAL past the record's end"
        packed = np.frombuffer(data, np.uint8, (l_seq + 1) // 2, p)
        p += (l_seq + 1) // 2
        qual = np.frombuffer(data, np.uint8, l_seq, p)
        p += l_seq
        tags = _tags(data[p:end])
        real = [t for t in tags if t[0] == "CG"]
        if real:                                                     # SAMv1 4.2.2: the real CIGAR is in the tag
            assert real[0][1] == "BI" and n_ops == 2 and int(ops[0]) == (l_seq << 4 | 4) and int(ops[1]) & 15 == 3
            placeholder = int(ops[1]) >> 4
            ops = real[0][2]
            assert ops.size > 65535 and placeholder == min(int((ops >> 4)[np.isin(ops & 15, on_reference)].sum()), 2**28 - 1)
            tags = [t for t in tags if t[0] != "CG"]
        assert all(int(v) & 15 < 9 for v in ops[:64])
        span = int((ops.astype(np.int64) >> 4)[np.isin(ops & 15, on_reference)].sum())
        assert bin_ == _bin_by_levels(pos, pos + (span or 1)) & 0xffff, ("bin", bin_, pos, span)
        if l_seq & 1:
            assert packed[-1] & 15 == 0, "the unused nibble"
        nibbles = np.stack([packed >> 4, packed & 15], 1).reshape(-1)[:l_seq]
        seq = "".join(SEQ_LETTERS[v] for v in nibbles) if l_seq else "*"
        qtext = "*" if l_seq == 0 or qual[0] == 0xff else bytes((qual + 33).astype(np.uint8)).decode("latin-1")
        cigar = "".join(f"{int(v) >> 4}{CIGAR_LETTERS[int(v) & 15]}" for v in ops) or "*"
        rname = names[ref_id] if ref_id >= 0 else "*"
        rnext = "*" if next_id < 0 else ("=" if next_id == ref_id else names[next_id])
        cols = [qname, flag, rname, pos + 1, mapq, cigar, rnext, next_pos + 1, tlen, seq, qtext]
        cols += [f"{n}:{k}:{v}" for n, k, v in tags]
        lines.append("\t".join(str(c) for c in cols))
        at = end
    return lines


# ------------------------------------------------------------------ the call
def _invoke(lib, ix, b, n_records, ptr, tags, flags, record_offsets, data, cap_data, totals, ws, ws_bytes, stream):
    table = b.get("contig_offsets")
    vp = C.c_void_p
    return lib.genie_bam_records(ix._h, vp(ptr("contig_offsets")), 0 if table is None else table.size - 1, vp(ptr("bases")),
                                 vp(ptr("read_offsets")), b["read_offsets"].size - 1, b["bases"].size, vp(ptr("quals")),
                                 vp(ptr("sel_offsets")), vp(ptr("records")), n_records, vp(ptr("sam")), vp(ptr("info")),
                                 vp(ptr("cigar_offsets")), vp(ptr("cigar")), b["cigar"].size, vp(ptr("names")), vp(ptr("name_offsets")),
                                 sum(len(x) for x in b["names"]), vp(ptr("contig_names")), vp(ptr("contig_name_offsets")),
                                 sum(len(x) for x in b["contig_names"]), tags, flags, vp(record_offsets), vp(data), cap_data, vp(totals),
                                 vp(ws), ws_bytes, vp(stream))


def call(lib, ix, b, tags=NM | AS, flags=0, cap_data=None, n_records=None, totals=True, want_rc=0):
    """The raw calls on torch tensors of the current device, as sam_text_util.call: the sizing call, then the filling call with
    room for cap_data bytes (default: all) -> data (cut to cap_data), record_offsets and totals as host_bam_records returns them."""
    import torch
    dev = "cuda"
    n_records, arrays = ST._arrays(b, n_records)
    N = b["read_offsets"].size - 1
    held = {}
    for name, (a, _) in arrays.items():
        if a is not None:
            held[name] = torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).to(dev) if a.size else \
                torch.zeros(16, dtype=torch.uint8, device=dev)
    ptr = lambda name: held[name].data_ptr() if name in held and (arrays[name][0].size or name in ("quals", "sam")) else 0      # noqa: E731
    ro = torch.full((N + n_records + 1 + 2,), -77, dtype=torch.int64, device=dev)
    tt = torch.full((3,), -77, dtype=torch.int64, device=dev) if totals else None
    wsb = lib.genie_bam_records_workspace_bytes(N, n_records)
    ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device=dev)
    tp = tt.data_ptr() if totals else 0
    rc = _invoke(lib, ix, b, n_records, ptr, tags, flags, ro.data_ptr(), 0, 0, tp, ws.data_ptr(), wsb, 0)
    torch.cuda.synchronize()
    assert rc == want_rc, rc
    if want_rc:
        return None
    sized = ro.cpu().numpy()
    n = int(np.flatnonzero(sized == -77)[0]) - 1
    total = int(sized[n])
    cap = total if cap_data is None else cap_data
    data = torch.full((cap + 64,), 0x7e, dtype=torch.uint8, device=dev)
    ro2 = torch.full_like(ro, -77)
    rc = _invoke(lib, ix, b, n_records, ptr, tags, flags, ro2.data_ptr(), data.data_ptr(), cap, tp, ws.data_ptr(), wsb, 0)
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert np.array_equal(ro2.cpu().numpy(), sized), "the sizing call and the filling call disagree about the offsets"
    assert (data[min(cap, total):] == 0x7e).all(), "bytes at or past min(cap_data, total) were written"
    res = {"data": data[:min(cap, total)].cpu().numpy(), "record_offsets": sized[:n + 1]}
    if totals:
        res["totals"] = tt.cpu().numpy()
    return res


def guarded_call(lib, ix, a, s, b, tags=NM | AS, flags=0, cap_data=0, n_records=None, totals=True, fill=True, want_rc=0):
    """ONE call on the guarded buffers of tests/guarded.py, as sam_text_util.guarded_call -> a contract_calls.Call."""
    import contract_calls as CC
    from guarded import as_numpy
    n_records, arrays = ST._arrays(b, n_records)
    N = b["read_offsets"].size - 1
    addr = {}
    for name, (arr, align) in arrays.items():
        if arr is not None:
            addr[name] = CC._inp(a, name, arr, align)
    ptr = lambda name: addr[name] if name in addr and (arrays[name][0].size or name in ("quals", "sam")) else 0      # noqa: E731
    ro = a.alloc("record_offsets", (N + n_records + 1) * 8, 8)
    data = a.alloc("data", cap_data, 1) if fill else None
    tt = a.alloc("totals", 24, 8) if totals else None
    w, wb = CC._workspace(a, lib.genie_bam_records_workspace_bytes(N, n_records), None)
    rc = _invoke(lib, ix, b, n_records, ptr, tags, flags, a.addr("record_offsets"), a.addr("data") if fill else 0, cap_data,
                 a.addr("totals") if totals else 0, w, wb, s)
    R = clamp(int(b["sel_offsets"][N]), 0, n_records)

    def collect():
        off = as_numpy(ro, np.int64)
        so = np.clip(b["sel_offsets"], 0, R)
        n = R + int((np.diff(so) == 0).sum())
        assert a.holds_poison(ro[(n + 1) * 8:]), "record offsets past n were written"
        res = {"record_offsets": off[:n + 1]}
        if fill:
            got = min(max(int(off[n]), 0), cap_data)
            res["data"] = as_numpy(data, np.uint8)[:got]
            assert a.holds_poison(data[got:]), "bytes past the total were written"
        if totals:
            res["totals"] = as_numpy(tt, np.int64)
        return res
    return CC.Call("bam_records", rc, collect, want_rc)
