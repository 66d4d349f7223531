"""GenieIndex: the device-resident index (suffix array, 2-bit packed reference, P-mer prefix
directory, K-mer table, optional RMI) and the batched entry points of the hot path.

Everything that computes goes through the C ABI (include/genie_smem.h); torch only owns the
device memory, the stream and -- multi-GPU -- the one-time broadcast of the index image.
"""
import ctypes as C
import os
import re
import struct
import zlib
from collections import namedtuple

import numpy as np
import torch

from . import _native as N


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream(device):
    if device.type != "cuda":
        raise RuntimeError("the SMEM hot path runs on an MI355X only (no CPU fallback); tensor is on " + str(device))
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


_CIGAR_LETTERS = {1: "I", 2: "D", 4: "S", 7: "=", 8: "X"}
_CIGAR_OP = re.compile(r"(\d+)([IDS=X])")


def cigar_strings(cigar_offsets, cigar):
    """The CSR of chain_cigars as text, one string per selected chain, such as "3S20=1X5=2D40=" ("" for a chain without ops).
    A host helper: tensors are copied to the host first."""
    off = cigar_offsets.cpu().numpy() if hasattr(cigar_offsets, "cpu") else np.asarray(cigar_offsets)
    if hasattr(cigar, "cpu"):
        cigar = cigar.view(torch.int32).cpu().numpy() if cigar.dtype == torch.uint32 else cigar.cpu().numpy()
    ops = np.asarray(cigar).astype(np.int64) & 0xFFFFFFFF
    return ["".join(f"{int(v) >> 4}{_CIGAR_LETTERS[int(v) & 15]}" for v in ops[int(off[k]):int(off[k + 1])]) for k in range(len(off) - 1)]


def paf_lines(records, info, cigar_offsets, cigar, read_names, read_lengths, contig_names, contig_lengths):
    """The records of select_alignments with chain_cigars' results for its `sel` as PAF text, one line per record: the twelve
    columns (query name, length, start, end in forward read coordinates, strand, target name, length, 0-based start, end,
    matches = n_eq, alignment length = n_eq + n_x + ins_bases + del_bases, mapq), then tp:A:P (primary and supplementary) or
    tp:A:S (secondary), NM:i and cg:Z, the CIGAR without its clips: columns 3 and 4 say them.  A host helper: tensors are
    copied to the host first."""
    host = lambda t: t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)      # noqa: E731
    rec, inf = host(records).reshape(-1, 12), host(info).reshape(-1, 8)
    texts = cigar_strings(cigar_offsets, cigar)
    if not len(rec) == len(inf) == len(texts):
        raise ValueError("records, info and the CIGARs must be parallel: chain_cigars on select_alignments' sel")
    lines = []
    for (read, _, kind, strand, contig, offset, r_span, qb, qe, _, _, mapq), row, text in zip(rec.tolist(), inf.tolist(), texts):
        n_eq, n_x, ins, dele = row[4:8]
        core = "".join(f"{n}{op}" for n, op in _CIGAR_OP.findall(text) if op != "S")
        cols = [read_names[read], int(read_lengths[read]), qb, qe, "-" if strand else "+", contig_names[contig], int(contig_lengths[contig]),
                offset - 1, offset - 1 + r_span, n_eq, n_eq + n_x + ins + dele, mapq, "tp:A:" + ("S" if kind == 2 else "P"),
                f"NM:i:{row[3]}", "cg:Z:" + core]
        lines.append("\t".join(str(c) for c in cols))
    return lines


def sam_header(contig_names, contig_lengths):
    """The header lines of a SAM file for sam_lines: @HD (unsorted, grouped by query), one @SQ per contig, @PG."""
    lines = ["@HD\tVN:1.6\tSO:unsorted\tGO:query"]
    lines += [f"@SQ\tSN:{name}\tLN:{int(length)}" for name, length in zip(contig_names, contig_lengths)]
    return lines + ["@PG\tID:genie-smem_amd\tPN:genie-smem_amd"]


def bam_header(contig_names, contig_lengths):
    """The header of a BAM file (SAMv1 section 4.2) as uncompressed bytes: the magic BAM\\1, l_text, the lines of sam_header
    joined with "\\n" plus a final "\\n", n_ref, and per contig l_name, the name with a NUL and l_ref.  The records of
    GenieIndex.bam_records follow it, and bgzf_compress turns the two into the file.  Names are str (UTF-8) or bytes."""
    names = [x.encode("utf-8") if isinstance(x, str) else bytes(x) for x in contig_names]
    lengths = [int(v) for v in contig_lengths]
    if len(names) != len(lengths):
        raise ValueError("one length per contig name")
    text = ("\n".join(sam_header([x.decode("latin-1") for x in names], lengths)) + "\n").encode("latin-1")
    out = [b"BAM\1", struct.pack("<i", len(text)), text, struct.pack("<i", len(names))]
    for name, length in zip(names, lengths):
        out += [struct.pack("<i", len(name) + 1), name, b"\0", struct.pack("<i", length)]
    return b"".join(out)


BGZF_PAYLOAD = 0xff00                                # input bytes per block: what they deflate to fits 64 KiB at any level
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def _bgzf_block(payload, level):
    z = zlib.compressobj(level, zlib.DEFLATED, -15)
    body = z.compress(payload) + z.flush()
    size = 18 + len(body) + 8                        # the member's header with the BC subfield, the body, CRC32 and ISIZE
    if size > 0x10000:
        raise ValueError("a BGZF block above 64 KiB")
    return b"".join([b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0", struct.pack("<H", size - 1), body,
                     struct.pack("<II", zlib.crc32(payload) & 0xffffffff, len(payload))])


def bgzf_blocks(buffers, level=1, threads=None):
    """The BGZF blocks of the concatenation of `buffers` (bytes or anything with the buffer interface), in order, the EOF block
    last: a generator, so that a writer holds a few blocks at a time and the buffers are never joined.  See bgzf_compress."""
    views = [memoryview(x).cast("B") for x in buffers]
    views = [v for v in views if len(v)]
    if threads is None:
        env = os.environ.get("OMP_NUM_THREADS", "")
        threads = int(env) if env.isdigit() and int(env) > 0 else min(4, os.cpu_count() or 1)

    def pieces():
        carry = b""                                  # the tail of a buffer that did not fill a payload: copied, below 0xff00 bytes
        for v in views:
            at = 0
            if carry:
                at = min(BGZF_PAYLOAD - len(carry), len(v))
                carry += bytes(v[:at])
                if len(carry) < BGZF_PAYLOAD:
                    continue
                yield carry
                carry = b""
            whole = at + (len(v) - at) // BGZF_PAYLOAD * BGZF_PAYLOAD
            for k in range(at, whole, BGZF_PAYLOAD):
                yield v[k:k + BGZF_PAYLOAD]
            carry = bytes(v[whole:])
        if carry:
            yield carry

    threads = max(1, int(threads)) if sum(len(v) for v in views) > BGZF_PAYLOAD else 1      # no pool for one block
    if threads == 1:
        for x in pieces():
            yield _bgzf_block(x, level)
    else:
        from collections import deque
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(threads) as pool:
            pending = deque()                        # at most four blocks per thread in flight, taken in order
            for x in pieces():
                pending.append(pool.submit(_bgzf_block, x, level))
                if len(pending) >= 4 * threads:
                    yield pending.popleft().result()
            while pending:
                yield pending.popleft().result()
    yield BGZF_EOF


def bgzf_compress(data, level=1, threads=None):
    """data (bytes or any buffer) as a BGZF stream (SAMv1 section 4.1): cut into payloads of at most 0xff00 bytes, each one
    gzip member with the BC extra subfield (BSIZE = the member's length - 1), raw deflate at `level`, CRC32 and ISIZE; then
    the 28-byte EOF block.  The blocks are independent and zlib releases the GIL, so a pool of `threads` compresses them: by
    default OMP_NUM_THREADS when that is set, else min(4, the CPUs there are).  The result does not depend on it."""
    return b"".join(bgzf_blocks([data], level, threads))


_COMPLEMENT = str.maketrans("ACGTNacgtn", "TGCANtgcan")


def sam_lines(records, sam, info, cigar_offsets, cigar, read_names, contig_names, seqs=None, quals=None):
    """The records of an interleaved batch of mates (map_pairs) as SAM text: one line per record, read by read in record
    order -- QNAME, FLAG and MAPQ from pair_alignments' `sam`, RNAME, POS (the record's 1-based offset), the chain's CIGAR
    with its clips, RNEXT (`=`, a contig name or `*`) and PNEXT from mate_record, TLEN, SEQ and QUAL (`*` when not given;
    given in read orientation, they are turned for strand 1), NM:i and AS:i -- and, for a read without records, the unmapped
    line: flag 0x4 plus the pair bits, placed at its mate's position if the mate is mapped.  read_names has one name per read;
    reads 2k and 2k + 1 are mates.  A host helper: tensors are copied to the host first."""
    host = lambda t: t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)      # noqa: E731
    rec, fields, inf = host(records).reshape(-1, 12).tolist(), host(sam).reshape(-1, 4).tolist(), host(info).reshape(-1, 8).tolist()
    texts = cigar_strings(cigar_offsets, cigar)
    if not len(rec) == len(fields) == len(inf) == len(texts):
        raise ValueError("records, sam, info and the CIGARs must be parallel: map_pairs' results")
    if len(read_names) % 2:
        raise ValueError("an even number of reads: reads 2k and 2k + 1 are mates")
    by_read, chosen = [[] for _ in read_names], {}
    for j, (row, field) in enumerate(zip(rec, fields)):
        by_read[row[0]].append(j)
        if not field[0] & 0x900:
            chosen[row[0]] = j

    def seq_qual(read, strand):
        seq = seqs[read] if seqs is not None else "*"
        qual = quals[read] if quals is not None else "*"
        if strand:
            seq = seq if seq == "*" else seq.translate(_COMPLEMENT)[::-1]
            qual = qual if qual == "*" else qual[::-1]
        return [seq, qual]

    lines = []
    for read, name in enumerate(read_names):
        for j in by_read[read]:
            _, _, _, strand, contig, offset, _, _, _, score, _, _ = rec[j]
            flag, mapq, mate, tlen = fields[j]
            rnext, pnext = "*", 0
            if mate >= 0:
                rnext, pnext = "=" if rec[mate][4] == contig else contig_names[rec[mate][4]], rec[mate][5]
            cols = [name, flag, contig_names[contig], offset, mapq, texts[j] or "*", rnext, pnext, tlen] + seq_qual(read, strand)
            lines.append("\t".join(str(c) for c in cols + [f"NM:i:{inf[j][3]}", f"AS:i:{score}"]))
        if not by_read[read]:
            flag, rname, pos, rnext = 0x1 | 0x4 | (0x80 if read & 1 else 0x40), "*", 0, "*"
            mate = chosen.get(read ^ 1)
            if mate is None:
                flag |= 0x8
            else:
                flag |= 0x20 if rec[mate][3] else 0
                rname, pos, rnext = contig_names[rec[mate][4]], rec[mate][5], "="
            lines.append("\t".join(str(c) for c in [name, flag, rname, pos, 0, "*", rnext, pos, 0] + seq_qual(read, 0)))
    return lines


InsertSize = namedtuple("InsertSize", "orient isize_min isize_max isize_mean estimated stats")
_PAIR_DEFAULTS = {"orient": "fr", "isize_min": 0, "isize_max": 1000, "isize_mean": 300}      # GenieIndex.pair_alignments'


def insert_size_options(stats, fallback=None):
    """The pairing options that insert_size_stats' statistics stand for -> InsertSize(orient, isize_min, isize_max, isize_mean,
    estimated, stats).  A host function: stats is int64[3, 12] as a CPU tensor or an array, one row per type (FR, RF, same) =
    (n, ok, q25, q50, q75, lo_b, hi_b, n_in, mean, std, isize_min, isize_max).  The ok type with the most samples gives its
    bit as orient (pair_alignments' mask), its window and its mean, and estimated is True; a tie goes to the lower type.  With
    no ok type the four values are the fallback's -- a dict of pair_alignments' options, those it lacks being that call's
    defaults -- and estimated is False.  ONE orientation: a window per orientation would need another pairing call.  stats
    comes back as a tuple of three tuples."""
    rows = np.asarray(stats.cpu() if hasattr(stats, "cpu") else stats, dtype=np.int64).reshape(3, 12)
    kept = tuple(tuple(int(v) for v in row) for row in rows)
    best = None
    for t in range(3):
        if kept[t][1] and (best is None or kept[t][0] > kept[best][0]):
            best = t
    if best is not None:
        return InsertSize(1 << best, kept[best][10], kept[best][11], kept[best][8], True, kept)
    opts = dict(_PAIR_DEFAULTS, **{k: v for k, v in (fallback or {}).items() if k in _PAIR_DEFAULTS})
    orient = N.PAIR_ORIENT[opts["orient"]] if isinstance(opts["orient"], str) else int(opts["orient"])
    return InsertSize(orient, int(opts["isize_min"]), int(opts["isize_max"]), int(opts["isize_mean"]), False, kept)


def names_csr(names, device=None):
    """Names that come from the host as sam_text takes them: a list of str (UTF-8) or bytes -> (bytes uint8[total], offsets
    int64[len(names) + 1]), two tensors on the host or, with `device`, there.  An empty list gives no bytes and the offset 0."""
    raw = [x.encode("utf-8") if isinstance(x, str) else bytes(x) for x in names]
    offsets = np.zeros(len(raw) + 1, np.int64)
    if raw:
        offsets[1:] = np.cumsum([len(x) for x in raw])
    data = torch.from_numpy(np.frombuffer(b"".join(raw), np.uint8).copy())
    offsets = torch.from_numpy(offsets)
    return (data, offsets) if device is None else (data.to(device), offsets.to(device))


class GenieIndex:
    def __init__(self):
        self._h = C.c_void_p(0)
        self.blob = None            # torch uint8 tensor holding the device image (keeps it alive)
        self._host_blob = None
        self.device = None

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                N.lib().genie_index_destroy(h)
            except Exception:  # noqa: BLE001 - interpreter shutdown
                pass

    # ------------------------------------------------------------------ construction (host)
    @classmethod
    def build(cls, codes, K, dir_bits=7, sa_one_based=None, table_bits=0, table_format="auto"):
        """codes: uint8 array of base codes 0..3; K: LUT / RMI key size (0 = none);
        sa_one_based: adopt this suffix array (reference JSON convention) instead of building;
        table_bits: P2 of the per-P2-mer tables (0 = automatic); table_format: "auto" (compact 16-byte entries below 2^24
        bases), "wide" or "compact" -- tuning knobs of the index image only."""
        codes = np.ascontiguousarray(codes, np.uint8)
        self = cls()
        u8p = C.POINTER(C.c_uint8)
        sa_p = None
        if sa_one_based is not None:
            sa = np.ascontiguousarray(sa_one_based, np.int32)
            if sa.size != codes.size + 1:
                raise ValueError("suffix array must have n+1 rows")
            sa_p = sa.ctypes.data_as(C.POINTER(C.c_int32))
        fmt = {"auto": 0, "wide": N.TABLE_WIDE, "compact": N.TABLE_COMPACT}[table_format]
        rc = N.lib().genie_index_create_ex(codes.ctypes.data_as(u8p), codes.size, sa_p, int(K), int(dir_bits),
                                           int(table_bits) | fmt, C.byref(self._h))
        N.check(rc, "genie_index_create")
        return self

    @classmethod
    def build_on_device(cls, codes, K, dir_bits=7, table_bits=0, table_format="auto", seed_table=True, device="cuda"):
        """Build the index image on the GPU (genie_index_create_device): the same image bytes as
        build(...).serialize(seed_table), written straight into device memory and bound like to() does.
        codes: numpy array or torch tensor of base codes 0..3 (uploaded if it is on the host).  The handle is
        device-only: no host arrays and no RMI model (RMI mode gives GENIE_E_NO_MODEL)."""
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("GenieIndex.build_on_device: an MI355X device is required (no CPU fallback)")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if not isinstance(codes, torch.Tensor):
            codes = torch.as_tensor(np.ascontiguousarray(codes, np.uint8))
        codes = codes.to(device=device, dtype=torch.uint8).contiguous().view(-1)
        n = codes.numel()
        tb = int(table_bits) | {"auto": 0, "wide": N.TABLE_WIDE, "compact": N.TABLE_COMPACT}[table_format]
        L = N.lib()
        cap = int(L.genie_index_device_image_bound(n, int(K), int(dir_bits), tb))
        tmp_bytes = int(L.genie_index_device_build_tmp_bytes(n, int(K), int(dir_bits), tb))
        if cap < 0 or tmp_bytes < 0:
            raise N.GenieError(min(cap, tmp_bytes), "genie_index_device_image_bound")
        image = torch.empty(cap, dtype=torch.uint8, device=device)     # torch allocations are 512-byte aligned
        tmp = torch.empty(tmp_bytes, dtype=torch.uint8, device=device)
        nbytes = C.c_int64(0)
        self = cls()
        with torch.cuda.device(device):
            rc = L.genie_index_create_device(_ptr(codes), n, int(K), int(dir_bits), tb,
                                             0 if seed_table else N.IMAGE_NO_SEED_TABLE, _ptr(image), cap, C.byref(nbytes),
                                             _ptr(tmp), tmp_bytes, device.index, _stream(device), C.byref(self._h))
        N.check(rc, "genie_index_create_device")
        del tmp
        # keep only the image itself (a copy, so the bound-sized buffer is released), then bind it as to() does
        blob = image[:nbytes.value].clone()
        del image
        self._bind(blob, blob[:N.HEADER_BYTES].cpu())
        return self

    def set_rmi(self, experts, coefs, icpts):
        """experts: the reference's list (RMI.experts); coefs/icpts: per-level float64 arrays."""
        sizes = np.asarray([len(c) for c in coefs], np.int32)
        scales = np.asarray(list(experts) + [1], np.int32)
        if len(sizes) != len(scales):
            raise ValueError("need len(experts)+1 levels of coefficients")
        coef = np.ascontiguousarray(np.concatenate([np.asarray(c, np.float64) for c in coefs]))
        icpt = np.ascontiguousarray(np.concatenate([np.asarray(c, np.float64) for c in icpts]))
        i32p, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
        N.check(N.lib().genie_index_set_rmi(self._h, len(sizes), sizes.ctypes.data_as(i32p),
                                            scales.ctypes.data_as(i32p), coef.ctypes.data_as(dp),
                                            icpt.ctypes.data_as(dp)), "genie_index_set_rmi")
        self._host_blob = None

    def train_rmi(self, experts):
        """Native RMI training (genie_index_train_rmi; RMI_LUT.train_RMI + RMI.fit without scikit-learn).
        Returns (coefs, icpts, leaf_err, mean_abs_err, max_abs_err): per-level float64 arrays, the
        per-leaf error bounds, and the error statistics over the training pairs."""
        ex = np.asarray(list(experts), np.int32)
        mean = C.c_double(0.0)
        worst = C.c_int32(0)
        N.check(N.lib().genie_index_train_rmi(self._h, len(ex), ex.ctypes.data_as(C.c_void_p), C.byref(mean),
                                              C.byref(worst)), "genie_index_train_rmi")
        self._host_blob = None
        sizes = [1] + [int(e) for e in ex]
        coef = np.empty(sum(sizes), np.float64)
        icpt = np.empty(sum(sizes), np.float64)
        err = np.empty(sizes[-1], np.int32)
        N.check(N.lib().genie_index_rmi_models(self._h, coef.ctypes.data_as(C.c_void_p), icpt.ctypes.data_as(C.c_void_p),
                                               err.ctypes.data_as(C.c_void_p)), "genie_index_rmi_models")
        cuts = np.cumsum([0] + sizes)
        coefs = [coef[cuts[i]:cuts[i + 1]].copy() for i in range(len(sizes))]
        icpts = [icpt[cuts[i]:cuts[i + 1]].copy() for i in range(len(sizes))]
        return coefs, icpts, err, float(mean.value), int(worst.value)

    def info(self):
        inf = N.GenieInfo()
        N.check(N.lib().genie_index_info(self._h, C.byref(inf)), "genie_index_info")
        return {f: getattr(inf, f) for f, _ in N.GenieInfo._fields_}

    @property
    def n(self):
        return self.info()["n"]

    @property
    def K(self):
        return self.info()["K"]

    def suffix_array(self):
        """1-based suffix array as the reference stores it (row 0 = n+1); host copy."""
        p = N.lib().genie_index_suffix_array(self._h)
        if not p:
            raise RuntimeError("this handle has no host arrays (opened from a broadcast image)")
        return np.ctypeslib.as_array(p, (self.n + 1,))

    def lut_arrays(self):
        """Sorted distinct K-mer codes and their inclusive SA intervals (host views)."""
        cp, lp, hp = C.POINTER(C.c_uint32)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)()
        N.check(N.lib().genie_index_lut_arrays(self._h, C.byref(cp), C.byref(lp), C.byref(hp)), "genie_index_lut_arrays")
        m = self.info()["lut_keys"]
        if m == 0:
            return np.zeros(0, np.uint32), np.zeros(0, np.int32), np.zeros(0, np.int32)
        return (np.ctypeslib.as_array(cp, (m,)), np.ctypeslib.as_array(lp, (m,)), np.ctypeslib.as_array(hp, (m,)))

    # ------------------------------------------------------------------ image / device
    def serialize(self, seed_table=True):
        """The flat index image as a CPU uint8 tensor (header + sections).  seed_table=False leaves out the K-mer hash
        table (GENIE_IMAGE_NO_SEED_TABLE): the image of a rank that only finds SMEMs."""
        if not seed_table:
            nbytes = N.lib().genie_index_image_bytes(self._h, N.IMAGE_NO_SEED_TABLE)
            if nbytes <= 0:
                raise N.GenieError(int(nbytes), "genie_index_image_bytes")
            buf = torch.empty(nbytes, dtype=torch.uint8)
            N.check(N.lib().genie_index_serialize_image(self._h, N.IMAGE_NO_SEED_TABLE, C.c_void_p(buf.data_ptr()), nbytes),
                    "genie_index_serialize_image")
            return buf
        if self._host_blob is None:
            nbytes = N.lib().genie_index_blob_bytes(self._h)
            if nbytes <= 0:
                raise N.GenieError(int(nbytes), "genie_index_blob_bytes")
            buf = torch.empty(nbytes, dtype=torch.uint8)
            N.check(N.lib().genie_index_serialize(self._h, C.c_void_p(buf.data_ptr()), nbytes), "genie_index_serialize")
            self._host_blob = buf
        return self._host_blob

    def to(self, device, seed_table=True):
        """Upload the image with torch and bind it (torch owns the device memory)."""
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("GenieIndex.to: an MI355X device is required (no CPU fallback)")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        host = self.serialize(seed_table)
        self._bind(host.to(device), host[:N.HEADER_BYTES])
        return self

    def _bind(self, dev_blob, host_header):
        host_header = host_header.contiguous()
        dev_index = dev_blob.device.index if dev_blob.device.type == "cuda" else -1
        N.check(N.lib().genie_index_open(C.c_void_p(host_header.data_ptr()), C.c_void_p(dev_blob.data_ptr()),
                                         dev_blob.numel(), dev_index, C.byref(self._h)), "genie_index_open")
        self.blob = dev_blob
        self.device = dev_blob.device
        if dev_blob.device.type == "cuda":
            # the header was checked by open; the contents (row numbers, entry links) on the device, once
            what = C.c_uint32(0)
            with torch.cuda.device(self.device):
                rc = N.lib().genie_index_validate(self._h, C.byref(what), _stream(self.device))
            if rc:
                self.blob = None
                raise N.GenieError(rc, f"genie_index_validate (sections {what.value:#x})")

    @classmethod
    def from_image(cls, dev_blob):
        """Open an image that already sits in device memory (e.g. received by broadcast)."""
        self = cls()
        self._bind(dev_blob, dev_blob[:N.HEADER_BYTES].cpu())
        return self

    # ------------------------------------------------------------------ hot path
    def _need_device(self):
        if self.blob is None or self.device is None or self.device.type != "cuda":
            raise RuntimeError("index is not on a GPU: call GenieIndex.to('cuda') first (no CPU fallback)")

    def _as_dev(self, t, dtype):
        if not isinstance(t, torch.Tensor):
            t = torch.as_tensor(np.ascontiguousarray(t))
        t = t.to(device=self.device, dtype=dtype)
        return t.contiguous()

    def _batch(self, reads, lens, names=("reads", "read")):
        """A batch of [N, stride] uint8 codes and its optional int32 lengths on the device -> (reads, lens, N, stride,
        fixed): fixed is the longest length, or stride without lengths."""
        self._need_device()
        reads = self._as_dev(reads, torch.uint8)
        if reads.dim() != 2:
            raise ValueError(f"{names[0]} must be [N, stride]")
        n, stride = reads.shape
        fixed = stride
        if lens is not None:
            lens = self._as_dev(lens, torch.int32)
            fixed = int(lens.max().item()) if n else 0
            if fixed > stride or (n and int(lens.min().item()) < 0):
                raise ValueError(f"{names[1]} length outside [0, stride]")
        return reads, lens, n, stride, fixed

    @staticmethod
    def _bwa_if_split(mode, split_breaks):
        if split_breaks and mode != "bwa":
            raise ValueError("split_breaks needs mode 'bwa' (genie_find_smems_split has no other traversal)")

    def _workspace(self, size_fn, *args):
        """(device buffer, bytes) of the workspace the C size function `size_fn` asks for."""
        nbytes = int(getattr(N.lib(), size_fn)(*args))
        if nbytes < 0:
            raise N.GenieError(nbytes, size_fn)
        return torch.empty(max(nbytes, 256), dtype=torch.uint8, device=self.device), nbytes

    def _run(self, name, *args):
        """Call the C entry point `name` on this handle with `args`, on the current stream of the index's device."""
        with torch.cuda.device(self.device):
            N.check(getattr(N.lib(), name)(self._h, *args, _stream(self.device)), name)

    def _run_csr(self, name, head, n_rows, cap_rows, tail):
        """Run a CSR entry point, name(handle, *head, offsets, rows, rows capacity, status, *tail, stream), with room for
        `cap_rows` rows, rerun with the exact size if they do not fit -> (offsets int64[n_rows+1], smems int32[S,4], status)."""
        offsets = torch.empty(n_rows + 1, dtype=torch.int64, device=self.device)
        status = torch.empty(n_rows, dtype=torch.int32, device=self.device)
        while True:
            rows = torch.empty((max(cap_rows, 1), 4), dtype=torch.int32, device=self.device)
            self._run(name, *head, _ptr(offsets), _ptr(rows), rows.shape[0], _ptr(status), *tail)
            total = int(offsets[-1].item())
            if total <= rows.shape[0]:
                return offsets, rows[:total], status
            cap_rows = total                      # capacity guess too small: rerun with the exact size

    def sa_interval(self, pats, lens=None):
        """Batched exact_match_back_prop.  pats: [N, stride] uint8 codes; lens: [N] or None.
        Returns int32 [N, 2] (lo, hi); (-1,-1) absent; (-2,-2) code > 3."""
        pats, lens, n_pat, stride, fixed = self._batch(pats, lens, ("pats", "pattern"))
        if stride == 0:
            pats = torch.zeros((n_pat, 1), dtype=torch.uint8, device=self.device)
            stride = 1
        out = torch.empty((n_pat, 2), dtype=torch.int32, device=self.device)
        self._run("genie_sa_interval", _ptr(pats), _ptr(lens), n_pat, stride, fixed, _ptr(out))
        return out

    def seed_lookup(self, mode, kmers, want_pred=False):
        """Batched K-mer seed lookup (LUT membership / RMI get_suffix_rmi). kmers: [N, K] codes."""
        self._need_device()
        kmers = self._as_dev(kmers, torch.uint8)
        if kmers.dim() != 2 or kmers.shape[1] != self.K:
            raise ValueError("kmers must be [N, K]")
        out = torch.empty((kmers.shape[0], 2), dtype=torch.int32, device=self.device)
        pred = torch.empty(kmers.shape[0], dtype=torch.float64, device=self.device) if want_pred else None
        self._run("genie_seed_lookup", N.MODES[mode], _ptr(kmers), kmers.shape[0], _ptr(out), _ptr(pred))
        return (out, pred) if want_pred else out

    def find_smems_slots(self, mode, reads, lens=None, min_len=1, cap=None):
        """One launch of the SMEM kernel.  reads: [N, stride] uint8 codes on the device.
        Returns (counts int32[N], slots int32[N, cap, 4], status int32[N])."""
        reads, lens, n_reads, stride, fixed = self._batch(reads, lens)
        if cap is None:
            cap = max(1, fixed)
        counts = torch.empty(n_reads, dtype=torch.int32, device=self.device)
        slots = torch.empty((n_reads, cap, 4), dtype=torch.int32, device=self.device)
        status = torch.empty(n_reads, dtype=torch.int32, device=self.device)
        if n_reads == 0 or stride == 0:
            counts.zero_()
            status.zero_()
            return counts, slots, status
        ws, ws_bytes = self._workspace("genie_find_smems_workspace_bytes", n_reads, fixed)
        self._run("genie_find_smems", N.MODES[mode], _ptr(reads), _ptr(lens), n_reads, stride, fixed, int(min_len),
                  _ptr(counts), _ptr(slots), cap, _ptr(status), _ptr(ws), ws_bytes)
        return counts, slots, status

    def compact(self, counts, slots, out=None):
        """Slotted output -> CSR: (offsets int64[N+1], smems int32[S, 4])."""
        self._need_device()
        n_reads, cap = slots.shape[0], slots.shape[1]
        offsets = torch.empty(n_reads + 1, dtype=torch.int64, device=self.device)
        tmp = torch.empty(max(int(N.lib().genie_compact_tmp_bytes(n_reads)), 16), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            st = _stream(self.device)
            if out is None:
                N.check(N.lib().genie_compact_smems(_ptr(counts), _ptr(slots), n_reads, cap, _ptr(offsets),
                                                    C.c_void_p(0), 0, _ptr(tmp), st), "genie_compact_smems")
                total = int(offsets[-1].item())
                out = torch.empty((max(total, 1), 4), dtype=torch.int32, device=self.device)
            N.check(N.lib().genie_compact_smems(_ptr(counts), _ptr(slots), n_reads, cap, _ptr(offsets), _ptr(out),
                                                out.shape[0], _ptr(tmp), st), "genie_compact_smems")
        return offsets, out

    def locate(self, intervals, sort=False):
        """Rows -> reference coordinates for a batch of SA intervals (ExactMatch.get_positions,
        ExactMatch.py:195-199): `intervals` is int32 [S, 2] (lo, hi) -- a sa_interval result -- or
        int32 [S, 4] (start, end, lo, hi) -- find_smems rows.  Returns (pos_offsets int64[S+1],
        positions int32[T]): 1-based positions in row order, or ascending per interval with sort=True
        (ExactMatch.exact_match's order, :174-192)."""
        self._need_device()
        iv = self._as_dev(intervals, torch.int32)
        if iv.dim() != 2 or iv.shape[1] not in (2, 4):
            raise ValueError("intervals must be [S, 2] (lo, hi) or [S, 4] (start, end, lo, hi)")
        iv = iv.contiguous()
        S, width = iv.shape
        offsets = torch.empty(S + 1, dtype=torch.int64, device=self.device)
        tmp, tmp_bytes = self._workspace("genie_locate_tmp_bytes", S)
        base = C.c_void_p(iv.data_ptr() + (8 if width == 4 else 0))
        self._run("genie_locate", base, width, S, _ptr(offsets), C.c_void_p(0), 0, _ptr(tmp), tmp_bytes)
        total = int(offsets[-1].item())
        pos = torch.empty(max(total, 1), dtype=torch.int32, device=self.device)
        self._run("genie_locate", base, width, S, _ptr(offsets), _ptr(pos), total, _ptr(tmp), tmp_bytes)
        pos = pos[:total]
        if sort and total:
            # ascending inside every interval: one sort on (interval, position) keys -- torch plumbing
            seg = torch.repeat_interleave(torch.arange(S, device=self.device), offsets[1:] - offsets[:-1])
            key = seg * (int(self.info()["n"]) + 2) + pos.to(torch.int64)
            pos = pos[torch.argsort(key)]
        return offsets, pos

    def find_smems(self, mode, reads, lens=None, min_len=1, cap=None, rows_hint=None):
        """Batched SMEM discovery -> (offsets int64[N+1], smems int32[S,4] = (start,end,lo,hi), status).
        Uses the fused CSR entry point (genie_find_smems_csr) unless an explicit slot capacity is asked for."""
        reads, lens, n_reads, stride, fixed = self._batch(reads, lens)
        if cap is not None or n_reads == 0 or stride == 0:
            counts, slots, status = self.find_smems_slots(mode, reads, lens, min_len, cap)
            offsets, out = self.compact(counts, slots)
            total = int(offsets[-1].item())
            return offsets, out[:total], status
        ws, ws_bytes = self._workspace("genie_find_smems_workspace_bytes", n_reads, fixed)
        return self._run_csr("genie_find_smems_csr", (N.MODES[mode], _ptr(reads), _ptr(lens), n_reads, stride, fixed,
                                                      int(min_len)),
                             n_reads, int(rows_hint) if rows_hint else n_reads * max(8, fixed // 6), (_ptr(ws), ws_bytes))

    def find_smems_both(self, mode, reads, lens=None, min_len=1, rows_hint=None):
        """SMEMs of both strands of every read (genie_find_smems_both) -> (offsets int64[2N+1], smems int32[S,4], status
        int32[2N]).  Strand-read 2i is read i, 2i + 1 its reverse complement (packing.reverse_complement); the result is that
        of find_smems on the interleaved batch [r0, rc(r0), r1, rc(r1), ...], with start / end of a strand-1 row positions in
        the reverse-complemented read (forward coordinates: L - end, L - start).  reads: [N, stride] uint8 codes (device or
        host: uploaded as uint8 codes)."""
        reads, lens, n_reads, stride, fixed = self._batch(reads, lens)
        if stride == 0:
            reads = torch.zeros((n_reads, 1), dtype=torch.uint8, device=self.device)
            stride = 1
        ws, ws_bytes = self._workspace("genie_find_smems_both_workspace_bytes", n_reads, fixed)
        return self._run_csr("genie_find_smems_both", (N.MODES[mode], _ptr(reads), _ptr(lens), n_reads, stride, fixed,
                                                       int(min_len)),
                             2 * n_reads, int(rows_hint) if rows_hint else 2 * n_reads * max(8, fixed // 6),
                             (_ptr(ws), ws_bytes))

    def find_smems_split(self, reads, lens=None, min_len=1, rows_hint=None):
        """SMEMs of reads that may contain breaks (genie_find_smems_split) -> (offsets int64[N+1], smems int32[S,4], status).
        reads: [N, stride] uint8 codes on the device or the host (uploaded as uint8 codes: the 2-bit packed host path cannot
        carry a break).  A break is any code > 3 or a base that never occurs in the reference; the SMEMs of a read are those
        of its segments (the runs between breaks), in read order, each found like get_SMEMS with min_len, with start / end
        positions in the whole read.  A read of length 0 or made only of breaks has no rows and status 0."""
        reads, lens, n_reads, stride, fixed = self._batch(reads, lens)
        if stride == 0:
            reads = torch.zeros((n_reads, 1), dtype=torch.uint8, device=self.device)
            stride = 1
        ws, ws_bytes = self._workspace("genie_find_smems_split_workspace_bytes", n_reads, fixed)
        return self._run_csr("genie_find_smems_split", (_ptr(reads), _ptr(lens), n_reads, stride, fixed, int(min_len)),
                             n_reads, int(rows_hint) if rows_hint else n_reads * max(8, fixed // 6), (_ptr(ws), ws_bytes))

    def find_smems_long(self, mode, bases, read_offsets, min_len=1, rows_hint=None, both_strands=False, split_breaks=False):
        """SMEMs of reads of any length (genie_find_smems_long) -> (offsets int64[N+1], smems int32[S,4], status).
        bases: uint8 codes of all reads back to back; read_offsets: int64[N+1], read r = bases[read_offsets[r] ..
        read_offsets[r+1]).  Either may be on the device or the host.  Rows and status as find_smems.
        both_strands / split_breaks (genie_find_smems_long_ex): with both_strands the result covers 2N strand-reads,
        interleaved as find_smems_both (2i is read i, 2i + 1 its reverse complement, rows in its own coordinates); with
        split_breaks (mode "bwa" only) codes > 3 and bases the reference lacks cut a strand-read into segments, as
        find_smems_split."""
        self._bwa_if_split(mode, split_breaks)
        bases, read_offsets, n_reads, total, max_len, flags, strands = self._csr_call(bases, read_offsets, both_strands, split_breaks)
        if not flags:
            ws, ws_bytes = self._workspace("genie_find_smems_long_workspace_bytes", n_reads, total, max_len)
            return self._run_csr("genie_find_smems_long", (N.MODES[mode], _ptr(bases), _ptr(read_offsets), n_reads, total,
                                                           max_len, int(min_len)),
                                 n_reads, int(rows_hint) if rows_hint else max(8 * n_reads, total // 6), (_ptr(ws), ws_bytes))
        ws, ws_bytes = self._workspace("genie_find_smems_long_ex_workspace_bytes", n_reads, total, max_len, flags)
        return self._run_csr("genie_find_smems_long_ex", (N.MODES[mode], flags, _ptr(bases), _ptr(read_offsets), n_reads, total,
                                                          max_len, int(min_len)),
                             strands * n_reads, int(rows_hint) if rows_hint else strands * max(8 * n_reads, total // 6),
                             (_ptr(ws), ws_bytes))

    def match_stats(self, bases, read_offsets, intervals=True, both_strands=False, split_breaks=False):
        """Matching statistics of every position of every read (genie_match_stats) -> (ms int32[S*total], lohi
        int32[S*total, 2] or None, status int32[S*N]) on the device, S = 2 with both_strands, else 1.  bases / read_offsets
        as find_smems_long.  Position p of strand-read S*i + s is element S*read_offsets[i] + s*L_i + p: ms = the length of the
        longest match that starts there (0: none; -1 throughout a strand-read flagged READ_BAD_BASE), lohi its inclusive
        suffix-array interval ((-1, -1) where there is none; not computed with intervals=False).  With split_breaks codes
        > 3 and bases the reference lacks are breaks that no match covers, and every status is READ_OK."""
        bases, read_offsets, n_reads, total, max_len, flags, strands = self._csr_call(bases, read_offsets, both_strands, split_breaks)
        ms =torch.empty(strands * total, dtype=torch.int32, device=self.device)
        lohi = torch.empty((strands * total, 2), dtype=torch.int32, device=self.device) if intervals else None
        status = torch.empty(strands * n_reads, dtype=torch.int32, device=self.device)
        ws, ws_bytes = self._workspace("genie_match_stats_workspace_bytes", n_reads, total, max_len, flags)
        self._run("genie_match_stats", flags, _ptr(bases), _ptr(read_offsets), n_reads, total, max_len, _ptr(ms), _ptr(lohi),
                  _ptr(status), _ptr(ws), ws_bytes)
        return ms, lohi, status

    def find_mems(self, bases, read_offsets, min_len, both_strands=False, split_breaks=False, max_occ=0, rows_hint=None):
        """Every maximal exact match of at least min_len bases (genie_find_mems) -> (offsets int64[S*N+1], mems
        int32[R, 4] = (start, end, pos, row), status int32[S*N], skipped int) on the device, S = 2 with both_strands, else
        1.  bases / read_offsets, the strand-reads, breaks and status as match_stats.  A row says that the strand-read's
        bases [start, end) equal the reference's from the 1-based position pos on (the suffix of suffix-array row `row`) and
        that neither side can be extended.  The rows of a strand-read are ordered by (start, row).  max_occ > 0 skips every
        position whose first min_len bases occur more than max_occ times in the reference; `skipped` counts them.  If the
        rows outnumber rows_hint the call is made again with room for all."""
        return self._find_mems("genie_find_mems", (), (), bases, read_offsets, min_len, both_strands, split_breaks, max_occ, rows_hint)

    def _find_mems(self, name, table, size_tail, bases, read_offsets, min_len, both_strands, split_breaks, max_occ, rows_hint):
        """genie_find_mems or genie_find_mems_contigs: `table` are the arguments between the handle and the flags,
        `size_tail` those the workspace function takes behind the flags."""
        bases, read_offsets, n_reads, total, max_len, flags, strands = self._csr_call(bases, read_offsets, both_strands, split_breaks)
        offsets =torch.empty(strands * n_reads + 1, dtype=torch.int64, device=self.device)
        status = torch.empty(strands * n_reads, dtype=torch.int32, device=self.device)
        totals = torch.empty(2, dtype=torch.int64, device=self.device)
        ws, ws_bytes = self._workspace(name + "_workspace_bytes", n_reads, total, max_len, flags, *size_tail)
        cap_rows = int(rows_hint) if rows_hint else strands * max(8 * n_reads, total)
        while True:
            rows = torch.empty((max(cap_rows, 1), 4), dtype=torch.int32, device=self.device)
            self._run(name, *table, flags, _ptr(bases), _ptr(read_offsets), n_reads, total, max_len, int(min_len),
                      int(max_occ), _ptr(offsets), _ptr(rows), rows.shape[0], _ptr(status), _ptr(totals), _ptr(ws), ws_bytes)
            found, skipped = (int(x) for x in totals.tolist())
            if found <= rows.shape[0]:
                return offsets, rows[:found], status, skipped
            cap_rows = found                      # capacity guess too small: rerun with the exact size

    def _contig_table(self, contigs):
        """The (pointer, count) of a ReferenceSet's table on this index's device; it must be the table of this reference."""
        self._need_device()
        off = contigs.device_offsets(self.device)
        if int(contigs.offsets[-1]) != self.n:
            raise ValueError(f"the contig table ends at {int(contigs.offsets[-1])}, the index holds {self.n} bases")
        return off, (_ptr(off), off.numel() - 1)

    def find_mems_contigs(self, contigs, bases, read_offsets, min_len, both_strands=False, split_breaks=False, max_occ=0,
                          rows_hint=None):
        """find_mems on a reference of several sequences (genie_find_mems_contigs; contigs: the ReferenceSet this index was
        built from).  The same four results; a row lies inside one contig: matches are cut at the contig boundaries, a
        contig start is a left end, and what is left of an occurrence with fewer than min_len bases to its contig's end is
        no row.  pos stays 1-based in the concatenation (contig_coords names it); max_occ counts occurrences in the
        concatenation.  If the rows outnumber rows_hint the call is made again with room for all."""
        off, table = self._contig_table(contigs)
        return self._find_mems("genie_find_mems_contigs", table, (table[1],), bases, read_offsets, min_len, both_strands,
                               split_breaks, max_occ, rows_hint)

    def _csr_call(self, bases, read_offsets, both_strands=False, split_breaks=False, name="read_offsets"):
        """The CSR batch of a call on the device -> (bases, read_offsets, N, total, max_len, flags, S).  `name`: what the
        offsets argument is called where it is too short."""
        self._need_device()
        bases = self._as_dev(bases, torch.uint8).reshape(-1)
        read_offsets = self._as_dev(read_offsets, torch.int64).reshape(-1)
        if read_offsets.numel() < 1:
            raise ValueError(f"{name} needs N + 1 entries")
        n_reads = read_offsets.numel() - 1
        total = bases.numel()
        max_len = int((read_offsets[1:] - read_offsets[:-1]).max().item()) if n_reads else 0
        max_len = min(max(max_len, 0), 2**31 - 1)
        if total == 0:
            bases = torch.zeros(1, dtype=torch.uint8, device=self.device)
        flags = (N.READS_BOTH_STRANDS if both_strands else 0) | (N.READS_SPLIT_BREAKS if split_breaks else 0)
        return bases, read_offsets, n_reads, total, max_len, flags, 2 if both_strands else 1

    def _step_stats(self, name, head, extra, size_tail, bases, read_offsets, intervals, both_strands, split_breaks):
        """A match-statistics call with a step, name(handle, *head, flags, *extra, batch, ms, lohi, status, totals, workspace)
        -> (ms, lohi, status, total); `size_tail`: what the workspace function takes behind the flags."""
        bases, read_offsets, n_reads, total, max_len, flags, strands = self._csr_call(bases, read_offsets, both_strands, split_breaks)
        ms = torch.empty(strands * total, dtype=torch.int32, device=self.device)
        lohi = torch.empty((strands * total, 2), dtype=torch.int32, device=self.device) if intervals else None
        status = torch.empty(strands * n_reads, dtype=torch.int32, device=self.device)
        totals = torch.zeros(1, dtype=torch.int64, device=self.device)
        ws, ws_bytes = self._workspace(name + "_workspace_bytes", n_reads, total, max_len, flags, *size_tail)
        self._run(name, *head, flags, *extra, _ptr(bases), _ptr(read_offsets), n_reads, total, max_len, _ptr(ms), _ptr(lohi),
                  _ptr(status), _ptr(totals), _ptr(ws), ws_bytes)
        return ms, lohi, status, int(totals.item())

    def _step_smems(self, name, head, extra, size_tail, mode, bases, read_offsets, min_len, rows_hint, both_strands, split_breaks):
        """An SMEM call with a step, name(handle, *head, mode, flags, batch, min_len, *extra, rows, status, totals, workspace)
        -> (offsets, smems, status, total); `size_tail` as in _step_stats."""
        self._bwa_if_split(mode, split_breaks)
        bases, read_offsets, n_reads, total, max_len, flags, strands = self._csr_call(bases, read_offsets, both_strands, split_breaks)
        totals = torch.zeros(1, dtype=torch.int64, device=self.device)
        ws, ws_bytes = self._workspace(name + "_workspace_bytes", n_reads, total, max_len, flags, *size_tail)
        offsets, rows, status = self._run_csr(name, (*head, N.MODES[mode], flags, _ptr(bases), _ptr(read_offsets), n_reads, total,
                                                     max_len, int(min_len), *extra),
                                              strands * n_reads, int(rows_hint) if rows_hint else strands * max(8 * n_reads, total // 6),
                                              (_ptr(totals), _ptr(ws), ws_bytes))
        return offsets, rows, status, int(totals.item())

    def match_stats_contigs(self, contigs, bases, read_offsets, intervals=True, both_strands=False, split_breaks=False):
        """match_stats that is exact with respect to a reference of several sequences (genie_match_stats_contigs; contigs:
        the ReferenceSet this index was built from) -> (ms, lohi, status, clipped).  ms[v] is the longest match from that
        position that lies inside ONE contig (the maximum over the contigs of the matching statistic against each alone),
        lohi its inclusive interval in the concatenation -- it may hold bridging rows, which locate_contigs drops, and holds
        at least one that does not --, status as match_stats, clipped the number of positions where ms is shorter than
        match_stats's."""
        off, table = self._contig_table(contigs)
        return self._step_stats("genie_match_stats_contigs", table, (), (table[1],), bases, read_offsets, intervals, both_strands,
                                split_breaks)

    def find_smems_contigs(self, contigs, mode, bases, read_offsets, min_len=1, rows_hint=None, both_strands=False,
                           split_breaks=False):
        """find_smems_long whose rows are the SMEMs with respect to the SET of sequences (genie_find_smems_contigs; contigs:
        the ReferenceSet this index was built from) -> (offsets, smems int32[S, 4], status, clipped).  The rows are what the
        traversal gives on the contig-exact matching statistics: (lo, hi) is the interval of the row's bases in the
        concatenation and at least one of its occurrences lies inside one contig, so every row has a hit in locate_contigs.
        Options, row order and status as find_smems_long; clipped as match_stats_contigs.  If the rows outnumber rows_hint
        the call is made again with room for all."""
        self._bwa_if_split(mode, split_breaks)      # before the table's own checks
        off, table = self._contig_table(contigs)
        return self._step_smems("genie_find_smems_contigs", table, (), (table[1],), mode, bases, read_offsets, min_len, rows_hint,
                                both_strands, split_breaks)

    def match_stats_min_occ(self, bases, read_offsets, min_occ, intervals=True, both_strands=False, split_breaks=False):
        """match_stats of what occurs at least min_occ times in the reference (genie_match_stats_min_occ) -> (ms, lohi,
        status, shortened).  ms[v] is the length of the longest match from that position whose suffix-array interval has
        at least min_occ rows, lohi that interval ((-1, -1) where ms is 0), shortened the number of positions where ms is
        shorter than match_stats's.  A base that occurs fewer than min_occ times is "rare": it flags its strand-read
        READ_ABSENT_BASE, or is a break with split_breaks.  min_occ = 1 is match_stats."""
        return self._step_stats("genie_match_stats_min_occ", (), (int(min_occ),), (), bases, read_offsets, intervals, both_strands,
                                split_breaks)

    def find_smems_min_occ(self, mode, bases, read_offsets, min_occ, min_len=1, rows_hint=None, both_strands=False,
                           split_breaks=False):
        """find_smems_long under a minimum occurrence count, BWA-MEM's min_intv (genie_find_smems_min_occ) -> (offsets,
        smems int32[S, 4], status, shortened).  The rows are the matches of at least min_occ occurrences that no other such
        match contains: hi - lo + 1 >= min_occ on every row.  Options, row order and status as find_smems_long, rare bases
        and shortened as match_stats_min_occ.  Re-seeding is a loop over min_occ = occ + 1 of this call that keeps the rows
        covering the long SMEM's midpoint.  If the rows outnumber rows_hint the call is made again with room for all."""
        return self._step_smems("genie_find_smems_min_occ", (), (int(min_occ),), (), mode, bases, read_offsets, min_len, rows_hint,
                                both_strands, split_breaks)

    def locate_contigs(self, contigs, rows):
        """SMEM rows int32 [S, 4] (start, end, lo, hi) of any find_smems* call -> (hit_offsets int64[S+1], hits int32[T, 2]
        = (contig, 1-based offset inside it), dropped) (genie_locate_contigs).  The rows stay SMEMs of the concatenation;
        this drops the occurrences that bridge two sequences (`dropped` counts them), BWA's rule.  Hits of a row are in
        suffix-array row order."""
        off, table = self._contig_table(contigs)
        rows = self._as_dev(rows, torch.int32)
        if rows.dim() != 2 or rows.shape[1] != 4:
            raise ValueError("rows must be [S, 4] (start, end, lo, hi)")
        S = rows.shape[0]
        offsets = torch.empty(S + 1, dtype=torch.int64, device=self.device)
        totals = torch.empty(2, dtype=torch.int64, device=self.device)
        tmp, tmp_bytes = self._workspace("genie_locate_contigs_tmp_bytes", S)
        self._run("genie_locate_contigs", *table, _ptr(rows), S, _ptr(offsets), C.c_void_p(0), 0, _ptr(totals), _ptr(tmp), tmp_bytes)
        kept, dropped = (int(x) for x in totals.tolist())
        hits = torch.empty((max(kept, 1), 2), dtype=torch.int32, device=self.device)
        self._run("genie_locate_contigs", *table, _ptr(rows), S, _ptr(offsets), _ptr(hits), kept, _ptr(totals), _ptr(tmp), tmp_bytes)
        return offsets, hits[:kept], dropped

    def chain_mems(self, offsets, rows, contigs=None, max_dist=5000, bandwidth=500, gap_cost=2, max_pred=5000, min_score=40,
                   by_score=False):
        """The MEM rows of find_mems / find_mems_contigs chained per strand-read (genie_chain_mems) -> (chain_offsets
        int64[U+1], chains int32[C, 8] = (q_begin, q_end, r_begin, r_end, score, n_anchors, contig, last), anchor_chain,
        anchor_pred, anchor_score int32[R], dropped) on the device.  offsets / rows: the first two results of find_mems*,
        unchanged; contigs: the ReferenceSet of find_mems_contigs, or None (every anchor in contig 0).  An anchor j may
        precede i when both lie on one contig, i starts 1 .. max_dist bases later in the read and in the reference, and
        the two distances differ by at most bandwidth; the link adds min(length of i, the distances) - gap_cost / 16 per
        base of that difference; max_pred > 0 looks at that many rows back at most.  A chain is kept when it scores at
        least min_score; `dropped` counts the others.  The chains of a unit come ordered by `last` (the row of the
        chain's top inside its unit); by_score=True reorders them by (score descending, last ascending) and renumbers
        anchor_chain.  Anchors behind offsets[U] belong to no unit: -1.  The defaults are this wrapper's; the C call has
        none."""
        self._need_device()
        offsets = self._as_dev(offsets, torch.int64).reshape(-1)
        rows = self._as_dev(rows, torch.int32)
        if offsets.numel() < 1:
            raise ValueError("offsets needs U + 1 entries")
        if rows.dim() != 2 or rows.shape[1] != 4:
            raise ValueError("rows must be [R, 4] (start, end, pos, row)")
        table = (C.c_void_p(0), 0)
        if contigs is not None:
            off, table = self._contig_table(contigs)
        U, R = offsets.numel() - 1, rows.shape[0]
        prm = (int(max_dist), int(bandwidth), int(gap_cost), int(max_pred), int(min_score))
        chain_offsets = torch.empty(U + 1, dtype=torch.int64, device=self.device)
        anchors = [torch.full((R,), -1, dtype=torch.int32, device=self.device) for _ in range(3)]
        totals = torch.empty(2, dtype=torch.int64, device=self.device)
        ws, ws_bytes = self._workspace("genie_chain_mems_workspace_bytes", U, R, table[1])
        none = C.c_void_p(0)
        head = (*table, _ptr(offsets), _ptr(rows) if R else none, U, R, *prm, _ptr(chain_offsets))
        tail = (*[_ptr(t) if R else none for t in anchors], _ptr(totals), _ptr(ws), ws_bytes)
        self._run("genie_chain_mems", *head, none, 0, none, none, none, *tail[3:])      # the sizing call
        kept, dropped = (int(x) for x in totals.tolist())
        chains = torch.empty((max(kept, 1), 8), dtype=torch.int32, device=self.device)
        self._run("genie_chain_mems", *head, _ptr(chains), kept, *tail)
        chains = chains[:kept]
        if by_score and kept:
            chains = chains[self._chains_by_score(offsets, chain_offsets, chains, anchors[0])]
        return chain_offsets, chains, anchors[0], anchors[1], anchors[2], dropped

    def _chains_by_score(self, offsets, chain_offsets, chains, anchor_chain):
        """The order of chain_mems' by_score: each unit's chains by (score descending, last ascending); anchor_chain is
        renumbered in place -> the permutation, which the caller applies to the chain rows (and to what is parallel to them)."""
        U, kept = offsets.numel() - 1, chains.shape[0]
        units = torch.arange(U, device=self.device)
        unit = torch.repeat_interleave(units, chain_offsets[1:] - chain_offsets[:-1])
        # stable sorts, least significant key first: last ascending, score descending, unit ascending
        order = torch.argsort(chains[:, 7], stable=True)
        order = order[torch.argsort(-chains[order, 4].long(), stable=True)]
        order = order[torch.argsort(unit[order], stable=True)]
        rank = torch.empty(kept, dtype=torch.int64, device=self.device)
        rank[order] = torch.arange(kept, device=self.device) - chain_offsets[unit[order]]
        a_unit = torch.repeat_interleave(units, offsets[1:] - offsets[:-1])
        ac = anchor_chain[:a_unit.numel()]
        has = ac >= 0
        ac[has] = rank[chain_offsets[a_unit[has]] + ac[has].long()].to(torch.int32)
        return order

    def align_chains(self, reads, offsets, rows, chains_result, contigs=None, both_strands=False, match=1, mismatch=4, gap_open=6,
                     gap_extend=1, band=32, max_indel=64, end_bonus=5):
        """Every chain of chain_mems aligned (genie_align_chains): a banded affine gap fill between the chain's members and
        a banded extension at both ends -> (aln int32[C, 8] = (score, q_begin, q_end, r_begin, r_end, flags, n_used,
        matched), (aligned, skipped)) on the device, one row per chain row.  reads: (bases, read_offsets) as find_mems took
        them; offsets / rows: its first two results; chains_result: what chain_mems returned for them with by_score=False
        (the call walks anchor_chain and anchor_pred as the C call wrote them); contigs and both_strands as in those calls.
        A match scores `match`, a mismatch -mismatch, a gap of g bases -(gap_open + g gap_extend); gaps are filled inside a
        band of `band` diagonals around the straight line, a chain with a gap whose sides differ by more than max_indel is
        skipped (flags 4, the rest 0); an extension that reaches its end of the read within end_bonus of its best local
        score goes to the end (flags 1: left, 2: right).  r_begin / r_end are 1-based in the concatenation.  Score and end
        points only: no traceback.  The defaults are this wrapper's; the C call has none."""
        bases, read_offsets = reads
        bases, read_offsets, n_reads, total, max_len, flags, strands = self._csr_call(bases, read_offsets, both_strands)
        offsets = self._as_dev(offsets, torch.int64).reshape(-1)
        rows = self._as_dev(rows, torch.int32)
        chain_offsets, chains, anchor_chain, anchor_pred = (self._as_dev(t, d) for t, d in zip(
            chains_result[:4], (torch.int64, torch.int32, torch.int32, torch.int32)))
        if rows.dim() != 2 or rows.shape[1] != 4 or chains.dim() != 2 or chains.shape[1] != 8:
            raise ValueError("rows must be [R, 4] and the chain rows [C, 8]")
        U, R, kept = offsets.numel() - 1, rows.shape[0], chains.shape[0]
        if U != strands * n_reads or chain_offsets.numel() != U + 1 or min(anchor_chain.numel(), anchor_pred.numel()) < R:
            raise ValueError("offsets, chain offsets and anchor arrays must be those of these reads' find_mems and chain_mems")
        table = (C.c_void_p(0), 0)
        if contigs is not None:
            off, table = self._contig_table(contigs)
        prm = (int(match), int(mismatch), int(gap_open), int(gap_extend), int(band), int(max_indel), int(end_bonus))
        aln = torch.empty((max(kept, 1), 8), dtype=torch.int32, device=self.device)
        totals = torch.empty(2, dtype=torch.int64, device=self.device)
        ws, ws_bytes = self._workspace("genie_align_chains_workspace_bytes", U, kept)
        none = C.c_void_p(0)
        self._run("genie_align_chains", *table, flags, _ptr(bases), _ptr(read_offsets), n_reads, total, max_len, _ptr(offsets),
                  _ptr(rows) if R else none, U, R, _ptr(anchor_chain) if R else none, _ptr(anchor_pred) if R else none,
                  _ptr(chain_offsets), _ptr(chains) if kept else none, kept, *prm, _ptr(aln) if kept else none, _ptr(totals),
                  _ptr(ws), ws_bytes)
        return aln[:kept], tuple(int(x) for x in totals.tolist())

    def chain_cigars(self, reads, offsets, rows, chains_result, aln, select=None, contigs=None, both_strands=False, match=1, mismatch=4,
                     gap_open=6, gap_extend=1, band=32, max_indel=64, end_bonus=5, ops_hint=None, dir_bytes_hint=None):
        """The CIGAR of selected chains (genie_chain_cigars): the traceback of align_chains -> (cigar_offsets int64[n_sel+1],
        cigar uint32[ops], info int32[n_sel, 8] = (chain, flags, n_ops, nm, n_eq, n_x, ins_bases, del_bases)) on the device;
        cigar_strings turns the first two into text.  reads, offsets, rows, chains_result, contigs, both_strands and the
        scoring options exactly as align_chains took them; aln: its first result.  select: global chain indices (rows of
        chains / aln), any order, repeats allowed, None: every chain.  An op is SAM's len << 4 | op with I = 1, D = 2, S = 4,
        '=' = 7, X = 8, in strand-read order, the clipped ends as S.  flags 4: the chain was skipped by align_chains, 16: an
        index outside the chains (or an aln row that is not this chain's); such a chain has no ops.  ops_hint and
        dir_bytes_hint size the first call (ops in all; bytes for the directions of the dynamic programs, four bits per
        cell); when either is too small the call is made again with room for all."""
        bases, read_offsets = reads
        bases, read_offsets, n_reads, total, max_len, flags, strands = self._csr_call(bases, read_offsets, both_strands)
        offsets = self._as_dev(offsets, torch.int64).reshape(-1)
        rows = self._as_dev(rows, torch.int32)
        chain_offsets, chains, anchor_chain, anchor_pred = (self._as_dev(t, d) for t, d in zip(
            chains_result[:4], (torch.int64, torch.int32, torch.int32, torch.int32)))
        aln = self._as_dev(aln, torch.int32)
        if rows.dim() != 2 or rows.shape[1] != 4 or chains.dim() != 2 or chains.shape[1] != 8 or aln.shape != chains.shape:
            raise ValueError("rows must be [R, 4], the chain rows [C, 8] and aln parallel to them")
        U, R, kept = offsets.numel() - 1, rows.shape[0], chains.shape[0]
        if U != strands * n_reads or chain_offsets.numel() != U + 1 or min(anchor_chain.numel(), anchor_pred.numel()) < R:
            raise ValueError("offsets, chain offsets and anchor arrays must be those of these reads' find_mems and chain_mems")
        none = C.c_void_p(0)
        sel = None
        if select is not None:
            sel = self._as_dev(select, torch.int64).reshape(-1)
            if sel.numel() == 0:
                sel = torch.zeros(1, dtype=torch.int64, device=self.device)[:0]
        n_sel = kept if sel is None else sel.numel()
        # an empty selection still has to be told from `every chain`: any aligned non-null address, it is never read
        sel_ptr = none if sel is None else C.c_void_p(sel.data_ptr() if n_sel else 8)
        table = (C.c_void_p(0), 0)
        if contigs is not None:
            off, table = self._contig_table(contigs)
        prm = (int(match), int(mismatch), int(gap_open), int(gap_extend), int(band), int(max_indel), int(end_bonus))
        # aln and chains may be empty tensors: the call wants an address for d_aln whatever cap_chains is
        aln_buf = aln if kept else torch.zeros((1, 8), dtype=torch.int32, device=self.device)
        cigar_offsets = torch.empty(n_sel + 1, dtype=torch.int64, device=self.device)
        info = torch.empty((max(n_sel, 1), 8), dtype=torch.int32, device=self.device)
        totals = torch.empty(3, dtype=torch.int64, device=self.device)
        cap_ops = int(ops_hint) if ops_hint else 8 * n_sel
        dir_bytes = int(dir_bytes_hint) if dir_bytes_hint is not None else min(n_sel << 14, 1 << 28)
        while True:
            cigar = torch.empty(max(cap_ops, 1), dtype=torch.int32, device=self.device)
            ws, ws_bytes = self._workspace("genie_chain_cigars_workspace_bytes", U, kept, n_sel if sel is not None else kept, dir_bytes)
            self._run("genie_chain_cigars", *table, flags, _ptr(bases), _ptr(read_offsets), n_reads, total, max_len, _ptr(offsets),
                      _ptr(rows) if R else none, U, R, _ptr(anchor_chain) if R else none, _ptr(anchor_pred) if R else none,
                      _ptr(chain_offsets), _ptr(chains) if kept else none, kept, *prm, _ptr(aln_buf), sel_ptr, n_sel,
                      _ptr(cigar_offsets), _ptr(cigar) if cap_ops else none, cap_ops, _ptr(info), none, _ptr(totals), dir_bytes,
                      _ptr(ws), ws_bytes)
            need = int(totals[2].item())
            if need > dir_bytes:                                     # some chain found no room for its directions
                dir_bytes = need
                continue
            ops = int(cigar_offsets[n_sel].item())
            if ops <= cap_ops:
                return cigar_offsets, cigar[:ops].view(torch.uint32), info[:n_sel]
            cap_ops = ops

    def select_alignments(self, read_offsets, chain_offsets, chains, aln, contigs=None, both_strands=False, mask_level=50, pri_ratio=80,
                          max_secondary=5, min_score=1, mapq_full=40):
        """The alignments of every read (genie_select_alignments): its chains, as align_chains scored them, classified as
        primary (kind 0), supplementary (1), secondary (2) or none (3) by minimap2's parent rule, with a mapping quality ->
        (sel_offsets int64[N+1], sel int64[n], records int32[n, 12] = (read, chain, kind, strand, contig, offset, r_span,
        q_begin, q_end, score, sub, mapq), klass int32[C, 4] = (kind, parent, order, mapq), read_counts int32[N, 4] =
        (candidates, primaries, secondaries, best chain or -1), totals int64[4] = (candidates, primaries, secondaries,
        selected)) on the device.  sel lists, read by read, the primaries by (score descending, chain ascending) and then at
        most max_secondary secondaries that score at least pri_ratio percent of their primary; it is chain_cigars' `select`.
        read_offsets as find_mems took them; chain_offsets and chains: chain_mems' first two results; aln: align_chains'
        first.  Two candidates overlap when their forward read intervals share more than mask_level percent of the shorter;
        chains below min_score are no candidates; mapq = 60 (1 - sub / score) min(1, matched / mapq_full), rounded down.  q_begin
        and q_end are in forward read coordinates, offset is 1-based inside the contig.  The defaults are this wrapper's; the
        C call has none."""
        self._need_device()
        read_offsets = self._as_dev(read_offsets, torch.int64).reshape(-1)
        chain_offsets = self._as_dev(chain_offsets, torch.int64).reshape(-1)
        chains, aln = self._as_dev(chains, torch.int32), self._as_dev(aln, torch.int32)
        if read_offsets.numel() < 1:
            raise ValueError("read_offsets needs N + 1 entries")
        if chains.dim() != 2 or chains.shape[1] != 8 or aln.shape != chains.shape:
            raise ValueError("the chain rows must be [C, 8] and aln parallel to them")
        strands = 2 if both_strands else 1
        n_reads, U, kept = read_offsets.numel() - 1, chain_offsets.numel() - 1, chains.shape[0]
        if U != strands * n_reads:
            raise ValueError("chain_offsets must be those of these reads' chain_mems")
        table = (C.c_void_p(0), 0)
        if contigs is not None:
            off, table = self._contig_table(contigs)
        prm = (int(mask_level), int(pri_ratio), int(max_secondary), int(min_score), int(mapq_full))
        none = C.c_void_p(0)
        klass = torch.empty((max(kept, 1), 4), dtype=torch.int32, device=self.device)
        sel_offsets = torch.empty(n_reads + 1, dtype=torch.int64, device=self.device)
        read_counts = torch.empty((max(n_reads, 1), 4), dtype=torch.int32, device=self.device)
        totals = torch.empty(4, dtype=torch.int64, device=self.device)
        ws, ws_bytes = self._workspace("genie_select_alignments_workspace_bytes", n_reads, kept)
        head = (*table, N.READS_BOTH_STRANDS if both_strands else 0, _ptr(read_offsets), n_reads, _ptr(chain_offsets), U,
                _ptr(chains) if kept else none, _ptr(aln) if kept else none, kept, *prm, _ptr(klass) if kept else none, _ptr(sel_offsets))
        tail = (_ptr(read_counts), _ptr(totals), _ptr(ws), ws_bytes)
        cap_sel = n_reads                                            # most reads have one alignment; more: a second call
        while True:
            sel = torch.empty(max(cap_sel, 1), dtype=torch.int64, device=self.device)
            records = torch.empty((max(cap_sel, 1), 12), dtype=torch.int32, device=self.device)
            self._run("genie_select_alignments", *head, _ptr(sel), _ptr(records), cap_sel, *tail)
            n_sel = int(sel_offsets[n_reads].item())
            if n_sel <= cap_sel:
                return sel_offsets, sel[:n_sel], records[:n_sel], klass[:kept], read_counts[:n_reads], totals
            cap_sel = n_sel

    def pair_alignments(self, sel_offsets, records, klass, orient="fr", isize_min=0, isize_max=1000, isize_mean=300, pen_slope=8,
                        pen_max=16, pen_unpaired=17, mapq_boost=40):
        """The alignments of paired-end reads (genie_pair_alignments): reads 2k and 2k + 1 are the mates of pair k; for every
        pair the best concordant combination of the mates' candidate records (the head of a read and the secondaries of that
        head) against the two heads taken alone -> (pairs int32[P, 8] = (rec0, rec1, flags, pair_score, sub_score, isize,
        n_concordant, type), sam int32[R, 4] = (flag, mapq, mate_record, tlen), totals int64[4] = (pairs with both mates
        mapped, proper pairs, mates whose chosen record is not their head, pairs with exactly one mate mapped)) on the device.
        sel_offsets, records, klass: select_alignments' first, third and fourth results.  orient: "fr", "rf", "same", "any" or
        the mask itself (bit 0 FR, bit 1 RF, bit 2 same strand).  A combination is concordant when its orientation is allowed
        and isize_min <= span <= isize_max; it is worth the two scores less min(pen_max, |span - isize_mean| pen_slope / 256),
        and the pair is proper when the best one is worth at least the two heads less pen_unpaired.  sam holds SAM's flag bits
        and, for the chosen record of a proper pair, a mapq raised to the pair's by at most mapq_boost.  The defaults are this
        wrapper's -- a concordant pair of heads always beats the unpaired alternative: pen_max < pen_unpaired --; the C call
        has none."""
        self._need_device()
        sel_offsets = self._as_dev(sel_offsets, torch.int64).reshape(-1)
        records, klass = self._as_dev(records, torch.int32), self._as_dev(klass, torch.int32)
        if sel_offsets.numel() < 1 or (sel_offsets.numel() - 1) % 2:
            raise ValueError("sel_offsets needs N + 1 entries for an even number of reads: mates are interleaved")
        if records.dim() != 2 or records.shape[1] != 12 or klass.dim() != 2 or klass.shape[1] != 4:
            raise ValueError("records must be [R, 12] and klass [C, 4], as select_alignments returns them")
        n_reads, n_rec, kept = sel_offsets.numel() - 1, records.shape[0], klass.shape[0]
        mask = N.PAIR_ORIENT[orient] if isinstance(orient, str) else int(orient)
        prm = (mask, int(isize_min), int(isize_max), int(isize_mean), int(pen_slope), int(pen_max), int(pen_unpaired), int(mapq_boost))
        none = C.c_void_p(0)
        pairs = torch.empty((max(n_reads // 2, 1), 8), dtype=torch.int32, device=self.device)
        sam = torch.empty((max(n_rec, 1), 4), dtype=torch.int32, device=self.device)
        totals = torch.empty(4, dtype=torch.int64, device=self.device)
        ws, ws_bytes = self._workspace("genie_pair_alignments_workspace_bytes", n_reads, n_rec)
        self._run("genie_pair_alignments", n_reads, _ptr(sel_offsets), _ptr(records) if n_rec else none, n_rec,
                  _ptr(klass) if kept else none, kept, *prm, _ptr(pairs), _ptr(sam) if n_rec else none, _ptr(totals), _ptr(ws), ws_bytes)
        return pairs[:n_reads // 2], sam[:n_rec], totals

    def insert_size_stats(self, sel_offsets, records, min_mapq=20, max_span=10000, min_samples=25, samples=False):
        """The insert-size distribution of a paired batch, estimated from the batch (genie_insert_size_stats) -> (stats
        int64[3, 12], one row per combination type FR, RF, same = (n, ok, q25, q50, q75, lo_b, hi_b, n_in, mean, std,
        isize_min, isize_max); samples int32[P, 2] = (type, span) per pair, (-1, 0) for a pair that gives none, or None; totals
        int64[4] = (pairs with both mates mapped, pairs sampled, refused for mapq alone, refused for contig, type or span)) on
        the device.  sel_offsets, records: select_alignments' first and third results.  A pair is a sample when both heads
        have a mapq of at least min_mapq, share a contig and span 1 to max_span bases; a type with at least min_samples
        samples and a twentieth of the largest type's is ok.  insert_size_options turns stats into pair_alignments' options.
        The defaults are this wrapper's; the C call has none."""
        self._need_device()
        sel_offsets = self._as_dev(sel_offsets, torch.int64).reshape(-1)
        records = self._as_dev(records, torch.int32)
        if sel_offsets.numel() < 1 or (sel_offsets.numel() - 1) % 2:
            raise ValueError("sel_offsets needs N + 1 entries for an even number of reads: mates are interleaved")
        if records.dim() != 2 or records.shape[1] != 12:
            raise ValueError("records must be [R, 12], as select_alignments returns them")
        n_reads, n_rec = sel_offsets.numel() - 1, records.shape[0]
        none = C.c_void_p(0)
        stats = torch.empty((3, 12), dtype=torch.int64, device=self.device)
        per_pair = torch.empty((max(n_reads // 2, 1), 2), dtype=torch.int32, device=self.device) if samples else None
        totals = torch.empty(4, dtype=torch.int64, device=self.device)
        ws, ws_bytes = self._workspace("genie_insert_size_stats_workspace_bytes", n_reads, int(max_span))
        self._run("genie_insert_size_stats", n_reads, _ptr(sel_offsets), _ptr(records) if n_rec else none, n_rec, int(min_mapq),
                  int(max_span), int(min_samples), _ptr(stats), _ptr(per_pair) if samples else none, _ptr(totals), _ptr(ws), ws_bytes)
        return stats, per_pair[:n_reads // 2] if samples else None, totals

    def rescue_windows(self, read_offsets, sel_offsets, records, pairs, contigs=None, orient="fr", isize_max=1000, min_anchor_score=40):
        """Where to seed a mate again next to its partner (genie_rescue_windows) -> (windows int32[2N, 2] = (wb, we), 0-based
        and half-open in the concatenation, (0, 0) for none; totals int64[3] = (units with a window, pairs with at least one,
        reads that are targets)) on the device.  Unit 2r + s is strand s of read r.  read_offsets as find_mems took them;
        sel_offsets, records: select_alignments' first and third results; pairs: pair_alignments' first.  A mate of a pair that
        is not proper is a target when the other mate's chosen record scores at least min_anchor_score; its windows are where
        a record would have to lie to be concordant with that record under orient and isize_max (pair_alignments' options).
        The defaults are this wrapper's; the C call has none."""
        self._need_device()
        read_offsets = self._as_dev(read_offsets, torch.int64).reshape(-1)
        sel_offsets = self._as_dev(sel_offsets, torch.int64).reshape(-1)
        records, pairs = self._as_dev(records, torch.int32), self._as_dev(pairs, torch.int32)
        n_reads = sel_offsets.numel() - 1
        if n_reads < 0 or n_reads % 2 or read_offsets.numel() != n_reads + 1:
            raise ValueError("read_offsets and sel_offsets need N + 1 entries for an even number of reads: mates are interleaved")
        if records.dim() != 2 or records.shape[1] != 12 or pairs.dim() != 2 or pairs.shape[1] != 8 or pairs.shape[0] != n_reads // 2:
            raise ValueError("records must be [R, 12] and pairs [N / 2, 8], as select_alignments and pair_alignments return them")
        table = (C.c_void_p(0), 0)
        if contigs is not None:
            off, table = self._contig_table(contigs)
        mask = N.PAIR_ORIENT[orient] if isinstance(orient, str) else int(orient)
        n_rec = records.shape[0]
        none = C.c_void_p(0)
        windows = torch.zeros((max(2 * n_reads, 1), 2), dtype=torch.int32, device=self.device)
        totals = torch.empty(3, dtype=torch.int64, device=self.device)
        ws, ws_bytes = self._workspace("genie_rescue_windows_workspace_bytes", n_reads)
        self._run("genie_rescue_windows", *table, _ptr(read_offsets), n_reads, _ptr(sel_offsets), _ptr(records) if n_rec else none, n_rec,
                  _ptr(pairs) if n_reads else none, mask, int(isize_max), int(min_anchor_score), _ptr(windows), _ptr(totals), _ptr(ws),
                  ws_bytes)
        return windows[:2 * n_reads], totals

    def window_mems(self, bases, read_offsets, windows, min_len, offsets=None, rows=None, both_strands=False, split_breaks=False,
                    rows_hint=None):
        """The MEMs of every strand-read against its own window of the reference, merged into the MEM rows of the batch
        (genie_window_mems) -> (offsets int64[U+1], mems int32[R, 4] = (start, end, pos, row), status int32[U], totals
        int64[3] = (rows in all, window rows added, units over a cap)) on the device.  bases / read_offsets and the units as
        find_mems; windows int32[U, 2] = (wb, we), 0-based and half-open, wb == we for none (rescue_windows' first result, or
        any other); offsets / rows: the first two results of find_mems* for the same batch, or None.  A unit without a window
        keeps its rows; one with a window gets the union of its rows and the MEMs of at least min_len bases against the window
        alone, ordered by (start, pos, end), the new rows with row -1.  status 1: searched, 2: more than WINDOW_MAX_ROWS rows,
        4: a read above MAX_READ_LEN (both keep their rows).  If the rows outnumber rows_hint the call is made again with room
        for all."""
        bases, read_offsets, n_reads, total, max_len, flags, strands = self._csr_call(bases, read_offsets, both_strands, split_breaks)
        U = strands * n_reads
        windows = self._as_dev(windows, torch.int32)
        if windows.numel() != 2 * U:
            raise ValueError("windows must be [U, 2], one row per strand-read")
        if windows.numel() == 0:
            windows = torch.zeros((1, 2), dtype=torch.int32, device=self.device)
        none = C.c_void_p(0)
        tail_in = (none, none, 0)
        if offsets is not None:
            in_offsets = self._as_dev(offsets, torch.int64).reshape(-1)
            in_rows = self._as_dev(rows, torch.int32)
            if in_offsets.numel() != U + 1 or in_rows.dim() != 2 or in_rows.shape[1] != 4:
                raise ValueError("offsets must have U + 1 entries and rows be [R, 4], as find_mems returns them")
            tail_in = (_ptr(in_offsets), _ptr(in_rows) if in_rows.shape[0] else none, in_rows.shape[0])
        out_offsets = torch.empty(U + 1, dtype=torch.int64, device=self.device)
        status = torch.empty(max(U, 1), dtype=torch.int32, device=self.device)
        totals = torch.empty(3, dtype=torch.int64, device=self.device)
        ws, ws_bytes = self._workspace("genie_window_mems_workspace_bytes", U)
        cap_rows = int(rows_hint) if rows_hint else tail_in[2] + 8 * U
        while True:
            out = torch.empty((max(cap_rows, 1), 4), dtype=torch.int32, device=self.device)
            self._run("genie_window_mems", flags, _ptr(bases), _ptr(read_offsets), n_reads, total, max_len, U, _ptr(windows), int(min_len),
                      *tail_in, _ptr(out_offsets), _ptr(out), out.shape[0], _ptr(status), _ptr(totals), _ptr(ws), ws_bytes)
            found = int(totals[0].item())
            if found <= out.shape[0]:
                return out_offsets, out[:found], status[:U], totals
            cap_rows = found                      # capacity guess too small: rerun with the exact size

    def sam_text(self, bases, read_offsets, sel_offsets, records, sam, info, cigar_offsets, cigar, names, name_offsets, contig_names,
                 contig_name_offsets, quals=None, contigs=None, tags=N.SAM_NM | N.SAM_AS, seq=True):
        """The SAM records of a mapped batch as text on the device (genie_sam_text) -> (text uint8[bytes], line_offsets
        int64[n_lines + 1], totals int64[3] = (lines, bytes, unmapped lines)): line l is text[line_offsets[l] :
        line_offsets[l + 1]], read by read and record by record as sam_lines orders them, a read without records one unmapped
        line, every line ended by "\\n"; the header is sam_header's.  bases / read_offsets: the batch in read orientation;
        sel_offsets, records, sam, info, cigar_offsets, cigar: map_pairs' results, or with sam=None map_records' (single-end
        mode); names / name_offsets and contig_names / contig_name_offsets: names as CSR bytes (names_csr,
        text_reads.fastq_fields); quals: uint8 parallel to bases, or None (`*`); contigs: the ReferenceSet of the records, or
        None for one contig; tags: a mask of SAM_NM, SAM_AS, SAM_MD, SAM_MC, SAM_MQ; seq=False writes `*` for SEQ and QUAL.
        Two native calls: one sizes the text, one fills it."""
        return self._sam_bytes("genie_sam_text", bases, read_offsets, sel_offsets, records, sam, info, cigar_offsets, cigar, names,
                               name_offsets, contig_names, contig_name_offsets, quals, contigs, tags, seq)

    def bam_records(self, bases, read_offsets, sel_offsets, records, sam, info, cigar_offsets, cigar, names, name_offsets, contig_names,
                    contig_name_offsets, quals=None, contigs=None, tags=N.SAM_NM | N.SAM_AS, seq=True):
        """The same batch as uncompressed BAM alignment records on the device (genie_bam_records) -> (data uint8[bytes],
        record_offsets int64[n + 1], totals int64[3] = (records, bytes, unmapped records)): record l is data[record_offsets[l] :
        record_offsets[l + 1]], one per line of sam_text and in its order, block_size first.  The arguments and their forms are
        sam_text's; of contig_names only the count matters (BAM names a contig by its index).  bam_header(...) + data, through
        bgzf_compress, is a BAM file.  Two native calls: one sizes the data, one fills it."""
        return self._sam_bytes("genie_bam_records", bases, read_offsets, sel_offsets, records, sam, info, cigar_offsets, cigar, names,
                               name_offsets, contig_names, contig_name_offsets, quals, contigs, tags, seq)

    def _sam_bytes(self, entry, bases, read_offsets, sel_offsets, records, sam, info, cigar_offsets, cigar, names, name_offsets,
                   contig_names, contig_name_offsets, quals, contigs, tags, seq):
        """sam_text and bam_records: two calls with the same arguments, and bytes, offsets and totals of one shape."""
        bases, read_offsets, n_reads, total, _, _, _ = self._csr_call(bases, read_offsets)
        sel_offsets = self._as_dev(sel_offsets, torch.int64).reshape(-1)
        records, info = self._as_dev(records, torch.int32), self._as_dev(info, torch.int32)
        n_rec = records.shape[0]
        if sel_offsets.numel() != n_reads + 1 or records.dim() != 2 or records.shape[1] != 12 or info.shape != (n_rec, 8):
            raise ValueError("sel_offsets needs N + 1 entries, records must be [R, 12] and info [R, 8], as map_records returns them")
        if sam is not None:
            sam = self._as_dev(sam, torch.int32)
            if sam.shape != (n_rec, 4) or n_reads % 2:
                raise ValueError("sam must be [R, 4] for an even number of reads: mates are interleaved")
        cigar_offsets = self._as_dev(cigar_offsets, torch.int64).reshape(-1)
        if cigar_offsets.numel() != n_rec + 1:
            raise ValueError("cigar_offsets needs one entry more than there are records")
        if isinstance(cigar, torch.Tensor) and cigar.dtype == torch.uint32:
            cigar = cigar.view(torch.int32)
        cigar = self._as_dev(cigar, torch.int32).reshape(-1)
        if quals is not None:
            quals = self._as_dev(quals, torch.uint8).reshape(-1)
            if quals.numel() != total:
                raise ValueError("quals must be parallel to bases")
            if total == 0:
                quals = torch.zeros(1, dtype=torch.uint8, device=self.device)      # an address: NULL would mean `*`
        names, contig_names = self._as_dev(names, torch.uint8).reshape(-1), self._as_dev(contig_names, torch.uint8).reshape(-1)
        name_offsets = self._as_dev(name_offsets, torch.int64).reshape(-1)
        contig_name_offsets = self._as_dev(contig_name_offsets, torch.int64).reshape(-1)
        table = (C.c_void_p(0), 0)
        if contigs is not None:
            off, table = self._contig_table(contigs)
        if name_offsets.numel() != n_reads + 1 or contig_name_offsets.numel() != max(table[1], 1) + 1:
            raise ValueError("one name per read and one per contig")
        none = C.c_void_p(0)
        opt = lambda t: _ptr(t) if t is not None and t.numel() else none      # noqa: E731
        line_offsets = torch.empty(n_reads + n_rec + 1, dtype=torch.int64, device=self.device)
        totals = torch.empty(3, dtype=torch.int64, device=self.device)
        ws, ws_bytes = self._workspace(entry + "_workspace_bytes", n_reads, n_rec)
        if sam is not None and n_rec == 0:
            sam = torch.zeros((1, 4), dtype=torch.int32, device=self.device)       # an address: NULL is single-end mode
        head = (*table, _ptr(bases), _ptr(read_offsets), n_reads, total, _ptr(quals), _ptr(sel_offsets),
                opt(records), n_rec, _ptr(sam), opt(info), _ptr(cigar_offsets), opt(cigar), cigar.numel(),
                opt(names), _ptr(name_offsets), names.numel(), opt(contig_names), _ptr(contig_name_offsets), contig_names.numel(),
                int(tags), 0 if seq else N.SAM_NO_SEQ, _ptr(line_offsets))
        self._run(entry, *head, none, 0, _ptr(totals), _ptr(ws), ws_bytes)
        n_lines, n_bytes, _ = (int(x) for x in totals.cpu())
        text = torch.empty(max(n_bytes, 1), dtype=torch.uint8, device=self.device)
        self._run(entry, *head, _ptr(text), n_bytes, _ptr(totals), _ptr(ws), ws_bytes)
        return text[:n_bytes], line_offsets[:n_lines + 1], totals

    def contig_coords(self, contigs, pos, stride=1):
        """1-based concatenation positions -> int32 [count, 2] = (contig, 1-based offset inside it) on the device
        (genie_contig_coords); (-1, -1) for a position outside [1, n].  pos: int32, flat; with stride > 1 every stride-th
        element from the first on is taken (stride 4 on find_mems rows [R, 4][:, 2:] -- or simply pass rows[:, 2])."""
        off, table = self._contig_table(contigs)
        pos = self._as_dev(pos, torch.int32).reshape(-1)
        stride = int(stride)
        if stride < 1:
            raise ValueError("stride must be at least 1")
        count = (pos.numel() + stride - 1) // stride
        out = torch.empty((count, 2), dtype=torch.int32, device=self.device)
        self._run("genie_contig_coords", *table, _ptr(pos), stride, count, _ptr(out))
        return out

    def segment_coords(self, segments, values, form="positions", stride=None):
        """Squeezed coordinates -> int64 [count, 2] = (record, 1-based offset inside the GIVEN record, breaks counted) on
        the device (genie_segment_coords; segments: the SegmentedReferenceSet this index was built from).  form
        "positions": values are 1-based positions in the squeezed concatenation, int32, flat, every stride-th taken
        (default 1); form "hits": values are locate_contigs hits [T, 2] = (segment, 1-based offset inside it), stride
        (default 2) int32 values apart.  (-1, -1) for a position outside [1, n], a segment outside the table or an offset
        outside its segment."""
        off, table = self._contig_table(segments)
        if form not in N.SEG_FORMS:
            raise ValueError(f"form must be one of {sorted(N.SEG_FORMS)}, got {form!r}")
        least = 2 if form == "hits" else 1
        stride = least if stride is None else int(stride)
        if stride < least:
            raise ValueError(f"stride must be at least {least}")
        values = self._as_dev(values, torch.int32).reshape(-1)
        count = (values.numel() + stride - 1) // stride if form == "positions" else (values.numel() + stride - 2) // stride
        rec, org = segments.device_segments(self.device)
        out = torch.empty((count, 2), dtype=torch.int64, device=self.device)
        self._run("genie_segment_coords", table[0], _ptr(rec), _ptr(org), table[1], N.SEG_FORMS[form], _ptr(values), stride, count,
                  _ptr(out))
        return out

    def exact_match(self, bases, pattern_offsets, both_strands=False, counts=False):
        """Suffix-array interval of every pattern of a CSR batch (genie_exact_match) -> (lohi int32[S*N, 2], counts
        int32[S*N] or None without counts=True, status int32[S*N]) on the device, S = 2 with both_strands, else 1.  bases:
        uint8 codes of all patterns back to back; pattern_offsets: int64[N+1], pattern i = bases[pattern_offsets[i] ..
        pattern_offsets[i+1]), any length; either on the device or the host.  Row S*i + s is pattern i (s = 0) or its reverse
        complement (s = 1): lohi as sa_interval -- (-1, -1) absent, (0, n) the empty pattern, (-2, -2) and status
        READ_BAD_BASE for a code > 3 --, counts = hi - lo + 1 (0 where absent or bad)."""
        bases, pattern_offsets, n_pat, total, max_len, flags, strands = self._csr_call(bases, pattern_offsets, both_strands,
                                                                                      name="pattern_offsets")
        lohi =torch.empty((strands * n_pat, 2), dtype=torch.int32, device=self.device)
        cnt = torch.empty(strands * n_pat, dtype=torch.int32, device=self.device) if counts else None
        status = torch.empty(strands * n_pat, dtype=torch.int32, device=self.device)
        ws, ws_bytes = self._workspace("genie_exact_match_workspace_bytes", n_pat, total, max_len, flags)
        self._run("genie_exact_match", flags, _ptr(bases), _ptr(pattern_offsets), n_pat, total, max_len, _ptr(lohi), _ptr(cnt),
                  _ptr(status), _ptr(ws), ws_bytes)
        return lohi, cnt, status

    def find_smems_packed(self, mode, packed, max_len, lens=None, min_len=1, rows_hint=None, row_bytes=8):
        """genie_find_smems_packed (or, `row_bytes` = 6, genie_find_smems_packed6): 2-bit packed reads (packing.pack_reads;
        uint8 [N, stride] on the device) -> (counts8 uint8[N], status8 uint8[N], rows uint8[S, row_bytes], escapes int64[E, 2]);
        packing.unpack_rows turns them into the offsets / int32 rows of find_smems.  Reads of at most 255 bases."""
        if row_bytes not in (6, 8):
            raise ValueError("row_bytes is 6 or 8")
        entry = "genie_find_smems_packed" if row_bytes == 8 else "genie_find_smems_packed6"
        self._need_device()
        packed = self._as_dev(packed, torch.uint8)
        if packed.dim() != 2:
            raise ValueError("packed reads must be [N, stride]")
        n_reads, stride = packed.shape
        if lens is not None:
            lens = self._as_dev(lens, torch.int32)
        counts8 = torch.zeros(n_reads, dtype=torch.uint8, device=self.device)
        status8 = torch.zeros(n_reads, dtype=torch.uint8, device=self.device)
        totals = torch.zeros(2, dtype=torch.int64, device=self.device)
        if n_reads == 0:
            return counts8, status8, torch.zeros((0, row_bytes), dtype=torch.uint8, device=self.device), torch.zeros((0, 2), dtype=torch.int64, device=self.device)
        ws, ws_bytes = self._workspace("genie_find_smems_workspace_bytes", n_reads, int(max_len))
        cap_rows = int(rows_hint) if rows_hint else n_reads * max(8, int(max_len) // 6)
        cap_esc = 1024
        while True:
            rows8 = torch.empty((max(cap_rows, 1), row_bytes), dtype=torch.uint8, device=self.device)
            esc = torch.empty((max(cap_esc, 1), 2), dtype=torch.int64, device=self.device)
            self._run(entry, N.MODES[mode], _ptr(packed), _ptr(lens), n_reads, stride, int(max_len), int(min_len),
                      _ptr(counts8), _ptr(status8), _ptr(rows8), rows8.shape[0], _ptr(totals), _ptr(esc), esc.shape[0],
                      _ptr(ws), ws_bytes)
            total, n_esc = (int(x) for x in totals.cpu())
            if total <= rows8.shape[0] and n_esc <= esc.shape[0]:
                return counts8, status8, rows8[:total], esc[:n_esc]
            cap_rows, cap_esc = max(cap_rows, total), max(cap_esc, n_esc)      # too small: rerun with the exact sizes

    def find_smems_host(self, mode, codes, lens=None, min_len=1):
        """Host arrays in, host arrays out, through the packed entry point (what SMEM.find_smems_* does with host inputs):
        codes uint8 [N, L] (L <= 255) -> (offsets int64[N+1], rows int32[S, 4], status int32[N]) as numpy arrays."""
        from . import packing
        codes = np.ascontiguousarray(codes, np.uint8)
        packed = torch.as_tensor(packing.pack_reads(codes))
        rb = 6 if self.n + 1 < (1 << 24) else 8                     # the 6-byte rows hold lo in 24 bits
        c8, s8, r8, esc = self.find_smems_packed(mode, packed, codes.shape[1], lens=lens, min_len=min_len, row_bytes=rb)
        offsets, rows = packing.unpack_rows(c8.cpu().numpy(), r8.cpu().numpy(), esc.cpu().numpy(), row_bytes=rb)
        return offsets, rows, s8.cpu().numpy().astype(np.int32)

    def set_option(self, option, value):
        N.check(N.lib().genie_index_set_option(self._h, int(option), int(value)), "genie_index_set_option")

    @staticmethod
    def workspace_shape(max_len):
        """Per-read rows of the find_smems workspace (bytes / counts), for traffic accounting."""
        out = (C.c_int32 * 4)()
        N.check(N.lib().genie_find_smems_workspace_rows(int(max_len), out), "genie_find_smems_workspace_rows")
        return {"fwd_stride": out[0], "qp_recs": out[1], "kj_row_bytes": out[3]}

    def search_kernel_name(self, mode, max_len):
        buf = C.create_string_buffer(160)
        N.check(N.lib().genie_search_kernel_name(self._h, N.MODES[mode], int(max_len), buf, 160), "genie_search_kernel_name")
        return buf.value.decode()

    def launch_info(self, mode, max_len):
        g, b, l = C.c_int32(), C.c_int32(), C.c_int32()
        N.check(N.lib().genie_launch_info(self._h, N.MODES[mode], int(max_len), C.byref(g), C.byref(b), C.byref(l)),
                "genie_launch_info")
        return {"grid": g.value, "block": b.value, "lds_bytes": l.value}
