"""Reads from text on the device (genie_reads_from_text, genie_reads_from_fasta): the bytes of a file with one read per
line, of a FASTQ file with four-line records, or of a FASTA file whose sequences are wrapped over any number of lines,
become base codes back to back and int64 offsets -- the (bases, read_offsets) that GenieIndex.find_smems_long takes.  The
text travels over the host link as it is, one byte per base; nothing is encoded on the host."""
import ctypes as C
import re
import warnings

import numpy as np
import torch

from . import _native as N


class TextFormatError(ValueError):
    """A malformed FASTQ record or FASTA text (GENIE_E_INVALID found on the device); `record` is the first bad record
    (FASTA: 0, the text does not begin with a header line)."""

    def __init__(self, record, fmt):
        self.record = int(record)
        if fmt == "fasta":
            why = "a non-empty line stands in front of the first '>' header line"
        else:
            why = ("a header line must start with '@', a separator line with '+', and without partial=True the last record "
                   "must be complete")
        super().__init__(f"{fmt} text: record {self.record} is malformed ({why})")


def _text_tensor(data, device):
    """bytes-like | numpy uint8 | torch uint8 (host or device) -> flat uint8 tensor on `device`."""
    if isinstance(data, torch.Tensor):
        if data.dtype != torch.uint8:
            raise TypeError("text tensor must be uint8")
        return data.reshape(-1).to(device).contiguous()
    if isinstance(data, np.ndarray):
        if data.dtype != np.uint8:
            raise TypeError("text array must be uint8")
        a = np.ascontiguousarray(data).reshape(-1)
    else:
        a = np.frombuffer(data, np.uint8)                   # bytes, bytearray, memoryview, mmap
    if a.size == 0:
        return torch.zeros(0, dtype=torch.uint8, device=device)
    with warnings.catch_warnings():                         # a read-only buffer (bytes): it is only read, by the upload
        warnings.simplefilter("ignore", UserWarning)
        return torch.from_numpy(a).to(device)


FORMATS = tuple(N.TEXT_FORMATS) + ("fasta",)
_NAME = re.compile(rb"[^ \t\r\n]*")


def reads_from_text(data, fmt="lines", code_of_byte=None, partial=False, device="cuda", return_starts=False):
    """-> (bases uint8[total_bases], read_offsets int64[N + 1], consumed): two tensors on `device` and a byte count.
    data: bytes-like, numpy uint8 or torch uint8 (host or device).  fmt: "lines" (every line a read), "fastq" (four-line
    records) or "fasta" ('>' header lines, sequences wrapped over any number of lines).  code_of_byte: 256 uint8 entries
    (ExactMatch.byte_codes(); default A C G T -> 0 1 2 3, anything else 4).  partial: the text is a chunk of a longer stream
    -- the unfinished last line (record) is left alone and `consumed` says where it starts.  return_starts ("fasta" only):
    a fourth value, record_starts int64[N] on `device`, the text position of every record's '>' (see record_names).  Two
    native calls: one sizes the outputs, one fills them.  A malformed FASTQ or FASTA raises TextFormatError."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("reads_from_text runs on an MI355X only (no CPU fallback); device is " + str(device))
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if fmt not in FORMATS:
        raise ValueError(f"fmt must be one of {sorted(FORMATS)}, got {fmt!r}")
    fasta = fmt == "fasta"
    if return_starts and not fasta:
        raise ValueError("return_starts needs fmt='fasta'")
    if code_of_byte is None:
        code_of_byte = default_byte_codes()
    table = np.ascontiguousarray(code_of_byte, np.uint8)
    if table.shape != (256,):
        raise ValueError("code_of_byte needs 256 entries")
    lib = N.lib()
    text = _text_tensor(data, device)
    nbytes = text.numel()
    flags = N.TEXT_PARTIAL if partial else 0
    out5 = (C.c_int64 * 5)()
    name = "genie_reads_from_fasta" if fasta else "genie_reads_from_text"
    size_of = getattr(lib, name + "_tmp_bytes")

    def call(bases, offsets, starts, cap_bases, cap_reads):
        tmp_bytes = int(size_of(nbytes, cap_reads))
        tmp = torch.empty(max(tmp_bytes, 256), dtype=torch.uint8, device=device)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else C.c_void_p(0)
        out5[4] = -1
        tab = table.ctypes.data_as(C.c_void_p)
        stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        with torch.cuda.device(device):
            if fasta:
                rc = lib.genie_reads_from_fasta(ptr(text), nbytes, flags, tab, ptr(bases), cap_bases, ptr(offsets), ptr(starts),
                                                cap_reads, out5, ptr(tmp), tmp_bytes, stream)
            else:
                rc = lib.genie_reads_from_text(ptr(text), nbytes, N.TEXT_FORMATS[fmt], flags, tab, ptr(bases), cap_bases,
                                               ptr(offsets), cap_reads, out5, ptr(tmp), tmp_bytes, stream)
        if rc == -1 and out5[4] >= 0:
            raise TextFormatError(out5[4], fmt)
        N.check(rc, name)

    call(None, None, None, 0, 0)
    n_reads, total = int(out5[0]), int(out5[1])
    bases = torch.empty(max(total, 1), dtype=torch.uint8, device=device)     # a pointer even for no bases
    offsets = torch.empty(n_reads + 1, dtype=torch.int64, device=device)
    starts = torch.empty(n_reads, dtype=torch.int64, device=device) if return_starts else None
    call(bases, offsets, starts, total, n_reads)
    if return_starts:
        return bases[:total], offsets, int(out5[3]), starts
    return bases[:total], offsets, int(out5[3])


def record_names(data, record_starts):
    """The names of FASTA records, on the host: for each text position in record_starts (of a record's '>', as
    reads_from_text(..., "fasta", return_starts=True) gives them) the bytes behind the '>' up to the first space, tab, '\\r'
    or '\\n' (or the text's end).  data: the bytes-like text those positions refer to.  -> list[bytes]."""
    text = data if isinstance(data, (bytes, bytearray)) else memoryview(data).cast("B")
    if isinstance(record_starts, torch.Tensor):
        record_starts = record_starts.cpu().tolist()
    names = []
    for at in record_starts:
        at = int(at)
        if not 0 <= at < len(text) or text[at] != 0x3E:
            raise ValueError(f"no '>' at text position {at}")
        names.append(bytes(_NAME.match(text, at + 1).group()))
    return names


def interleave_reads(csr1, csr2):
    """Two batches (bases, read_offsets) of equally many reads -> the interleaved batch (bases uint8, read_offsets int64[2n+1]):
    read 2k is read k of the first and read 2k + 1 read k of the second, the convention of the paired calls, so the two files
    of a paired run become one batch.  Torch calls on the tensors' device only: nothing per read on the host."""
    (b1, o1), (b2, o2) = csr1, csr2
    o1 = torch.as_tensor(o1).to(torch.int64).reshape(-1)
    dev = o1.device
    o2 = torch.as_tensor(o2).to(device=dev, dtype=torch.int64).reshape(-1)
    b1 = torch.as_tensor(b1).to(device=dev, dtype=torch.uint8).reshape(-1)
    b2 = torch.as_tensor(b2).to(device=dev, dtype=torch.uint8).reshape(-1)
    if o1.numel() < 1 or o1.numel() != o2.numel():
        raise ValueError("the two batches must hold equally many reads")
    n = o1.numel() - 1
    len1, len2 = o1[1:] - o1[:-1], o2[1:] - o2[:-1]
    offsets = torch.zeros(2 * n + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(torch.stack([len1, len2], 1).reshape(-1), 0)
    # per base of a batch: how far its read moved; the bases of a batch are those its offsets name, from position 0 on
    shifts = [torch.repeat_interleave(offsets[first:2 * n:2] - o[:-1], lens) for o, lens, first in ((o1, len1, 0), (o2, len2, 1))]
    if shifts[0].numel() > b1.numel() or shifts[1].numel() > b2.numel():
        raise ValueError("read_offsets name more bases than there are")
    bases = torch.empty(shifts[0].numel() + shifts[1].numel(), dtype=torch.uint8, device=dev)
    for b, shift in zip((b1, b2), shifts):
        bases[torch.arange(shift.numel(), device=dev) + shift] = b[:shift.numel()]
    return bases, offsets


def fastq_fields(data, read_offsets, device=None):
    """The names and the qualities of the first N records of a FASTQ text -> (names uint8, name_offsets int64[N + 1], quals
    uint8[total bases]) on `device` (default: where read_offsets lies): what GenieIndex.sam_text takes next to the (bases,
    read_offsets) that reads_from_text made of the same text.  A record's name is the bytes behind its '@' up to the first
    space, tab, '\\r' or the line's end; the quality lines are laid back to back under read_offsets.  Lines are those of
    genie_reads_from_text: a '\\n' ends a line, a '\\r' in front of it is dropped, a non-empty tail is one more line.  Torch
    calls on the device only, nothing per read on the host.  ValueError when the text holds fewer than N records or a
    quality line is not as long as its read: one reduction and one host read.  The qualities of two files go through
    interleave_reads like their bases."""
    read_offsets = torch.as_tensor(read_offsets).to(torch.int64).reshape(-1)
    dev = read_offsets.device if device is None else torch.device(device)
    read_offsets = read_offsets.to(dev)
    text = _text_tensor(data, dev)
    n, size = read_offsets.numel() - 1, text.numel()
    if n < 0:
        raise ValueError("read_offsets needs N + 1 entries")
    i64 = lambda *v: torch.tensor(v, dtype=torch.int64, device=dev)      # noqa: E731
    ends = torch.nonzero(text == 10).reshape(-1)
    starts = torch.cat([i64(0), ends + 1])
    closed = ends.numel()                                   # lines that a '\n' ends; the tail is one more where it is not empty
    cr = torch.zeros(closed, dtype=torch.int64, device=dev)
    if closed:
        cr = ((ends > starts[:closed]) & (text[(ends - 1).clamp(min=0)] == 13)).to(torch.int64)
    ends = torch.cat([ends - cr, i64(size)])
    if closed + 1 < 4 * n:                                  # the tail counted: an empty one can only be an empty quality line
        raise ValueError(f"the text holds {(closed + 1) // 4} complete records, read_offsets names {n}")
    q0, q1 = starts[3:4 * n:4], ends[3:4 * n:4]
    # a name ends at the first space, tab or '\r' behind the '@', or where its line ends
    h0 = torch.minimum(starts[0:4 * n:4] + 1, ends[0:4 * n:4])
    stop = torch.nonzero((text == 32) | (text == 9) | (text == 13)).reshape(-1)
    first = torch.cat([stop, i64(size)])[torch.searchsorted(stop, h0)]
    h1 = torch.maximum(torch.minimum(ends[0:4 * n:4], first), h0)
    lens = read_offsets[1:] - read_offsets[:-1]
    if n and bool(((q1 - q0) != lens).any()):
        raise ValueError("a quality line is not as long as its read")

    def gather(begin, length, offsets):
        shift = torch.repeat_interleave(begin - offsets[:-1], length)      # per byte: how far it moves
        return text[torch.arange(shift.numel(), device=dev) + shift]
    name_offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    name_offsets[1:] = torch.cumsum(h1 - h0, 0)
    return gather(h0, h1 - h0, name_offsets), name_offsets, gather(q0, lens, read_offsets)


def default_byte_codes():
    """A C G T -> 0 1 2 3, every other byte 4."""
    table = np.full(256, 4, np.uint8)
    for i, ch in enumerate(b"ACGT"):
        table[ch] = i
    return table
