"""The specification of genie_reads_from_text (include/genie_smem.h) restated in Python, and raw calls of the C entry
point, for tests/test_text_reads_*.py.  parse() never calls the code under test: lines come from bytes.find, codes from a
numpy table lookup."""
import ctypes as C

import numpy as np

LINES, FASTQ = 0, 1
PARTIAL = 1
OK, E_INVALID, E_CAPACITY = 0, -1, -10
FORMATS = (LINES, FASTQ)

ACGT4 = np.full(256, 4, np.uint8)
for _i, _ch in enumerate(b"ACGT"):
    ACGT4[_ch] = _i

# lower case, N, a quality line that starts with '@' and holds '+', a CRLF record, an empty read
MIXED_FASTQ = (b"@r0\nACGTN\n+\n@+III\n@r1 x\r\nacgT\r\n+r1\r\n!!!!\r\n@r2\n\n+\n\n"
               b"@r3\nGGNNAC\x00\xffT\n+\nIIIIIIIII\n")


def lines_of(text, partial):
    """[(start, end)] of the lines and the start of the tail."""
    text = bytes(text)
    out, at = [], 0
    while True:
        nl = text.find(b"\n", at)
        if nl < 0:
            break
        end = nl
        if end > at and text[end - 1] == 0x0D:
            end -= 1
        out.append((at, end))
        at = nl + 1
    tail = at
    if not partial and at < len(text):
        out.append((at, len(text)))                                 # no '\r' is dropped from the tail
    return out, tail


def parse(text, fmt, flags=0, table=ACGT4):
    """-> (status, out5, read_offsets int64[N + 1], bases uint8[total]) as the specification has them."""
    text = bytes(text)
    partial = bool(flags & PARTIAL)
    lines, tail = lines_of(text, partial)
    bad = -1
    if fmt == LINES:
        reads = lines
        consumed = tail if partial else len(text)
    else:
        n = len(lines) // 4
        reads = [lines[4 * r + 1] for r in range(n)]
        for r in range(n):
            (h0, h1), (p0, p1) = lines[4 * r], lines[4 * r + 2]
            if h1 == h0 or text[h0] != ord("@") or p1 == p0 or text[p0] != ord("+"):
                bad = r
                break
        if bad < 0 and not partial and len(lines) % 4:
            bad = n
        if partial:
            consumed = lines[4 * n][0] if len(lines) > 4 * n else tail
        else:
            consumed = len(text)
    raw = np.frombuffer(text, np.uint8)
    codes = np.where(np.asarray(table, np.uint8) <= 3, np.asarray(table, np.uint8), np.uint8(4))
    parts = [codes[raw[a:b]] for a, b in reads]
    offs = np.zeros(len(reads) + 1, np.int64)
    offs[1:] = np.cumsum([b - a for a, b in reads]) if reads else []
    bases = np.concatenate(parts).astype(np.uint8) if parts else np.zeros(0, np.uint8)
    out5 = [len(reads), int(offs[-1]), max([b - a for a, b in reads] + [0]), consumed, bad]
    return (E_INVALID if bad >= 0 else OK), out5, offs, bases


def reads_of(offs, bases):
    return [bytes(bases[offs[r]:offs[r + 1]]) for r in range(len(offs) - 1)]


def tmp_bytes(lib, nbytes, cap_reads):
    return int(lib.genie_reads_from_text_tmp_bytes(nbytes, cap_reads))


def raw_call(lib, text_ptr, nbytes, fmt, flags, table, bases_ptr, cap_bases, offs_ptr, cap_reads, tmp_ptr, tmp_len, stream=None):
    """One call on raw addresses -> (status, out5 list)."""
    out5 = (C.c_int64 * 5)(-99, -99, -99, -99, -99)
    table = np.ascontiguousarray(table, np.uint8)
    rc = lib.genie_reads_from_text(C.c_void_p(text_ptr), nbytes, fmt, flags, table.ctypes.data_as(C.c_void_p),
                                   C.c_void_p(bases_ptr), cap_bases, C.c_void_p(offs_ptr), cap_reads, out5,
                                   C.c_void_p(tmp_ptr), tmp_len, C.c_void_p(stream) if stream else None)
    return rc, list(out5)


def device_parse(lib, text, fmt, flags=0, table=ACGT4, fill=0xA5):
    """The sizing call, then the full call into buffers of exactly the sizes it reported, on the current torch stream
    -> (status, out5, read_offsets, bases) as numpy, like parse().  Asserts that the two calls agree on out5 and that
    the outputs' slack (one int64 past the offsets, 8 bytes past the bases) keeps its fill."""
    import torch
    text = bytes(text)
    t = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).cuda() if text else torch.zeros(1, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    tb = tmp_bytes(lib, len(text), 0)
    tmp = torch.empty(max(tb, 256), dtype=torch.uint8, device="cuda")
    rc0, size5 = raw_call(lib, t.data_ptr() if text else 0, len(text), fmt, flags, table, 0, 0, 0, 0, tmp.data_ptr(), tb, stream)
    n, total = size5[0], size5[1]
    assert n >= 0 and total >= 0
    offs = torch.full((n + 2,), -77, dtype=torch.int64, device="cuda")
    bases = torch.full((total + 8,), fill, dtype=torch.uint8, device="cuda")
    tb = tmp_bytes(lib, len(text), n)
    tmp = torch.empty(max(tb, 256), dtype=torch.uint8, device="cuda")
    rc, out5 = raw_call(lib, t.data_ptr() if text else 0, len(text), fmt, flags, table, bases.data_ptr(), total, offs.data_ptr(), n,
                        tmp.data_ptr(), tb, stream)
    assert (rc, out5) == (rc0, size5), "the sizing call and the full call disagree"
    o, b = offs.cpu().numpy(), bases.cpu().numpy()
    assert o[n + 1] == -77 and (b[total:] == fill).all(), "written past the outputs"
    return rc, out5, o[:n + 1], b[:total]


def same_as_model(lib, text, fmt, flags=0, table=ACGT4):
    want = parse(text, fmt, flags, table)
    got = device_parse(lib, text, fmt, flags, table)
    assert got[0] == want[0], (got[0], want[0], got[1], want[1])
    assert got[1] == want[1], (got[1], want[1])
    if want[0] == OK:
        assert np.array_equal(got[2], want[2]), "offsets"
        assert np.array_equal(got[3], want[3]), "bases"
    return want
