"""The specification of genie_reads_from_text (include/genie_smem.h) restated in Python, and raw calls of the C entry
point, for tests/test_text_reads_*.py.  parse() never calls the code under test: lines come from bytes.find, codes from a
numpy table lookup."""
import ctypes as C

import numpy as np

import ingest_calls

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


CALL = ingest_calls.Call("genie_reads_from_text", [("int64", 1)], 5)
tmp_bytes = CALL.tmp_bytes


def raw_call(lib, text_ptr, nbytes, fmt, flags, table, bases_ptr, cap_bases, offs_ptr, cap_reads, tmp_ptr, tmp_len, stream=None):
    """One call on raw addresses -> (status, out5 list)."""
    table = np.ascontiguousarray(table, np.uint8)
    return CALL.raw(lib, text_ptr, nbytes, (fmt, flags, table.ctypes.data_as(C.c_void_p)), bases_ptr, cap_bases, [offs_ptr], cap_reads,
                    tmp_ptr, tmp_len, stream)


def device_parse(lib, text, fmt, flags=0, table=ACGT4):
    """CALL.run with the sizes the sizing call reported -> (status, out5, read_offsets, bases) as numpy, like parse()."""
    text, table = bytes(text), np.ascontiguousarray(table, np.uint8)
    rc, out5, b, (o,) = CALL.run(lib, text, (fmt, flags, table.ctypes.data_as(C.c_void_p)), lambda cap: tmp_bytes(lib, len(text), cap))
    return rc, out5, o[:out5[0] + 1], b[:out5[1]]


def same_as_model(lib, text, fmt, flags=0, table=ACGT4):
    return ingest_calls.same(device_parse(lib, text, fmt, flags, table), parse(text, fmt, flags, table), ("offsets", "bases"))
