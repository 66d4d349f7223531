"""The specification of genie_reads_from_fasta (include/genie_smem.h) restated in Python, and raw calls of the C entry
point, for tests/test_fasta_reads_*.py.  parse() never calls the code under test: lines come from text_util.lines_of
(bytes.find), codes from a numpy table lookup."""
import ctypes as C

import numpy as np

import ingest_calls
from text_util import ACGT4, E_CAPACITY, E_INVALID, OK, PARTIAL, lines_of, reads_of  # noqa: F401  (re-exported)


def parse(text, flags=0, table=ACGT4):
    """-> (status, out5, read_offsets int64[N + 1], bases uint8[total], record_starts int64[N]) as the specification has
    them.  A malformed text keeps its records (the bytes in front of the first header belong to none), so out5[0 .. 3]
    are defined for it too."""
    text = bytes(text)
    partial = bool(flags & PARTIAL)
    lines, _ = lines_of(text, partial)
    headers = [j for j, (a, b) in enumerate(lines) if b > a and text[a] == ord(">")]
    first = headers[0] if headers else len(lines)
    bad = 0 if any(b > a for a, b in lines[:first]) else -1
    n = max(len(headers) - 1, 0) if partial else len(headers)
    consumed = len(text) if not partial else (lines[headers[-1]][0] if headers else 0)
    codes = np.where(np.asarray(table, np.uint8) <= 3, np.asarray(table, np.uint8), np.uint8(4))
    ends = headers[1:] + [len(lines)]
    reads = [b"".join(text[a:b] for a, b in lines[headers[r] + 1:ends[r]]) for r in range(n)]
    offs = np.zeros(n + 1, np.int64)
    offs[1:] = np.cumsum([len(r) for r in reads]) if reads else []
    bases = codes[np.frombuffer(b"".join(reads), np.uint8)].astype(np.uint8)
    starts = np.asarray([lines[headers[r]][0] for r in range(n)], np.int64)
    out5 = [n, int(offs[-1]), max([len(r) for r in reads] + [0]), consumed, bad]
    return (E_INVALID if bad == 0 else OK), out5, offs, bases, starts


def names_of(text, starts):
    """The records' names: the bytes behind the '>' up to the first space, tab, '\\r' or '\\n'."""
    out = []
    for s in starts:
        e = s + 1
        while e < len(text) and text[e] not in b" \t\r\n":
            e += 1
        out.append(bytes(text[s + 1:e]))
    return out


CALL = ingest_calls.Call("genie_reads_from_fasta", [("int64", 1), ("int64", 0)], 5)
tmp_bytes = CALL.tmp_bytes


def raw_call(lib, text_ptr, nbytes, flags, table, bases_ptr, cap_bases, offs_ptr, starts_ptr, cap_reads, tmp_ptr, tmp_len, stream=None):
    """One call on raw addresses -> (status, out5 list)."""
    table = np.ascontiguousarray(table, np.uint8)
    return CALL.raw(lib, text_ptr, nbytes, (flags, table.ctypes.data_as(C.c_void_p)), bases_ptr, cap_bases, [offs_ptr, starts_ptr],
                    cap_reads, tmp_ptr, tmp_len, stream)


def device_parse(lib, text, flags=0, table=ACGT4):
    """CALL.run with the sizes the sizing call reported -> (status, out5, read_offsets, bases, record_starts), like parse()."""
    text, table = bytes(text), np.ascontiguousarray(table, np.uint8)
    rc, out5, b, (o, s) = CALL.run(lib, text, (flags, table.ctypes.data_as(C.c_void_p)), lambda cap: tmp_bytes(lib, len(text), cap))
    return rc, out5, o[:out5[0] + 1], b[:out5[1]], s[:out5[0]]


def same_as_model(lib, text, flags=0, table=ACGT4):
    return ingest_calls.same(device_parse(lib, text, flags, table), parse(text, flags, table), ("offsets", "bases", "record starts"))
