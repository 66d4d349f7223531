"""The specification of genie_reads_from_fasta (include/genie_smem.h) restated in Python, and raw calls of the C entry
point, for tests/test_fasta_reads_*.py.  parse() never calls the code under test: lines come from text_util.lines_of
(bytes.find), codes from a numpy table lookup."""
import ctypes as C

import numpy as np

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


def tmp_bytes(lib, nbytes, cap_reads):
    return int(lib.genie_reads_from_fasta_tmp_bytes(nbytes, cap_reads))


def raw_call(lib, text_ptr, nbytes, flags, table, bases_ptr, cap_bases, offs_ptr, starts_ptr, cap_reads, tmp_ptr, tmp_len, stream=None):
    """One call on raw addresses -> (status, out5 list)."""
    out5 = (C.c_int64 * 5)(-99, -99, -99, -99, -99)
    table = np.ascontiguousarray(table, np.uint8)
    rc = lib.genie_reads_from_fasta(C.c_void_p(text_ptr), nbytes, flags, table.ctypes.data_as(C.c_void_p), C.c_void_p(bases_ptr),
                                    cap_bases, C.c_void_p(offs_ptr), C.c_void_p(starts_ptr), cap_reads, out5, C.c_void_p(tmp_ptr),
                                    tmp_len, C.c_void_p(stream) if stream else None)
    return rc, list(out5)


def device_parse(lib, text, flags=0, table=ACGT4, fill=0xA5):
    """The sizing call, then the full call into buffers of exactly the sizes it reported, on the current torch stream
    -> (status, out5, read_offsets, bases, record_starts) as numpy, like parse().  Asserts that the two calls agree and
    that the outputs' slack (one int64 past the offsets and past the starts, 8 bytes past the bases) keeps its fill."""
    import torch
    text = bytes(text)
    t = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).cuda() if text else torch.zeros(1, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    tb = tmp_bytes(lib, len(text), 0)
    tmp = torch.empty(max(tb, 256), dtype=torch.uint8, device="cuda")
    rc0, size5 = raw_call(lib, t.data_ptr() if text else 0, len(text), flags, table, 0, 0, 0, 0, 0, tmp.data_ptr(), tb, stream)
    n, total = size5[0], size5[1]
    assert n >= 0 and total >= 0
    offs = torch.full((n + 2,), -77, dtype=torch.int64, device="cuda")
    starts = torch.full((n + 1,), -55, dtype=torch.int64, device="cuda")
    bases = torch.full((total + 8,), fill, dtype=torch.uint8, device="cuda")
    tb = tmp_bytes(lib, len(text), n)
    tmp = torch.empty(max(tb, 256), dtype=torch.uint8, device="cuda")
    rc, out5 = raw_call(lib, t.data_ptr() if text else 0, len(text), flags, table, bases.data_ptr(), total, offs.data_ptr(),
                        starts.data_ptr(), n, tmp.data_ptr(), tb, stream)
    assert (rc, out5) == (rc0, size5), "the sizing call and the full call disagree"
    o, b, s = offs.cpu().numpy(), bases.cpu().numpy(), starts.cpu().numpy()
    assert o[n + 1] == -77 and s[n] == -55 and (b[total:] == fill).all(), "written past the outputs"
    return rc, out5, o[:n + 1], b[:total], s[:n]


def same_as_model(lib, text, flags=0, table=ACGT4):
    want = parse(text, flags, table)
    got = device_parse(lib, text, flags, table)
    assert got[0] == want[0], (got[0], want[0], got[1], want[1])
    assert got[1] == want[1], (got[1], want[1])
    if want[0] == OK:
        assert np.array_equal(got[2], want[2]), "offsets"
        assert np.array_equal(got[3], want[3]), "bases"
        assert np.array_equal(got[4], want[4]), "record starts"
    return want
