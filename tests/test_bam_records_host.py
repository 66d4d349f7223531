"""CPU-only tests of genie_bam_records (BAM records on the device) and its host helpers: the brute-force encoder of
tests/bam_util.py decoded by that module's independent decoder gives exactly the text of sam_text_util's brute force, on the
pinned fixture of tests/test_pair_host.py's kind and on random batches, which ties the BAM definition to the SAM one; hand-made
records for bin, POS 0, odd and even lengths on both strands, names and mapq at their limits and the CG convention; bam_header
and bgzf_compress; the symbols and the header's wording; the workspace function; and the C ABI's argument checks in their
documented order (before the device check, so a host-only handle reaches them)."""
import ctypes as C
import gzip
import os
import struct

import numpy as np
import pytest

import bam_util as BU
import sam_text_util as ST

INVALID, NO_DEVICE, CAPACITY, TOO_LONG = ST.INVALID, ST.NO_DEVICE, ST.CAPACITY, ST.TOO_LONG
TABLE = np.asarray([0, 6000, 11000, 16384], np.int64)
EQ, X, D, I, S = ST.EQ, ST.X, ST.D, ST.I, ST.S
op = ST.op


@pytest.fixture(scope="module")
def pkg():
    import genie_smem_amd as g
    g._native.build()
    return g


def _round_trip(b, T, tags, flags=0):
    want = bytes(ST.expected(b, T, tags, flags)["text"]).decode("latin-1").split("\n")
    enc = BU.host_bam_records(b, T, tags, flags)
    got = BU.bam_to_sam(enc["data"], b["contig_names"])
    assert want[-1] == "" and got == want[:-1]
    assert enc["totals"].tolist()[0::2] == ST.expected(b, T, tags, flags)["totals"].tolist()[0::2]
    off = enc["record_offsets"]
    for k in range(off.size - 1):                                    # block_size: the record's length minus 4
        assert struct.unpack_from("<i", enc["data"], int(off[k]))[0] == off[k + 1] - off[k] - 4
    return enc, got


# ------------------------------------------------------------------ the encoder, decoded, is the SAM text
def test_round_trip_on_the_pinned_fixture():
    ops = lambda *v: [op(n, o) for n, o in v]      # noqa: E731
    records = np.asarray([[0, 4, 0, 0, 0, 101, 50, 0, 50, 48, 40, 0], [0, 6, 2, 0, 1, 11, 50, 0, 50, 40, 0, 0],
                          [1, 9, 0, 1, 0, 301, 52, 3, 53, 50, 0, 60], [2, 12, 0, 1, 1, 41, 50, 0, 50, 50, 0, 60]], np.int32)
    sam = np.asarray([[99, 6, 2, 252], [355, 0, 2, 0], [147, 60, 0, -252], [89, 60, -1, 0]], np.int32)
    info = np.asarray([[4, 0, 1, 1, 49, 1, 0, 0], [6, 0, 1, 2, 48, 2, 0, 0], [9, 0, 4, 2, 50, 0, 0, 2], [12, 0, 1, 0, 50, 0, 0, 0]], np.int32)
    cigar = np.asarray(ops((50, 7)) + ops((50, 7)) + ops((3, 4), (20, 7), (2, 2), (30, 7)) + ops((50, 7)), np.uint32)
    b = {"sel_offsets": np.asarray([0, 2, 3, 4, 4], np.int64), "records": records, "sam": sam, "info": info,
         "cigar_offsets": np.asarray([0, 1, 2, 6, 7], np.int64), "cigar": cigar, "names": [b"p0", b"p0", b"p1", b"p1"],
         "contig_names": [b"chrA", b"chrB"], "contig_offsets": np.asarray([0, 500, 1100], np.int64),
         "bases": np.asarray([0, 1, 2, 3, 0, 0, 0, 1, 1, 2, 3, 3, 3, 3, 2, 2, 2, 2, 2, 0], np.uint8),
         "read_offsets": np.asarray([0, 5, 10, 15, 20], np.int64), "quals": np.frombuffer(b"IIIIHABCDEFFFFG#####", np.uint8)}
    T = np.random.default_rng(3).integers(0, 4, 1100).astype(np.uint8)
    for tags in (3, 31, 0, 4, 24):
        enc, lines = _round_trip(b, T, tags)
    _round_trip(b, T, 31, ST.NO_SEQ)
    _round_trip(dict(b, quals=None), T, 31)
    _round_trip(dict(b, sam=None), T, 31)
    # the first record, byte by byte
    enc = BU.host_bam_records(b, T, 3)
    r0 = bytes(enc["data"][:int(enc["record_offsets"][1])])
    assert struct.unpack_from("<iiiBBHHHiiii", r0) == (len(r0) - 4, 0, 100, 3, 6, 4681, 1, 99, 5, 0, 300, 252)
    assert r0[36:39] == b"p0\0" and r0[39:43] == struct.pack("<I", 50 << 4 | 7)
    assert r0[43:46] == bytes([0x12, 0x48, 0x10]) and r0[46:51] == bytes(c - 33 for c in b"IIIIH")      # ACGTA
    assert r0[51:] == b"NMi" + struct.pack("<i", 1) + b"ASi" + struct.pack("<i", 48)
    last = bytes(enc["data"][int(enc["record_offsets"][4]):])                 # the unmapped record, placed at its mate
    assert struct.unpack_from("<iiiBBHHHiiii", last)[1:] == (1, 40, 3, 0, 4681, 0, 165, 5, 1, 40, 0)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_round_trip_on_random_batches(seed):
    rng = np.random.default_rng(300 + seed)
    counts = rng.integers(0, 4, 40).tolist() + [0, 0, 3, 0]
    reads = [(max(n, 1), recs) for n, recs in ST.random_reads(rng, counts, TABLE)]              # reads of at least one base
    names = [b"q" * int(rng.integers(1, 255)) if r % 7 == 0 else f"read{r // 2}".encode() for r in range(len(reads))]
    b = ST.make_batch(rng, reads, names=names, contig_offsets=TABLE, quals=seed != 1, single=seed == 2)
    T = rng.integers(0, 4, int(TABLE[-1])).astype(np.uint8)
    for tags in (3, 31, int(rng.integers(0, 32))):
        _round_trip(b, T, tags)
    _round_trip(b, T, 31, ST.NO_SEQ)


# ------------------------------------------------------------------ records by hand
def _one(ops, offset=1, length=4, strand=0, name=b"r", mapq=30, quals=True, tags=0, codes=None):
    """One mapped read in single-end mode -> (its record's bytes, the decoder's line)."""
    rng = np.random.default_rng(5)
    b = ST.make_batch(rng, [(length, [dict(ops=ops, offset=offset, strand=strand, mapq=mapq)])], names=[name], contig_names=[b"c"],
                      quals=quals, single=True)
    if codes is not None:
        b["bases"] = np.asarray(codes, np.uint8)
    enc = BU.host_bam_records(b, np.zeros(64, np.uint8), tags)
    assert enc["record_offsets"].size == 2
    return bytes(enc["data"]), BU.bam_to_sam(enc["data"], [b"c"])[0].split("\t"), b


def _bin(raw):
    return struct.unpack_from("<H", raw, 14)[0]


def test_bin_at_the_level_boundaries():
    first = {14: 4681, 17: 585, 20: 73, 23: 9, 26: 1}
    for shift, base in first.items():
        edge = 1 << shift
        # [edge - 100, edge): ends on the boundary, still one bin of this level
        raw, cols, _ = _one([op(100, EQ)], offset=edge - 100 + 1)
        want = 4681 + ((edge - 100) >> 14)
        assert _bin(raw) == want & 0xffff and int(cols[3]) == edge - 99
        # [edge - 100, edge + 1): crosses it, so the bin is of the next coarser level (2^shift is no boundary of that one)
        raw, cols, _ = _one([op(60, EQ), op(1, D), op(40, X)], offset=edge - 100 + 1)
        up = shift + 3
        assert _bin(raw) == (0 if up > 26 else first[up] + ((edge - 100) >> up)) == BU.reg2bin(edge - 100, edge + 1)
    assert BU.reg2bin(0, 1) == 4681 and BU.reg2bin(-1, 0) == 4680 and BU.reg2bin(0, 1 << 29) == 0
    assert BU.reg2bin((1 << 26) - 1, (1 << 26) + 1) == 0 and BU.reg2bin(1 << 26, (1 << 26) + 5) == 4681 + 4096
    assert BU.reg2bin((1 << 14) - 1, (1 << 14) + 1) == 585 and BU.reg2bin((1 << 17) - 1, (1 << 17) + 1) == 73
    assert BU.reg2bin((1 << 20) - 1, (1 << 20) + 1) == 9 and BU.reg2bin((1 << 23) - 1, (1 << 23) + 1) == 1
    # I and S do not count; a record without reference bases covers one position
    raw, _, _ = _one([op(3, S), op(1, I)], offset=(1 << 14) + 1)
    assert _bin(raw) == 4682
    for beg, end in ((0, 1), (5, 1 << 14), (16383, 16385), (1 << 20, (1 << 20) + 1), (123456789, 123456999), (-1, 0), (-70000, -5)):
        assert BU.reg2bin(beg, end) == BU._bin_by_levels(beg, end)


def test_pos_zero_is_minus_one_and_bin_4680():
    rng = np.random.default_rng(6)
    b = ST.make_batch(rng, [(3, []), (2, [])], contig_names=[b"c"])                             # a pair without records
    enc = BU.host_bam_records(b, np.zeros(64, np.uint8), 31)
    raw = bytes(enc["data"])
    head = struct.unpack_from("<iiiBBHHHiiii", raw)
    assert head[1:3] == (-1, -1) and head[5] == 4680 and head[9:11] == (-1, -1) and head[7] == 77
    line = BU.bam_to_sam(raw, [b"c"])[0].split("\t")
    assert line[1:9] == ["77", "*", "0", "0", "*", "*", "0", "0"]
    raw, cols, _ = _one([], offset=0)                                # a record whose POS is 0, without ops: [-1, 0)
    assert struct.unpack_from("<i", raw, 8)[0] == -1 and _bin(raw) == 4680 and cols[3] == "0"
    raw, cols, _ = _one([op(4, EQ)], offset=0)                       # ... with ops [-1, 3): no bin but the root holds it
    assert struct.unpack_from("<i", raw, 8)[0] == -1 and _bin(raw) == 0


def test_seq_of_odd_and_even_length_on_both_strands():
    codes = [0, 1, 2, 3, 4, 0, 0]
    for n in (7, 6, 1, 2):
        for strand in (0, 1):
            raw, cols, b = _one([op(n, EQ)], length=n, strand=strand, codes=codes[:n])
            seq = raw[36 + 2 + 4:36 + 2 + 4 + (n + 1) // 2]
            c = codes[:n]
            if strand:
                c = [3 - v if v < 4 else v for v in c[::-1]]
            nib = [1 << v if v < 4 else 15 for v in c] + [0]
            assert list(seq) == [nib[2 * i] << 4 | nib[2 * i + 1] for i in range((n + 1) // 2)]
            assert cols[9] == "".join("ACGTN"[v] for v in c)
            q = b["quals"] - 33
            assert list(raw[36 + 6 + (n + 1) // 2:][:n]) == list(q[::-1] if strand else q)
    raw, cols, _ = _one([op(4, EQ)], quals=False)
    assert raw[36 + 6 + 2:][:4] == b"\xff" * 4 and cols[10] == "*"
    raw = BU.encode_record(b"r", 0, 0, 0, 0, [], -1, -1, 0, [0, 1], [20, 40], False, b"")     # qualities below 33 are 0
    assert raw[-2:] == bytes([0, 7])


def test_names_and_mapq_at_their_limits():
    long = bytes(65 + k % 26 for k in range(255))
    raw, cols, _ = _one([op(4, EQ)], name=long)
    assert raw[12] == 255 and raw[36:36 + 254] == long[:254] and raw[36 + 254] == 0 and cols[0] == long[:254].decode()
    raw, cols, _ = _one([op(4, EQ)], name=long[:254])
    assert raw[12] == 255 and cols[0] == long[:254].decode()
    raw, cols, _ = _one([op(4, EQ)], name=b"")
    assert raw[12] == 2 and raw[36:38] == b"*\0" and cols[0] == "*"
    raw, cols, _ = _one([op(4, EQ)], mapq=300)
    assert raw[13] == 255 and cols[4] == "255"
    raw, cols, _ = _one([op(4, EQ)], mapq=-3)
    assert raw[13] == 0


def test_cg_by_hand():
    n = 65536
    ops = [op(2, EQ)] * n
    raw, cols, _ = _one(ops, offset=11, length=2 * n, tags=ST.NM | ST.AS)
    l_seq = 2 * n
    assert struct.unpack_from("<H", raw, 16)[0] == 2
    assert struct.unpack_from("<II", raw, 36 + 2) == (l_seq << 4 | 4, (2 * n) << 4 | 3)
    tail = raw[-(8 + 4 * n):]
    assert tail[:4] == b"CGBI" and struct.unpack_from("<i", tail, 4)[0] == n and tail[8:] == struct.pack("<I", 2 << 4 | 7) * n
    assert raw[-(8 + 4 * n) - 14:-(8 + 4 * n)] == b"NMi" + struct.pack("<i", 0) + b"ASi" + struct.pack("<i", 60)      # CG is the last tag
    assert _bin(raw) == BU.reg2bin(10, 10 + 2 * n) & 0xffff == 73
    assert cols[5] == "2=" * n and cols[11:] == ["NM:i:0", "AS:i:60"]                           # the decoder undoes it
    raw, cols, _ = _one(ops[:-1], offset=11, length=2 * n - 2)       # 65535 ops still fit the field
    assert struct.unpack_from("<H", raw, 16)[0] == 65535 and b"CGBI" not in raw[-20:] and cols[5] == "2=" * (n - 1)
    # a span above 2^28 - 1 is cut in the placeholder only
    rec = BU.encode_record(b"r", 0, 0, 0, 0, [op(2**28 - 1, EQ)] * 2 + [op(1, I)] * n, -1, -1, 0, [0], None, False, b"")
    assert struct.unpack_from("<II", rec, 36 + 2) == (1 << 4 | 4, (2**28 - 1) << 4 | 3)


# ------------------------------------------------------------------ the file: header and BGZF
def test_bam_header(pkg):
    h = pkg.bam_header(["chrA", b"chrB"], [500, np.int64(600)])
    text = ("\n".join(pkg.sam_header(["chrA", "chrB"], [500, 600])) + "\n").encode()
    assert h[:4] == b"BAM\1" and struct.unpack_from("<i", h, 4)[0] == len(text) and h[8:8 + len(text)] == text
    at = 8 + len(text)
    assert struct.unpack_from("<i", h, at)[0] == 2
    assert h[at + 4:] == struct.pack("<i", 5) + b"chrA\0" + struct.pack("<i", 500) + struct.pack("<i", 5) + b"chrB\0" + struct.pack("<i", 600)
    assert pkg.bam_header([], [])[-4:] == struct.pack("<i", 0)
    with pytest.raises(ValueError):
        pkg.bam_header(["a"], [])


def test_bgzf_compress(pkg):
    eof = bytes([0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0])
    rng = np.random.default_rng(9)
    for n in (0, 1, 0xff00, 0xff01, 200000):
        # half noise, half runs: neither trivially compressible nor all stored
        data = bytes(rng.integers(0, 256, n // 2, dtype=np.uint8)) + bytes(n - n // 2)
        for level in (0, 1, 6):
            z = pkg.bgzf_compress(data, level, threads=1)
            assert gzip.decompress(z) == data and z[-28:] == eof
            assert z == pkg.bgzf_compress(data, level, threads=4) == pkg.bgzf_compress(memoryview(data), level)
            at, blocks = 0, 0
            while at < len(z):
                assert z[at:at + 4] == b"\x1f\x8b\x08\x04" and z[at + 10:at + 16] == b"\x06\0BC\x02\0"
                bsize = struct.unpack_from("<H", z, at + 16)[0]
                isize = struct.unpack_from("<I", z, at + bsize - 3)[0]
                assert isize <= 0xff00
                at += bsize + 1                                      # BSIZE is the block's length minus 1
                blocks += 1
            assert at == len(z) and blocks == (n + 0xff00 - 1) // 0xff00 + 1
    assert pkg.bgzf_compress(b"") == eof
    # the blocks of several buffers are those of their concatenation, wherever the boundary falls in a payload
    blocks = pkg.index.bgzf_blocks
    body = bytes(rng.integers(0, 256, 3 * 0xff00 + 11, dtype=np.uint8))
    for n_head in (0, 5, 0xff00, 0xff00 + 7, 70000):
        head = bytes(rng.integers(0, 64, n_head, dtype=np.uint8))
        for threads in (1, 4):
            assert b"".join(blocks([head, b"", np.frombuffer(body, np.uint8)], 1, threads)) == pkg.bgzf_compress(head + body, 1, 1)


def test_bgzf_threads_come_from_omp_num_threads(pkg, monkeypatch):
    import concurrent.futures as F
    seen = []

    class Pool(F.ThreadPoolExecutor):
        def __init__(self, n):
            seen.append(n)
            super().__init__(n)
    monkeypatch.setattr(F, "ThreadPoolExecutor", Pool)
    data = bytes(5 * 0xff00)
    monkeypatch.setenv("OMP_NUM_THREADS", "3")
    monkeypatch.setattr(os, "cpu_count", lambda: 512)
    pkg.bgzf_compress(data)
    monkeypatch.delenv("OMP_NUM_THREADS")
    pkg.bgzf_compress(data)
    assert seen == [3, 4]                                            # never the machine's CPU count alone


# ------------------------------------------------------------------ the C layer
def test_bam_records_symbols_exported(pkg):
    lib = pkg._native.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "genie_smem.h")).read()
    for name, nargs, res in (("genie_bam_records", 31, C.c_int), ("genie_bam_records_workspace_bytes", 2, C.c_int64)):
        assert name in pkg._native.SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is res and len(fn.argtypes) == nargs
        assert name + "(" in header
    assert lib.genie_abi_version() == 2 and pkg._native.ABI_VERSION == 2      # an addition: the version stays
    assert lib.genie_bam_records.argtypes == lib.genie_sam_text.argtypes
    for words in ("{records, bytes, unmapped records}", "NULL is the sizing call", "a record starts at any byte alignment",
                  "No atomic decides a value", "`CG`, `B`, `I`", "gives 4680", "every byte 0xFF with d_quals == NULL"):
        assert words in header, words
    for fn in (pkg.GenieIndex.bam_records, pkg.SMEM.bam_records, pkg.SMEM.write_bam, pkg.bam_header, pkg.bgzf_compress):
        assert callable(fn)


def test_bam_records_workspace_bytes(pkg):
    ws = pkg._native.lib().genie_bam_records_workspace_bytes
    assert ws(-2, 1) == INVALID and ws(2, -1) == INVALID
    for k, vals in enumerate(([0, 1, 2, 127, 2048, 2050, 10**6, 10**8], [0, 1, 63, 65, 10**4, 10**8])):
        seen = []
        for v in vals:
            args = [6, 9]
            args[k] = v
            seen.append(ws(*args))
            assert seen[-1] > 0 and seen[-1] % 256 == 0
        assert all(a <= b for a, b in zip(seen, seen[1:])), (k, seen)
    up = lambda v: (v + 255) & ~255      # noqa: E731
    for n, r in ((0, 0), (1, 0), (2, 7), (6, 2000), (2050, 3), (100002, 99999)):      # the header's pieces, each rounded up on its own
        recs = n + r
        scan = ((recs + 1023) // 1024 + 2) * 8 + 16
        assert ws(n, r) == 256 + up(4 * n) + up(8 * (n + 1)) + up(8 * recs) + up(4 * recs) + up(8 * (recs + 1)) + up(scan), (n, r)


def test_bam_records_argument_checks_before_device(pkg):
    lib = pkg._native.lib()
    ref = np.random.default_rng(1).integers(0, 4, 2000).astype(np.uint8)
    h = C.c_void_p(0)
    assert lib.genie_index_create(ref.ctypes.data_as(C.POINTER(C.c_uint8)), ref.size, 8, 0, C.byref(h)) == 0
    try:
        buf = np.zeros(1 << 16, np.uint8)
        al = (buf.ctypes.data + 255) & ~255
        p = C.c_void_p(al)
        at = lambda k: C.c_void_p(al + k)      # noqa: E731
        bytes_ok = lib.genie_bam_records_workspace_bytes(4, 10)
        assert 0 < bytes_ok <= (1 << 16) - 256
        order = ("ix", "ctg", "nctg", "bases", "ro", "N", "total", "quals", "so", "rec", "nrec", "sam", "info", "co", "cigar", "nops",
                 "names", "no", "nbytes", "cnames", "cno", "cbytes", "tags", "flags", "offs", "data", "cap", "tt", "wsp", "wsb")
        base = dict(ix=h, ctg=p, nctg=3, bases=p, ro=p, N=4, total=100, quals=p, so=p, rec=p, nrec=10, sam=p, info=p, co=p, cigar=p,
                    nops=50, names=p, no=p, nbytes=20, cnames=p, cno=p, cbytes=9, tags=31, flags=1, offs=p, data=p, cap=1000, tt=p, wsp=p,
                    wsb=bytes_ok)

        def call(**kw):
            return lib.genie_bam_records(*[dict(base, **kw)[k] for k in order], None)

        for name in ("ix", "ro", "so", "no", "cno", "offs"):
            assert call(**{name: None}) == INVALID, name
        for name in ("N", "total", "nrec", "nops", "nbytes", "cbytes", "cap", "wsb"):
            assert call(**{name: -1}) == INVALID, name
        assert call(N=3) == INVALID and call(N=3, sam=None) == NO_DEVICE      # an odd N in single-end mode only
        assert call(tags=32) == INVALID and call(tags=-1) == INVALID and call(flags=2) == INVALID and call(flags=-1) == INVALID
        for name in ("bases", "names", "cnames", "cigar", "rec", "info", "co"):
            assert call(**{name: None}) == INVALID, name
        for name in ("rec", "sam", "info"):                             # 16-byte aligned
            assert call(**{name: at(8)}) == INVALID, name
        for name in ("ro", "so", "co", "no", "cno", "offs", "tt"):      # 8-byte aligned
            assert call(**{name: at(4)}) == INVALID, name
        assert call(cigar=at(2)) == INVALID
        assert call(data=at(1)) == NO_DEVICE and call(data=at(3), cap=7) == NO_DEVICE      # the data start at any byte
        assert call(ctg=None) == INVALID and call(ctg=at(4)) == INVALID and call(nctg=0) == INVALID and call(nctg=-1) == INVALID
        assert call(nctg=2**31) == TOO_LONG and call(N=2**31) == TOO_LONG and call(nrec=2**31) == TOO_LONG
        assert call(N=2**31, wsp=None) == TOO_LONG and call(N=2**31, tags=32) == INVALID
        assert call(wsp=None) == CAPACITY and call(wsp=at(16)) == CAPACITY
        assert call(wsb=bytes_ok - 1) == CAPACITY and call(wsb=0) == CAPACITY and call(N=10**4) == CAPACITY
        assert call(tags=32, wsp=None) == INVALID
        assert call() == NO_DEVICE
        assert call(ctg=None, nctg=0) == NO_DEVICE and call(quals=None) == NO_DEVICE and call(sam=None) == NO_DEVICE
        assert call(data=None, cap=0) == NO_DEVICE and call(tt=None) == NO_DEVICE and call(tags=0, flags=0) == NO_DEVICE
        assert call(total=0, bases=None, nbytes=0, names=None, cbytes=0, cnames=None, nops=0, cigar=None) == NO_DEVICE
        assert call(nrec=0, rec=None, info=None, co=None, sam=None) == NO_DEVICE
        assert call(N=0, wsp=None, wsb=0) == NO_DEVICE
    finally:
        lib.genie_index_destroy(h)


def test_python_layer_refuses_without_a_device(pkg):
    ref = np.random.default_rng(2).integers(0, 4, 3000).astype(np.uint8)
    ix = pkg.GenieIndex.build(ref, 8)                               # host-only: no device was touched
    with pytest.raises(RuntimeError, match="index is not on a GPU"):
        ix.bam_records(np.zeros(0, np.uint8), np.zeros(1, np.int64), np.zeros(1, np.int64), np.zeros((0, 12), np.int32), None,
                       np.zeros((0, 8), np.int32), np.zeros(1, np.int64), np.zeros(0, np.int32), *pkg.names_csr([]), *pkg.names_csr(["ref"]))
