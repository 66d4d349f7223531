"""CPU-only tests of genie_sam_text (SAM text on the device, with the MD, MC and MQ tags): the brute force of
tests/sam_text_util.py against sam_lines on the fixture of tests/test_pair_host.py's kind and on random batches, which ties the
new definition to the existing one; hand-written MD cases; text_reads.fastq_fields and names_csr on CPU tensors; the symbols and
the header's wording; the workspace function's formula; and the C ABI's argument checks in their documented order (before the
device check, so a host-only handle reaches them)."""
import ctypes as C
import os

import numpy as np
import pytest

import sam_text_util as ST

INVALID, NO_DEVICE, CAPACITY, TOO_LONG = ST.INVALID, ST.NO_DEVICE, ST.CAPACITY, ST.TOO_LONG
TABLE = np.asarray([0, 6000, 11000, 16384], np.int64)


@pytest.fixture(scope="module")
def pkg():
    import genie_smem_amd as g
    g._native.build()
    return g


def _as_lines(b, pkg, seq=True):
    text = lambda raw: [bytes(x).decode("latin-1") for x in raw]      # noqa: E731
    ro = b["read_offsets"]
    seqs = [ST.seq_text(b["bases"][ro[r]:ro[r + 1]], False) for r in range(ro.size - 1)] if seq else None
    quals = [bytes(b["quals"][ro[r]:ro[r + 1]]).decode("latin-1") for r in range(ro.size - 1)] if seq and b["quals"] is not None else None
    return pkg.sam_lines(b["records"], b["sam"], b["info"], b["cigar_offsets"], b["cigar"], text(b["names"]), text(b["contig_names"]),
                         seqs, quals)


# ------------------------------------------------------------------ the brute force is sam_lines
def test_brute_force_equals_sam_lines_on_the_pinned_fixture(pkg):
    ops = lambda *v: [ST.op(n, o) for n, o in v]      # noqa: E731
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
    want = ST.expected(b, T)
    lines = bytes(want["text"]).decode().split("\n")
    assert lines[-1] == "" and lines[:-1] == _as_lines(b, pkg)
    assert lines[0] == "p0\t99\tchrA\t101\t6\t50=\t=\t301\t252\tACGTA\tIIIIH\tNM:i:1\tAS:i:48"
    assert lines[2].split("\t")[9:11] == ["CGGTT", "EDCBA"] and lines[4] == "p1\t165\tchrB\t41\t0\t*\t=\t41\t0\tGGGGA\t#####"
    assert want["totals"].tolist() == [5, len(want["text"]), 1] and want["line_offsets"][-1] == len(want["text"])
    bare = ST.expected(dict(b, quals=None), T, flags=ST.NO_SEQ)
    assert bytes(bare["text"]).decode().split("\n")[:-1] == _as_lines(b, pkg, seq=False)
    # every tag: MD from the reference, MC and MQ from the mate's chosen record, also on the unmapped line
    full = bytes(ST.expected(b, T, 31)["text"]).decode().split("\n")
    md = "20^" + "".join("ACGT"[c] for c in T[320:322]) + "30"
    assert full[2].split("\t")[11:] == ["NM:i:2", "AS:i:50", "MD:Z:" + md, "MC:Z:50=", "MQ:i:6"]
    assert full[0].split("\t")[13:] == ["MD:Z:50", "MC:Z:3S20=2D30=", "MQ:i:60"]
    assert full[3].split("\t")[11:] == ["NM:i:0", "AS:i:50", "MD:Z:50"] and full[4].split("\t")[11:] == ["MC:Z:50=", "MQ:i:60"]
    single = bytes(ST.expected(dict(b, sam=None), T, 31)["text"]).decode().split("\n")
    assert single[1].split("\t")[:9] == ["p0", "256", "chrB", "11", "0", "50=", "*", "0", "0"] and "MC:Z" not in "".join(single)
    assert single[2].split("\t")[1] == "16" and single[4] == "p1\t4\t*\t0\t0\t*\t*\t0\t0\tGGGGA\t#####"


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_brute_force_equals_sam_lines_on_random_batches(pkg, seed):
    rng = np.random.default_rng(100 + seed)
    counts = rng.integers(0, 4, 40).tolist() + [0, 0, 3, 0]
    b = ST.make_batch(rng, ST.random_reads(rng, counts, TABLE), contig_offsets=TABLE, quals=seed != 1)
    T = rng.integers(0, 4, int(TABLE[-1])).astype(np.uint8)
    want = ST.expected(b, T)
    assert bytes(want["text"]).decode("latin-1") == "\n".join(_as_lines(b, pkg)) + "\n"
    assert want["totals"][2] == counts.count(0) and want["totals"][0] == sum(counts) + counts.count(0)


# ------------------------------------------------------------------ MD by hand
def test_md_by_hand():
    T = np.asarray([0, 1, 2, 3] * 8, np.uint8)                       # ACGTACGT...
    md = lambda t, *v: ST.md_text([ST.op(n, o) for n, o in v], T, t)      # noqa: E731
    EQ, X, D, I, S = ST.EQ, ST.X, ST.D, ST.I, ST.S
    assert md(0, (5, EQ), (1, X), (1, X), (3, EQ)) == "5C0G3"        # adjacent X
    assert md(0, (5, EQ), (2, X), (3, EQ)) == "5C0G3"                # the same as one op
    assert md(0, (1, X), (7, EQ)) == "0A7"                           # X first
    assert md(4, (7, EQ), (1, X)) == "7T0"                           # X last
    assert md(0, (4, EQ), (2, D), (1, X), (2, EQ)) == "4^AC0G2"      # D then X
    assert md(0, (3, S), (4, EQ), (2, I), (5, EQ), (6, S)) == "9"    # I between = runs, clips: nothing
    assert md(3, (2, S), (1, EQ), (3, I), (1, D), (2, EQ)) == "1^A2"
    assert md(0) == "0" and md(0, (4, S)) == "0"
    assert md(0, (0, D)) == "0^0" and md(0, (3, EQ), (0, X), (2, EQ)) == "5"      # the definition, taken literally
    assert md(30, (4, X)) == "0G0T0T0T0" and md(-2, (3, D)) == "0^AAA0"            # positions outside [0, n) are clamped
    assert md(0, (2**28 - 1, EQ), (1, X), (2**28 - 1, EQ)) == f"{2**28 - 1}T{2**28 - 1}"
    assert ST.cigar_text([ST.op(3, S), ST.op(20, EQ), ST.op(1, X), ST.op(2, D), ST.op(5, I)]) == "3S20=1X2D5I" and ST.cigar_text([]) == ""


# ------------------------------------------------------------------ text helpers on CPU tensors
def test_names_csr(pkg):
    import torch
    data, off = pkg.names_csr(["chr1", b"x", "", "scaffold_22"])
    assert data.dtype == torch.uint8 and off.dtype == torch.int64 and bytes(data.numpy()) == b"chr1xscaffold_22"
    assert off.tolist() == [0, 4, 5, 5, 16]
    data, off = pkg.names_csr([])
    assert data.numel() == 0 and off.tolist() == [0]
    assert pkg.names_csr(["é"])[1].tolist() == [0, 2]


def test_fastq_fields_on_cpu_tensors(pkg):
    import torch
    F = pkg.text_reads.fastq_fields
    text = b"@r1 first read\r\nACGT\r\n+\r\n@II!\r\n@r2\tx\nAC\n+r2\nI+\n@r/3\n\n+\n\n@last\rz\nACGTA\n+\n@@@@@"      # a tail without '\n'
    ro = torch.tensor([0, 4, 6, 6, 11])
    names, no, quals = F(text, ro)
    assert names.dtype == torch.uint8 and no.dtype == torch.int64 and quals.dtype == torch.uint8
    assert bytes(names.numpy()) == b"r1r2r/3last" and no.tolist() == [0, 2, 4, 7, 11]
    assert bytes(quals.numpy()) == b"@II!I+@@@@@"                   # a quality line may start with '@'
    again = F(np.frombuffer(text + b"\n", np.uint8), ro.numpy())      # the same with the last line closed; numpy inputs
    assert all(torch.equal(x, y) for x, y in zip(again, (names, no, quals)))
    first = F(text, ro[:3])                                          # fewer reads than records: the first ones
    assert bytes(first[0].numpy()) == b"r1r2" and bytes(first[2].numpy()) == b"@II!I+"
    with pytest.raises(ValueError):
        F(text, torch.tensor([0, 4, 6, 6, 10]))                      # the last quality line is one byte longer than its read
    with pytest.raises(ValueError):
        F(text, torch.tensor([0, 4, 5, 5, 10]))
    with pytest.raises(ValueError):
        F(text, torch.tensor([0, 4, 6, 6, 11, 11]))                  # more reads than records
    empty = F(b"", torch.tensor([0]))
    assert empty[0].numel() == 0 and empty[1].tolist() == [0] and empty[2].numel() == 0
    only = F(b"@\n\n+\n", torch.tensor([0, 0]))                       # an empty name, an empty read, an empty tail as quality line
    assert only[0].numel() == 0 and only[1].tolist() == [0, 0] and only[2].numel() == 0
    # two files: the qualities are interleaved like the bases
    b1, o1, _ = (torch.tensor([0, 1, 2, 3, 0], dtype=torch.uint8), torch.tensor([0, 2, 5]), None)
    q1, q2 = torch.tensor(list(b"ABCDE"), dtype=torch.uint8), torch.tensor(list(b"xyz"), dtype=torch.uint8)
    o2 = torch.tensor([0, 3, 3])
    inter = pkg.text_reads.interleave_reads((q1, o1), (q2, o2))
    assert bytes(inter[0].numpy()) == b"ABxyzCDE" and inter[1].tolist() == [0, 2, 5, 8, 8] and b1.numel() == 5


# ------------------------------------------------------------------ the C layer
def test_sam_text_symbols_exported(pkg):
    lib = pkg._native.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "genie_smem.h")).read()
    for name, nargs, res in (("genie_sam_text", 31, C.c_int), ("genie_sam_text_workspace_bytes", 2, C.c_int64)):
        assert name in pkg._native.SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is res and len(fn.argtypes) == nargs
        assert name + "(" in header
    assert lib.genie_abi_version() == 2 and pkg._native.ABI_VERSION == 2      # an addition: the version stays
    N = pkg._native
    assert (N.SAM_NM, N.SAM_AS, N.SAM_MD, N.SAM_MC, N.SAM_MQ, N.SAM_NO_SEQ) == (ST.NM, ST.AS, ST.MD, ST.MC, ST.MQ, ST.NO_SEQ)
    for k, v in (("NM", 1), ("AS", 2), ("MD", 4), ("MC", 8), ("MQ", 16), ("NO_SEQ", 1)):
        assert f"#define GENIE_SAM_{k} {v}\n" in header
    for words in ("5A0C3, 0A7, 4^AC0T2", "No atomic decides a value", "NULL is the sizing call", "the LAST record in the range of read r ^ 1",
                  "{lines, bytes, unmapped lines}", "Single-end mode (d_sam == NULL)", "a prefix sum less a prefix maximum"):
        assert words in header, words
    assert callable(pkg.GenieIndex.sam_text) and callable(pkg.SMEM.sam_text) and callable(pkg.SMEM.write_sam)


def test_sam_text_workspace_bytes(pkg):
    ws = pkg._native.lib().genie_sam_text_workspace_bytes
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
    for n, r in ((0, 0), (1, 0), (2, 7), (6, 2000), (2050, 3), (100002, 99999)):      # every piece is rounded up to 256 on its own
        lines = n + r
        scan = ((lines + 1023) // 1024 + 2) * 8 + 16
        assert ws(n, r) == 256 + up(4 * n) + up(8 * (n + 1)) + up(8 * lines) + up(4 * lines) + up(8 * (lines + 1)) + up(scan), (n, r)
    big = 10**8
    assert 32 <= (ws(2 * big, 7) - ws(big, 7)) / big < 32.01 and 20 <= (ws(7, 2 * big) - ws(7, big)) / big < 20.01


def test_sam_text_argument_checks_before_device(pkg):
    lib = pkg._native.lib()
    ref = np.random.default_rng(1).integers(0, 4, 2000).astype(np.uint8)
    h = C.c_void_p(0)
    assert lib.genie_index_create(ref.ctypes.data_as(C.POINTER(C.c_uint8)), ref.size, 8, 0, C.byref(h)) == 0
    try:
        buf = np.zeros(1 << 16, np.uint8)
        al = (buf.ctypes.data + 255) & ~255
        p = C.c_void_p(al)
        at = lambda k: C.c_void_p(al + k)      # noqa: E731
        bytes_ok = lib.genie_sam_text_workspace_bytes(4, 10)
        assert 0 < bytes_ok <= (1 << 16) - 256
        order = ("ix", "ctg", "nctg", "bases", "ro", "N", "total", "quals", "so", "rec", "nrec", "sam", "info", "co", "cigar", "nops",
                 "names", "no", "nbytes", "cnames", "cno", "cbytes", "tags", "flags", "lo", "text", "cap", "tt", "wsp", "wsb")
        base = dict(ix=h, ctg=p, nctg=3, bases=p, ro=p, N=4, total=100, quals=p, so=p, rec=p, nrec=10, sam=p, info=p, co=p, cigar=p,
                    nops=50, names=p, no=p, nbytes=20, cnames=p, cno=p, cbytes=9, tags=31, flags=1, lo=p, text=p, cap=1000, tt=p, wsp=p,
                    wsb=bytes_ok)

        def call(**kw):
            return lib.genie_sam_text(*[dict(base, **kw)[k] for k in order], None)

        for name in ("ix", "ro", "so", "no", "cno", "lo"):
            assert call(**{name: None}) == INVALID, name
        for name in ("N", "total", "nrec", "nops", "nbytes", "cbytes", "cap", "wsb"):
            assert call(**{name: -1}) == INVALID, name
        assert call(N=3) == INVALID and call(N=3, sam=None) == NO_DEVICE      # an odd N in single-end mode only
        assert call(tags=32) == INVALID and call(tags=-1) == INVALID and call(flags=2) == INVALID and call(flags=-1) == INVALID
        for name in ("bases", "names", "cnames", "cigar", "rec", "info", "co"):
            assert call(**{name: None}) == INVALID, name
        for name in ("rec", "sam", "info"):                             # 16-byte aligned
            assert call(**{name: at(8)}) == INVALID, name
        for name in ("ro", "so", "co", "no", "cno", "lo", "tt"):        # 8-byte aligned
            assert call(**{name: at(4)}) == INVALID, name
        assert call(cigar=at(2)) == INVALID
        assert call(ctg=None) == INVALID and call(ctg=at(4)) == INVALID and call(nctg=0) == INVALID and call(nctg=-1) == INVALID
        assert call(nctg=2**31) == TOO_LONG and call(N=2**31) == TOO_LONG and call(nrec=2**31) == TOO_LONG
        assert call(N=2**31, wsp=None) == TOO_LONG and call(N=2**31, tags=32) == INVALID
        assert call(wsp=None) == CAPACITY and call(wsp=at(16)) == CAPACITY
        assert call(wsb=bytes_ok - 1) == CAPACITY and call(wsb=0) == CAPACITY and call(N=10**4) == CAPACITY
        assert call(tags=32, wsp=None) == INVALID
        assert call() == NO_DEVICE
        assert call(ctg=None, nctg=0) == NO_DEVICE and call(quals=None) == NO_DEVICE and call(sam=None) == NO_DEVICE
        assert call(text=None, cap=0) == NO_DEVICE and call(tt=None) == NO_DEVICE and call(tags=0, flags=0) == NO_DEVICE
        assert call(total=0, bases=None, nbytes=0, names=None, cbytes=0, cnames=None, nops=0, cigar=None) == NO_DEVICE
        assert call(nrec=0, rec=None, info=None, co=None, sam=None) == NO_DEVICE
        assert call(N=0, wsp=None, wsb=0) == NO_DEVICE
    finally:
        lib.genie_index_destroy(h)


def test_python_layer_refuses_without_a_device(pkg):
    ref = np.random.default_rng(2).integers(0, 4, 3000).astype(np.uint8)
    ix = pkg.GenieIndex.build(ref, 8)                               # host-only: no device was touched
    with pytest.raises(Exception):
        ix.sam_text(np.zeros(0, np.uint8), np.zeros(1, np.int64), np.zeros(1, np.int64), np.zeros((0, 12), np.int32), None,
                    np.zeros((0, 8), np.int32), np.zeros(1, np.int64), np.zeros(0, np.int32), *pkg.names_csr([]), *pkg.names_csr(["ref"]))
