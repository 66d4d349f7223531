"""CPU-only tests of genie_reads_from_text (text -> base codes and offsets on the device): the symbols, the argument checks
of the C ABI (all before any HIP call, so they hold on a machine without a GPU), the scratch size function, the byte table
of the drop-in, and the Python restatement of the specification (tests/text_util.py) on the properties the GPU tests rely on."""
import ctypes as C
import os

import numpy as np
import pytest

import text_util as TU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    import genie_smem_amd as g
    g._native.build()
    return g


def test_text_symbols_declared_and_listed(pkg):
    lib = pkg._native.lib()
    header = open(os.path.join(ROOT, "include", "genie_smem.h")).read()
    for name in ("genie_reads_from_text", "genie_reads_from_text_tmp_bytes"):
        assert name in pkg._native.SYMBOLS
        getattr(lib, name)
        assert name + "(" in header
    for line in ("#define GENIE_TEXT_LINES 0", "#define GENIE_TEXT_FASTQ 1", "#define GENIE_TEXT_PARTIAL 1"):
        assert line in header
    assert (pkg._native.TEXT_LINES, pkg._native.TEXT_FASTQ, pkg._native.TEXT_PARTIAL) == (TU.LINES, TU.FASTQ, TU.PARTIAL)
    assert lib.genie_abi_version() == 2


def test_text_argument_checks_need_no_gpu(pkg):
    lib = pkg._native.lib()
    buf = np.zeros(1 << 16, np.uint8)
    al = (buf.ctypes.data + 255) & ~255                              # a 256-byte aligned host address: never dereferenced
    table = TU.ACGT4
    need = TU.tmp_bytes(lib, 100, 10)
    assert 0 < need <= (1 << 16) - 256

    def call(text=al, nbytes=100, fmt=TU.LINES, flags=0, tab=table.ctypes.data, bases=al + 1, cap_bases=100, offs=al + 8, cap_reads=10,
             out5=True, tmp=al, tmp_len=need):
        o5 = (C.c_int64 * 5)()
        return lib.genie_reads_from_text(C.c_void_p(text), nbytes, fmt, flags, C.c_void_p(tab), C.c_void_p(bases), cap_bases,
                                         C.c_void_p(offs), cap_reads, o5 if out5 else None, C.c_void_p(tmp), tmp_len, None)

    assert call(text=0) == TU.E_INVALID                             # null text with text_bytes > 0
    assert call(tab=0) == TU.E_INVALID
    assert call(out5=False) == TU.E_INVALID
    assert call(nbytes=-1) == TU.E_INVALID
    assert call(cap_bases=-1) == TU.E_INVALID
    assert call(cap_reads=-1) == TU.E_INVALID
    assert call(tmp_len=-1) == TU.E_INVALID
    for fmt in (2, -1, 7):
        assert call(fmt=fmt) == TU.E_INVALID
    for flags in (2, 4, 3, -1, 1 << 20):
        assert call(flags=flags) == TU.E_INVALID
    assert call(bases=0) == TU.E_INVALID                            # exactly one of the two outputs null
    assert call(offs=0) == TU.E_INVALID
    for off in (1, 2, 4, 7):
        assert call(offs=al + 8 + off) == TU.E_INVALID              # d_read_offsets 8-byte aligned
    assert call(tmp=0) == TU.E_CAPACITY
    for off in (1, 16, 128):
        assert call(tmp=al + off) == TU.E_CAPACITY                  # d_tmp 256-byte aligned
    assert call(tmp_len=need - 1) == TU.E_CAPACITY
    assert call(tmp=0, fmt=9) == TU.E_INVALID                       # a bad argument is reported before the scratch


def test_text_tmp_bytes(pkg):
    lib = pkg._native.lib()
    f = lib.genie_reads_from_text_tmp_bytes
    assert f(-1, 0) < 0 and f(0, -1) < 0 and f(-5, -5) < 0
    ts = [0, 1, 15, 16, 4095, 4096, 4097, 10**6, 2**31 - 1, 2**31, 2**33 + 5]
    ns = [0, 1, 1023, 1024, 1025, 10**6, 2**31, 2**40]
    grid = [[f(t, n) for n in ns] for t in ts]
    for i in range(len(ts)):
        for j in range(len(ns)):
            assert grid[i][j] > 0 and grid[i][j] % 256 == 0
            if i:
                assert grid[i][j] >= grid[i - 1][j], (i, j)
            if j:
                assert grid[i][j] >= grid[i][j - 1], (i, j)
    assert f(10**9, 10**9) < 0.02 * 10**9                           # a small fraction of the text


def test_byte_codes_equal_encode_lenient(pkg):
    rng = np.random.default_rng(7)
    every = bytes(range(256)).decode("latin-1")
    for ref in ("ACGTTGCAACGGT", "ACGACGGGCA", "CATTACCAT", "XYZZYXXZ"):      # four letters, three of ACGT, three of its own
        m = pkg.ExactMatch("text_codes.fa")
        m.set_reference(ref)
        table = m.byte_codes()
        assert table.dtype == np.uint8 and table.shape == (256,) and table.max() == 4
        assert (table[np.frombuffer(b"\n\rNn@+", np.uint8)] == 4).all()
        strings = [every, "", "ACGTNacgtn", ref, ref.lower()] + \
            ["".join(chr(int(c)) for c in rng.integers(0, 256, 300)) for _ in range(5)]
        for s in strings:
            want = m.encode_lenient(s)
            got = table[np.frombuffer(s.encode("latin-1"), np.uint8)]
            assert np.array_equal(got, want), (ref, s[:20])
        folded = m.byte_codes(fold_case=True)
        for ch in range(ord("A"), ord("Z") + 1):
            assert folded[ch] == table[ch]
            assert folded[ch + 32] == table[ch], chr(ch)
        rest = [b for b in range(256) if not ord("a") <= b <= ord("z")]
        assert np.array_equal(folded[rest], table[rest])


# ------------------------------------------------------------------ the Python restatement itself
def test_model_on_the_specification_examples():
    P = TU.PARTIAL
    assert TU.parse(b"", TU.LINES)[1] == [0, 0, 0, 0, -1]
    assert TU.parse(b"\n\n", TU.LINES)[1] == [2, 0, 0, 2, -1]
    assert TU.parse(b"A", TU.LINES)[1] == [1, 1, 1, 1, -1]
    assert TU.parse(b"A", TU.LINES, P)[1] == [0, 0, 0, 0, -1]
    st, o5, offs, bases = TU.parse(b"AC\nGT", TU.LINES)
    assert (o5, offs.tolist(), bases.tolist()) == ([2, 4, 2, 5, -1], [0, 2, 4], [0, 1, 2, 3])
    st, o5, offs, bases = TU.parse(b"AC\nGT", TU.LINES, P)
    assert (o5, offs.tolist(), bases.tolist()) == ([1, 2, 2, 3, -1], [0, 2], [0, 1])
    assert TU.parse(b"AC\r\n\r\nG\r", TU.LINES)[2].tolist() == [0, 2, 2, 4]      # no '\r' is dropped from the tail
    st, o5, offs, bases = TU.parse(TU.MIXED_FASTQ, TU.FASTQ)
    assert st == TU.OK and o5[0] == 4 and offs.tolist() == [0, 5, 9, 9, 18]
    assert bases.tolist() == [0, 1, 2, 3, 4, 4, 4, 4, 3, 2, 2, 4, 4, 0, 1, 4, 4, 3]
    five = b"@a\nAC\n+\nII\n@b\n"
    assert TU.parse(five, TU.FASTQ)[:2] == (TU.E_INVALID, [1, 2, 2, len(five), 1])
    assert TU.parse(five, TU.FASTQ, P)[:2] == (TU.OK, [1, 2, 2, 11, -1])


def _resume_texts():
    fq = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate((b"ACGT", b"", b"GGN", b"T\r", b"ACGTA")))
    return (TU.FASTQ, fq), (TU.LINES, b"ACGT\n\nGG\r\nT\nNNA\nC\n")


def test_model_resumes_at_every_prefix():
    for fmt, text in _resume_texts():
        whole = TU.parse(text, fmt)
        assert whole[0] == TU.OK
        for p in range(len(text) + 1):
            st, o5, offs, bases = TU.parse(text[:p], fmt, TU.PARTIAL)
            assert st == TU.OK and o5[3] <= p
            st2, _, offs2, bases2 = TU.parse(text[o5[3]:], fmt)
            assert st2 == TU.OK
            assert TU.reads_of(offs, bases) + TU.reads_of(offs2, bases2) == TU.reads_of(whole[2], whole[3]), (fmt, p)
