"""CPU-only tests of genie_reads_from_fasta (FASTA text -> base codes, offsets and record starts on the device): the
symbols, the argument checks of the C ABI (all before any HIP call, so they hold on a machine without a GPU), the scratch
size function, the host helper record_names, and the Python restatement of the specification (tests/fasta_util.py) on the
properties the GPU tests rely on."""
import ctypes as C
import os

import numpy as np
import pytest

import fasta_util as FU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    import genie_smem_amd as g
    g._native.build()
    return g


def test_fasta_symbols_declared_and_listed(pkg):
    lib = pkg._native.lib()
    header = open(os.path.join(ROOT, "include", "genie_smem.h")).read()
    for name in ("genie_reads_from_fasta", "genie_reads_from_fasta_tmp_bytes"):
        assert name in pkg._native.SYMBOLS
        getattr(lib, name)
        assert name + "(" in header
    assert lib.genie_abi_version() == 2                             # the change is additive


def test_fasta_argument_checks_need_no_gpu(pkg):
    lib = pkg._native.lib()
    buf = np.zeros(1 << 16, np.uint8)
    al = (buf.ctypes.data + 255) & ~255                              # a 256-byte aligned host address: never dereferenced
    table = FU.ACGT4
    need = FU.tmp_bytes(lib, 100, 10)
    assert 0 < need <= (1 << 16) - 256

    def call(text=al, nbytes=100, flags=0, tab=table.ctypes.data, bases=al + 1, cap_bases=100, offs=al + 8, starts=al + 24,
             cap_reads=10, out5=True, tmp=al, tmp_len=need):
        o5 = (C.c_int64 * 5)()
        return lib.genie_reads_from_fasta(C.c_void_p(text), nbytes, flags, C.c_void_p(tab), C.c_void_p(bases), cap_bases,
                                          C.c_void_p(offs), C.c_void_p(starts), cap_reads, o5 if out5 else None, C.c_void_p(tmp),
                                          tmp_len, None)

    assert call(text=0) == FU.E_INVALID                             # null text with text_bytes > 0
    assert call(tab=0) == FU.E_INVALID
    assert call(out5=False) == FU.E_INVALID
    assert call(nbytes=-1) == FU.E_INVALID
    assert call(cap_bases=-1) == FU.E_INVALID
    assert call(cap_reads=-1) == FU.E_INVALID
    assert call(tmp_len=-1) == FU.E_INVALID
    for flags in (2, 4, 3, -1, 1 << 20):
        assert call(flags=flags) == FU.E_INVALID
    assert call(bases=0) == FU.E_INVALID                            # exactly one of the two outputs null
    assert call(offs=0) == FU.E_INVALID
    assert call(bases=0, offs=0) == FU.E_INVALID                    # the sizing call takes no record starts
    for off in (1, 2, 4, 7):
        assert call(offs=al + 8 + off) == FU.E_INVALID              # d_read_offsets 8-byte aligned
        assert call(starts=al + 24 + off) == FU.E_INVALID           # d_record_starts too
    assert call(tmp=0) == FU.E_CAPACITY
    assert call(tmp=0, starts=0) == FU.E_CAPACITY                   # d_record_starts may be null
    assert call(tmp=0, bases=0, offs=0, starts=0) == FU.E_CAPACITY  # the sizing call's arguments are fine
    for off in (1, 16, 128):
        assert call(tmp=al + off) == FU.E_CAPACITY                  # d_tmp 256-byte aligned
    assert call(tmp_len=need - 1) == FU.E_CAPACITY
    assert call(tmp=0, flags=2) == FU.E_INVALID                     # a bad argument is reported before the scratch


def test_fasta_tmp_bytes(pkg):
    lib = pkg._native.lib()
    f = lib.genie_reads_from_fasta_tmp_bytes
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


def test_fasta_on_the_cpu_is_an_error(pkg):
    with pytest.raises(RuntimeError):
        pkg.text_reads.reads_from_text(b">a\nACGT\n", fmt="fasta", device="cpu")


def test_record_names(pkg):
    text = b">chr1 Homo sapiens\nACGT\n>chr2\tx\r\nAC\r\n>\n>r3\r\n>last"
    want = FU.parse(text)
    assert want[0] == FU.OK and want[1][0] == 5
    names = pkg.text_reads.record_names(text, want[4])
    assert names == [b"chr1", b"chr2", b"", b"r3", b"last"] == FU.names_of(text, want[4])
    assert pkg.text_reads.record_names(bytearray(text), want[4].tolist()) == names
    assert pkg.text_reads.record_names(np.frombuffer(text, np.uint8), want[4]) == names
    assert pkg.text_reads.record_names(text, []) == []
    for at in (1, len(text), -1):
        with pytest.raises(ValueError):
            pkg.text_reads.record_names(text, [at])


# ------------------------------------------------------------------ the Python restatement itself
def test_model_on_the_specification_examples():
    P = FU.PARTIAL
    assert FU.parse(b"")[:2] == (FU.OK, [0, 0, 0, 0, -1])
    assert FU.parse(b"\n\n")[:2] == (FU.OK, [0, 0, 0, 2, -1])
    assert FU.parse(b"\r\n\n", P)[:2] == (FU.OK, [0, 0, 0, 0, -1])
    assert FU.parse(b">")[:2] == (FU.OK, [1, 0, 0, 1, -1])
    assert FU.parse(b">", P)[:2] == (FU.OK, [0, 0, 0, 0, -1])      # the tail is not a line
    assert FU.parse(b">\n", P)[:2] == (FU.OK, [0, 0, 0, 0, -1])    # one header: its record may go on
    st, o5, offs, bases, starts = FU.parse(b"\n>a x\nAC\r\nG>T\n\n;N\n>b\n>c\nT")
    assert st == FU.OK and o5 == [3, 8, 7, 25, -1]
    assert offs.tolist() == [0, 7, 7, 8] and starts.tolist() == [1, 18, 21]
    assert bases.tolist() == [0, 1, 2, 4, 3, 4, 4, 3]               # '>' inside a line, ';' and 'N' are code 4
    st, o5, offs, bases, starts = FU.parse(b"\n>a x\nAC\r\nG>T\n\n;N\n>b\n>c\nT", P)
    assert st == FU.OK and o5 == [2, 7, 7, 21, -1] and offs.tolist() == [0, 7, 7] and starts.tolist() == [1, 18]
    assert FU.parse(b">a\nAC\r")[3].tolist() == [0, 1, 4]           # no '\r' is dropped from the tail
    assert FU.parse(b">a\nA\rC\r\r\n")[3].tolist() == [0, 4, 1, 4]  # a lone '\r' is a byte like any other
    # malformed: a non-empty line in front of the first header, the tail included unless the text is partial
    assert FU.parse(b"AC\n>a\nAC\n")[:2] == (FU.E_INVALID, [1, 2, 2, 9, 0])
    assert FU.parse(b"AC\n>a\nAC\n>b\n", P)[:2] == (FU.E_INVALID, [1, 2, 2, 9, 0])
    assert FU.parse(b"AC")[:2] == (FU.E_INVALID, [0, 0, 0, 2, 0])
    assert FU.parse(b"AC", P)[:2] == (FU.OK, [0, 0, 0, 0, -1])
    assert FU.parse(b"AC\n", P)[:2] == (FU.E_INVALID, [0, 0, 0, 0, 0])
    assert FU.parse(b"\n\r\n\n>a\nAC")[:2] == (FU.OK, [1, 2, 2, 9, -1])     # leading empty lines are fine
    assert FU.parse(b" >a\nAC\n")[0] == FU.E_INVALID                # a header's '>' is the first byte of its line


def _resume_texts():
    return (b">r0 first\nACGT\nAC\n>r1\n>r2\r\nGG\r\nN\r\n\r\n>r3\nA>C\n\n\nT\n>r4\nACGTA",      # no newline at the end
            b"\n\r\n>a\n\n\n>b\nAC\r\r\nG\n>\n>c\r\nT\r",           # leading empty lines, empty records, a '\r' at the end
            b">only\n" + b"ACGTACGTAC\n" * 5,
            b">x\n>y\n>z\n")


def test_model_resumes_at_every_prefix():
    for text in _resume_texts():
        whole = FU.parse(text)
        assert whole[0] == FU.OK
        for p in range(len(text) + 1):
            st, o5, offs, bases, starts = FU.parse(text[:p], FU.PARTIAL)
            assert st == FU.OK and o5[3] <= p, p
            st2, _, offs2, bases2, starts2 = FU.parse(text[o5[3]:])
            assert st2 == FU.OK, p
            assert FU.reads_of(offs, bases) + FU.reads_of(offs2, bases2) == FU.reads_of(whole[2], whole[3]), p
            assert starts.tolist() + (starts2 + o5[3]).tolist() == whole[4].tolist(), p
