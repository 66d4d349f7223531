"""CPU-only tests of the split-read feature (SMEMs of reads with ambiguous bases): the lenient encoder, the C ABI's
argument checks of genie_find_smems_split (they come before the device check, so a host-only handle reaches them), and
the host-side split reference the GPU tests compare against."""
import ctypes as C

import numpy as np
import pytest

import split_util as SU


@pytest.fixture(scope="module")
def pkg():
    import genie_smem_amd as g
    g._native.build()
    return g


def test_encode_lenient_maps_every_other_symbol_to_a_break(pkg):
    m = pkg.ExactMatch("x.fa")
    m.set_reference("ACGTTGCAACGT")
    assert m.encode_lenient("ACGT").tolist() == [0, 1, 2, 3]
    assert m.encode_lenient("ANnCRYKM-.$ t").tolist() == [0, 4, 4, 1, 4, 4, 4, 4, 4, 4, 4, 4, 4]
    everything = "".join(chr(c) for c in range(256))
    codes = m.encode_lenient(everything)
    assert codes.dtype == np.uint8 and codes.size == 256
    for c in range(256):
        assert codes[c] == ("ACGT".index(chr(c)) if chr(c) in "ACGT" else 4), c
    assert m.encode_lenient("").size == 0


def test_encode_still_raises(pkg):
    m = pkg.ExactMatch("x.fa")
    m.set_reference("ACACACCACAACCA")                       # no G, no T
    with pytest.raises(KeyError):
        m.encode("ACN")
    with pytest.raises(KeyError):
        m.encode("ACG")
    # the lenient form keeps the alphabet's code for a base the reference lacks: the device treats it as a break
    assert m.encode_lenient("ACGN").tolist() == [0, 1, 2, 4]


def test_split_symbols_exported(pkg):
    lib = pkg._native.lib()
    for name in ("genie_find_smems_split", "genie_find_smems_split_workspace_bytes"):
        assert name in pkg._native.SYMBOLS
        getattr(lib, name)


def test_split_workspace_bytes_arguments(pkg):
    lib = pkg._native.lib()
    assert lib.genie_find_smems_split_workspace_bytes(-1, 150) < 0
    assert lib.genie_find_smems_split_workspace_bytes(10, -1) < 0
    assert lib.genie_find_smems_split_workspace_bytes(10, pkg._native.MAX_READ_LEN + 1) < 0
    w0 = lib.genie_find_smems_split_workspace_bytes(0, 150)
    w1 = lib.genie_find_smems_split_workspace_bytes(1000, 150)
    w2 = lib.genie_find_smems_split_workspace_bytes(1000, 8192)
    assert 0 < w0 < w1 < w2
    # at least the find_smems workspace of the same batch (the no-break path runs it unchanged)
    assert w1 >= lib.genie_find_smems_workspace_bytes(1000, 150)


def test_split_argument_checks(pkg):
    lib = pkg._native.lib()
    ix = pkg.GenieIndex.build(np.asarray([0, 1, 2, 3] * 64, np.uint8), 4)        # host arrays only, no device image
    p = C.c_void_p(1 << 20)                                                       # never dereferenced: checks fail first
    ws = lib.genie_find_smems_split_workspace_bytes(10, 150)
    f = lib.genie_find_smems_split

    def call(h=ix._h, reads=p, lens=None, n=10, stride=150, fixed=150, offsets=p, rows=p, cap=100, status=None, wsp=p,
             wsb=ws):
        return f(h, reads, lens, n, stride, fixed, 1, offsets, rows, cap, status, wsp, wsb, None)

    assert call(h=None) == -1                          # GENIE_E_INVALID
    assert call(n=-1) == -1
    assert call(offsets=None) == -1
    assert call(reads=None) == -1
    assert call(rows=None) == -1
    assert call(wsp=None) == -1
    assert call(cap=-1) == -1
    assert call(stride=100) == -1                      # stride shorter than the reads
    assert call(rows=C.c_void_p((1 << 20) + 4)) == -1  # rows must be 16-byte aligned
    assert call(wsp=C.c_void_p((1 << 20) + 16)) == -1  # workspace must be 256-byte aligned
    assert call(fixed=pkg._native.MAX_READ_LEN + 1, stride=pkg._native.MAX_READ_LEN + 1) == -6   # GENIE_E_TOO_LONG
    assert call(wsb=ws - 1) == -10                     # GENIE_E_CAPACITY
    assert call() == -4                                # every argument fine: GENIE_E_NO_DEVICE on a host-only handle
    assert call(n=0, reads=None, rows=None, wsp=None, wsb=0) == -4


def test_segments_reference():
    assert SU.segments(np.asarray([], np.uint8)) == []
    assert SU.segments(np.asarray([4, 4, 255], np.uint8)) == []
    assert SU.segments(np.asarray([0, 1, 4, 2, 3, 3, 9], np.uint8)) == [(0, 2), (3, 3)]
    assert SU.segments(np.asarray([4, 0, 1, 2, 3], np.uint8)) == [(1, 4)]
    # a base the reference lacks (here G = 2) is a break too
    assert SU.segments(np.asarray([0, 2, 1, 1, 2], np.uint8), present=0b1011) == [(0, 1), (2, 2)]
    assert SU.present_mask([0, 1, 3, 3]) == 0b1011


def test_split_reference_equals_oracle_without_breaks(oracle_mod):
    from genie_smem_amd import synth
    ref = synth.synth_ref(20_000, 7)
    o = oracle_mod.Oracle(ref, 8)
    reads = np.concatenate([synth.reads_from_ref(ref, 20, 120, 3), synth.reads_random(20, 120, 4)])
    for min_len in (1, 19):
        for r in reads:
            rc, want = o.find_smems("bwa", r, min_len)
            assert rc >= 0
            assert SU.split_rows(o, r, min_len).tolist() == want.tolist()


def test_split_reference_cuts_at_breaks(oracle_mod):
    from genie_smem_amd import synth
    ref = synth.synth_ref(20_000, 8)
    o = oracle_mod.Oracle(ref, 8)
    a, b = synth.reads_from_ref(ref, 2, 60, 5)
    read = np.concatenate([a, [4], b])
    _, ra = o.find_smems("bwa", a)
    _, rb = o.find_smems("bwa", b)
    rb = rb.copy()
    rb[:, :2] += 61
    assert SU.split_rows(o, read).tolist() == ra.tolist() + rb.tolist()
