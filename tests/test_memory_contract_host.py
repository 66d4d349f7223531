"""CPU-only part of the memory-contract tests: the detector of tests/guarded.py detects (a byte written into a front guard,
into a back guard, a byte changed in a frozen input; a clean run passes; every buffer has the alignment and misalignment
asked for and exactly the bytes asked for), and the workspace size functions keep what include/genie_smem.h says of them."""
import itertools

import numpy as np
import pytest
import torch

import guarded
from guarded import GUARD, POISONS, Arena

SHAPES = [("ws", 1000, 256), ("rows", 48, 16), ("rows6", 6 * 7, 2), ("lens", 4 * 5, 4), ("offs", 8 * 6, 8), ("reads", 151 * 3, 1),
          ("none", 0, 16), ("one", 1, 1), ("tmp", 257, 256)]


def _arena(poison):
    a = Arena("cpu", poison, capacity=1 << 20)
    return a, {name: a.alloc(name, nbytes, align) for name, nbytes, align in SHAPES}


def test_conditions():
    assert GUARD >= 4096 and POISONS == (0x00, 0xFF, 0x5A)


@pytest.mark.parametrize("poison", POISONS)
def test_clean_run_passes(poison):
    a, bufs = _arena(poison)
    frozen = a.freeze(torch.arange(100, dtype=torch.int64))
    inside = a.freeze(a.put("codes", np.arange(77, dtype=np.uint8)))
    for t in bufs.values():
        assert a.holds_poison(t)
        t.fill_(poison ^ 0x33)                        # writing the whole of every buffer is allowed
    a.check()
    a.check_frozen()
    assert frozen[5] == 5 and inside[76] == 76


@pytest.mark.parametrize("poison", POISONS)
def test_sizes_alignment_and_guards(poison):
    a, bufs = _arena(poison)
    last_end = 0
    for (name, nbytes, align), (bname, g0, start, end, g1) in zip(SHAPES, a.bufs):
        t = bufs[name]
        assert bname == name and t.numel() == nbytes == end - start          # exactly the bytes asked for
        assert t.data_ptr() == a.base + start or nbytes == 0
        addr = a.base + start
        assert addr % align == 0 and addr % (2 * align) == align, (name, addr)   # the weakest address of that alignment
        assert start - g0 >= GUARD and g1 - end >= GUARD and g0 >= last_end
        last_end = g1
    # an explicit misalignment, the aligned one included
    for align, mis in ((256, 0), (256, 256), (16, 0), (8, 8), (1, 0), (1, 1)):
        t = a.alloc("m", 5, align, mis)
        assert t.data_ptr() % (2 * align) == mis


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("name", [s[0] for s in SHAPES])
def test_one_byte_before_a_buffer_is_reported(poison, name):
    a, bufs = _arena(poison)
    _, g0, start, end, g1 = next(b for b in a.bufs if b[0] == name)
    a.mem[start - 1] = poison ^ 1
    with pytest.raises(AssertionError, match=f"front guard of buffer '{name}'.*1 bytes before its start"):
        a.check()


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("name", [s[0] for s in SHAPES])
def test_one_byte_past_a_buffer_is_reported(poison, name):
    a, bufs = _arena(poison)
    _, g0, start, end, g1 = next(b for b in a.bufs if b[0] == name)
    a.mem[end] = poison ^ 0x80
    with pytest.raises(AssertionError, match=f"back guard of buffer '{name}'.*0 bytes past its end"):
        a.check()


@pytest.mark.parametrize("where", ["first", "last"])
def test_far_ends_of_the_guards_are_watched(where):
    a, bufs = _arena(0x5A)
    _, g0, start, end, g1 = a.bufs[3]
    a.mem[g0 if where == "first" else g1 - 1] = 0
    with pytest.raises(AssertionError, match="guard of buffer 'lens'"):
        a.check()


def test_changed_frozen_input_is_reported():
    a, bufs = _arena(0xFF)
    outside = a.freeze(torch.zeros(1000, dtype=torch.int32), "image")
    inside = a.freeze(a.put("reads2", np.zeros(333, np.uint8)), "reads2")
    a.check_frozen()
    outside[999] = 1
    with pytest.raises(AssertionError, match="read-only tensor 'image'"):
        a.check_frozen()
    outside[999] = 0
    a.check_frozen()
    inside[0] = 1
    with pytest.raises(AssertionError, match="read-only tensor 'reads2'"):
        a.check_frozen()
    a.check()                                         # the buffer's own bytes are not guard bytes


def test_put_and_as_numpy_round_trip():
    a = Arena("cpu", 0x5A, capacity=1 << 16)
    src = np.arange(-5, 6, dtype=np.int64)
    t = a.put("x", src, align=8)
    assert t.numel() == src.nbytes and t.data_ptr() % 16 == 8
    assert np.array_equal(guarded.as_numpy(t, np.int64), src)
    with pytest.raises(MemoryError):
        a.alloc("big", 1 << 16)


# ------------------------------------------------------------------ the size functions
@pytest.fixture(scope="module")
def lib():
    import genie_smem_amd as g
    g._native.build()
    return g._native.lib()


NS = [0, 1, 2, 15, 16, 17, 255, 256, 1000, 4097, 10**6]
MAX_LENS = [0, 1, 15, 16, 100, 150, 151, 255, 256, 257, 1000, 2048, 8191, 8192]
TOTALS = [0, 1, 31, 32, 33, 10**4, 123457, 10**8]
LONG_MAX = [0, 1, 150, 8192, 8193, 10**6]


def test_short_read_sizes_are_multiples_of_256(lib):
    for n, m in itertools.product(NS, MAX_LENS):
        for fn in (lib.genie_find_smems_workspace_bytes, lib.genie_find_smems_both_workspace_bytes,
                   lib.genie_find_smems_split_workspace_bytes):
            v = fn(n, m)
            assert v > 0 and v % 256 == 0, (fn.__name__, n, m, v)
    for s in NS:
        v = lib.genie_locate_tmp_bytes(s)
        assert v > 0 and v % 256 == 0, (s, v)


def test_long_read_sizes_are_multiples_of_256(lib):
    for n, t, m in itertools.product(NS, TOTALS, LONG_MAX):
        v = lib.genie_find_smems_long_workspace_bytes(n, t, m)
        assert v > 0 and v % 256 == 0, (n, t, m, v)
        for flags in range(4):
            v = lib.genie_find_smems_long_ex_workspace_bytes(n, t, m, flags)
            assert v > 0 and v % 256 == 0, (n, t, m, flags, v)


def test_both_strands_workspace_holds_the_interleaved_batch(lib):
    """include/genie_smem.h: genie_find_smems_both_workspace_bytes(N, L) is at least genie_find_smems_workspace_bytes(2N, L)."""
    for n, m in itertools.product(NS, MAX_LENS):
        assert lib.genie_find_smems_both_workspace_bytes(n, m) >= lib.genie_find_smems_workspace_bytes(2 * n, m), (n, m)


def test_long_ex_without_flags_is_long(lib):
    for n, t, m in itertools.product(NS, TOTALS, LONG_MAX):
        assert lib.genie_find_smems_long_ex_workspace_bytes(n, t, m, 0) == lib.genie_find_smems_long_workspace_bytes(n, t, m), (n, t, m)
