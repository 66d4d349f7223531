"""GPU tests of genie_reads_from_text (run with -m gpu on an MI355X): text -> base codes back to back and int64 offsets on
the device.  Expected values come from the Python restatement of the specification in tests/text_util.py (bytes.find and a
numpy table lookup); every comparison is exact.  Through the raw C ABI unless a test says drop-in."""
import numpy as np
import pytest

import golden_util as G
import text_util as TU
from guarded import POISONS, Arena, as_numpy

pytestmark = pytest.mark.gpu

TILE = 4096                  # bytes of text per block in csrc/text_reads.inc (tiles lie on the 16-byte grid of the address)


@pytest.fixture(scope="module")
def pkg():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import genie_smem_amd as g
    g._native.lib()
    return g


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg._native.lib()


@pytest.fixture(scope="module")
def random_lines():
    """200 000 lines of 0 .. 3 symbols (some of them '\\r', 'N' or lower case)."""
    rng = np.random.default_rng(11)
    lens = rng.integers(0, 4, 200_000)
    sym = np.frombuffer(b"ACGTNa\r", np.uint8)[rng.integers(0, 7, int(lens.sum()))]
    out = np.full(int(lens.sum()) + lens.size, 0x0A, np.uint8)
    ends = np.cumsum(lens + 1) - 1                                   # where the newlines go
    keep = np.ones(out.size, bool)
    keep[ends] = False
    out[keep] = sym
    return out.tobytes()


# ------------------------------------------------------------------ 1. edge texts
EDGE_TEXTS = [b"", b"\n", b"\n\n\n", b"A", b"A\n", b"AC\nGT", b"AC\r\nGT\r\n", b"\r\n", b"AC\nGT\r", b"\r", b"\r\r\n\r",
              b"A\x00C\xffG\nT\x00\n", b"acgtN\nNNnn\nACGT", TU.MIXED_FASTQ, TU.MIXED_FASTQ[:-1], TU.MIXED_FASTQ + b"@r4\nAC",
              b"@a\nACGT\n+\nIIII", b"@a\r\nAC\r\n+\r\nII\r"]


@pytest.mark.parametrize("fmt", TU.FORMATS)
def test_edge_texts(lib, fmt):
    for text in EDGE_TEXTS:
        for flags in (0, TU.PARTIAL):
            TU.same_as_model(lib, text, fmt, flags)
    want = TU.same_as_model(lib, b"", fmt)
    assert want[1] == [0, 0, 0, 0, -1] and want[2].tolist() == [0]
    # another table: a three-letter alphabet of its own, and entries above 4 clamp to 4
    table = np.full(256, 9, np.uint8)
    table[list(b"XYZ")] = [0, 1, 2]
    table[ord("Q")] = 200
    TU.same_as_model(lib, b"@h\nXYZQAX\n+\n!!!!!!\n" if fmt == TU.FASTQ else b"XYZQ\nAXX\n\nZ", fmt, 0, table)


# ------------------------------------------------------------------ 2. boundaries
def _boundary_ks():
    return sorted(set(range(0, 301)) | {2 ** j + d - 3 for j in range(6, 17) for d in range(6)})


def test_every_tile_and_vector_boundary(lib):
    """'A' * k + "\\n" + "CG\\r\\n" + "T": the '\\n', the '\\r' and the next line's start on each side of every power-of-two
    boundary from 64 bytes to 64 KiB (the tile is 4096 bytes, the vector load 16)."""
    for k in _boundary_ks():
        text = b"A" * k + b"\nCG\r\nT"
        want = TU.same_as_model(lib, text, TU.LINES)
        assert want[1][:3] == [3, k + 3, max(k, 2)]
        TU.same_as_model(lib, text, TU.LINES, TU.PARTIAL)


def test_boundaries_with_the_text_at_an_odd_address(lib):
    """The same with the text 5 bytes behind a 16-byte boundary: the tiles follow the address, so k is 5 smaller."""
    import torch
    lead = 5
    ks = sorted({k - lead for k in _boundary_ks() if k >= 59} | set(range(0, 40)))
    buf = torch.zeros(TILE * 17 + 64, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    stream = torch.cuda.current_stream().cuda_stream
    tb = TU.tmp_bytes(lib, 1 << 17, 3)
    tmp = torch.empty(tb, dtype=torch.uint8, device="cuda")
    for k in ks:
        text = b"A" * k + b"\nCG\r\nT"
        buf[lead:lead + len(text)] = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).cuda()
        want = TU.parse(text, TU.LINES)
        offs = torch.full((5,), -77, dtype=torch.int64, device="cuda")
        bases = torch.full((k + 3 + 9,), 0xA5, dtype=torch.uint8, device="cuda")
        rc, out5 = TU.raw_call(lib, buf.data_ptr() + lead, len(text), TU.LINES, 0, TU.ACGT4, bases.data_ptr() + 1, k + 3, offs.data_ptr(),
                               3, tmp.data_ptr(), tb, stream)
        assert (rc, out5) == (TU.OK, want[1]), k
        assert offs.cpu().tolist() == want[2].tolist() + [-77]
        b = bases.cpu().numpy()
        assert b[0] == 0xA5 and np.array_equal(b[1:k + 4], want[3]) and (b[k + 4:] == 0xA5).all(), k


# ------------------------------------------------------------------ 3. extremes of density
def test_only_newlines(lib):
    want = TU.same_as_model(lib, b"\n" * 65536, TU.LINES)
    assert want[1] == [65536, 0, 0, 65536, -1]
    TU.same_as_model(lib, b"\n" * 65536, TU.LINES, TU.PARTIAL)


def test_many_tiny_lines(lib, random_lines):
    want = TU.same_as_model(lib, random_lines, TU.LINES)
    assert want[1][0] == 200_000
    TU.same_as_model(lib, random_lines[:-1], TU.LINES, TU.PARTIAL)


def test_one_very_long_line(lib):
    rng = np.random.default_rng(5)
    long_ = np.frombuffer(b"ACGTN", np.uint8)[rng.integers(0, 5, 1_000_003)].tobytes()
    want = TU.same_as_model(lib, b"ACG\n" + long_ + b"\r\nTT", TU.LINES)
    assert want[1][:3] == [3, 1_000_008, 1_000_003]
    fq = b"@a\nAC\n+\nII\n@long\n" + long_[:300_001] + b"\n+\n" + b"I" * 300_001 + b"\n@c\nG\n+\nI\n"
    want = TU.same_as_model(lib, fq, TU.FASTQ)
    assert want[1][:3] == [3, 300_004, 300_001]


# ------------------------------------------------------------------ 4. GENIE_TEXT_PARTIAL and resume
def test_partial_prefixes_resume(lib):
    from test_text_reads_host import _resume_texts
    for fmt, text in _resume_texts():
        whole = TU.parse(text, fmt)
        for p in range(len(text) + 1):
            st, o5, offs, bases = TU.device_parse(lib, text[:p], fmt, TU.PARTIAL)
            assert st == TU.OK and o5[3] <= p, (fmt, p)
            assert (st, o5) == TU.parse(text[:p], fmt, TU.PARTIAL)[:2], (fmt, p)
            st2, _, offs2, bases2 = TU.device_parse(lib, text[o5[3]:], fmt)
            assert st2 == TU.OK
            assert TU.reads_of(offs, bases) + TU.reads_of(offs2, bases2) == TU.reads_of(whole[2], whole[3]), (fmt, p)


# ------------------------------------------------------------------ 5. malformed FASTQ
def test_malformed_fastq(lib):
    rec = lambda i, h=b"@", p=b"+": h + b"r%d\nACG\n" % i + p + b"\nIII\n"
    good = [rec(i) for i in range(5)]
    both = b"".join([good[0], rec(1, p=b"-"), good[2], rec(3, h=b">"), good[4]])
    for flags in (0, TU.PARTIAL):
        st, o5, _, _ = TU.same_as_model(lib, both, TU.FASTQ, flags)
        assert st == TU.E_INVALID and o5[4] == 1 and o5[0] == 5
    st, o5, _, _ = TU.same_as_model(lib, b"".join(good[:3]) + rec(3, h=b">"), TU.FASTQ)
    assert st == TU.E_INVALID and o5[4] == 3
    st, o5, _, _ = TU.same_as_model(lib, good[0] + b"\nACG\n+\nIII\n", TU.FASTQ)          # an empty header line
    assert st == TU.E_INVALID and o5[4] == 1
    st, o5, _, _ = TU.same_as_model(lib, good[0] + b"@r\nACG\n\nIII\n", TU.FASTQ)          # an empty plus line
    assert st == TU.E_INVALID and o5[4] == 1
    five = good[0] + b"@r1\n"
    st, o5, _, _ = TU.same_as_model(lib, five, TU.FASTQ)
    assert st == TU.E_INVALID and o5[4] == 1 and o5[0] == 1
    st, o5, _, _ = TU.same_as_model(lib, five, TU.FASTQ, TU.PARTIAL)
    assert st == TU.OK and o5[0] == 1 and o5[3] == len(good[0])
    # the incomplete record is not looked at: its header may be anything
    st, o5, _, _ = TU.same_as_model(lib, good[0] + b">r1\nAC", TU.FASTQ, TU.PARTIAL)
    assert st == TU.OK and o5[:2] == [1, 3]


# ------------------------------------------------------------------ 6 + 7. sizing, capacity and the memory contract
def _guarded(lib, arena, text, fmt, flags, stream, cap_reads=None, cap_bases=None):
    """The full call on buffers of exactly the bytes the contract names, each at the weakest address it allows."""
    want = TU.parse(text, fmt, flags)
    n, total = want[1][0], want[1][1]
    cap_reads = n if cap_reads is None else cap_reads
    cap_bases = total if cap_bases is None else cap_bases
    t = arena.freeze(arena.put("text", np.frombuffer(text, np.uint8), align=1), "text")
    bases = arena.alloc("bases", cap_bases, align=1)
    offs = arena.alloc("offsets", 8 * (cap_reads + 1), align=8)
    tb = TU.tmp_bytes(lib, len(text), cap_reads)
    tmp = arena.alloc("tmp", tb, align=256)
    assert arena.addr("text") % 2 == 1 and arena.addr("bases") % 2 == 1
    assert arena.addr("offsets") % 16 == 8 and arena.addr("tmp") % 512 == 256
    rc, out5 = TU.raw_call(lib, arena.addr("text"), len(text), fmt, flags, TU.ACGT4, arena.addr("bases"), cap_bases,
                           arena.addr("offsets"), cap_reads, arena.addr("tmp"), tb, stream)
    del t, tmp
    return want, rc, out5, bases, offs


def test_sizing_and_capacity(lib):
    import torch
    stream = torch.cuda.current_stream().cuda_stream
    for fmt, text in ((TU.FASTQ, TU.MIXED_FASTQ), (TU.LINES, b"ACGT\n\nGG\r\nT\nNNA\nC\nGGG")):
        want = TU.same_as_model(lib, text, fmt)                      # the sizing call gives the full call's out5
        n, total = want[1][0], want[1][1]
        for cap_reads, cap_bases in ((n - 1, total), (n, total - 1), (0, 0), (n - 1, total - 1)):
            a = Arena("cuda", 0x5A, capacity=1 << 20)
            _, rc, out5, bases, offs = _guarded(lib, a, text, fmt, 0, stream, cap_reads, cap_bases)
            torch.cuda.synchronize()
            assert rc == TU.E_CAPACITY and out5 == want[1], (cap_reads, cap_bases)
            a.check()
            a.check_frozen()
            assert a.holds_poison(bases)                            # no base is stored when the call fails
        # roomy capacities are fine, and what lies behind the outputs stays as it was
        a = Arena("cuda", 0x5A, capacity=1 << 20)
        _, rc, out5, bases, offs = _guarded(lib, a, text, fmt, 0, stream, n + 5, total + 100)
        assert rc == TU.OK and out5 == want[1]
        assert np.array_equal(as_numpy(offs, np.int64)[:n + 1], want[2]) and a.holds_poison(offs[8 * (n + 1):])
        assert np.array_equal(as_numpy(bases, np.uint8)[:total], want[3]) and a.holds_poison(bases[total:])
        a.check()


@pytest.mark.parametrize("which", ["mixed", "random_lines"])
def test_memory_contract(lib, random_lines, which):
    import torch
    stream = torch.cuda.current_stream().cuda_stream
    fmt, text = (TU.FASTQ, TU.MIXED_FASTQ) if which == "mixed" else (TU.LINES, random_lines)
    results = []
    for poison in POISONS:
        a = Arena("cuda", poison, capacity=8 << 20)
        want, rc, out5, bases, offs = _guarded(lib, a, text, fmt, 0, stream)
        torch.cuda.synchronize()
        assert rc == TU.OK and out5 == want[1]
        a.check()
        a.check_frozen()
        results.append((as_numpy(offs, np.int64), as_numpy(bases, np.uint8)))
        assert np.array_equal(results[-1][0], want[2]) and np.array_equal(results[-1][1], want[3])
    for o, b in results[1:]:
        assert np.array_equal(o, results[0][0]) and np.array_equal(b, results[0][1])


# ------------------------------------------------------------------ 8. stream
def test_explicit_stream(lib, random_lines):
    """Every launch goes to the stream given and the call waits for it: no other synchronisation before the outputs are read."""
    import torch
    text = random_lines[:300_000] + TU.MIXED_FASTQ
    want = TU.parse(text, TU.LINES)
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()                                        # the default stream is idle
    with torch.cuda.stream(stream):                                 # the arena's fill and the input copy go ahead on that stream
        a = Arena("cuda", 0x5A, capacity=4 << 20)
        _, rc, out5, bases, offs = _guarded(lib, a, text, TU.LINES, 0, stream.cuda_stream)
        got = (as_numpy(offs, np.int64), as_numpy(bases, np.uint8))
    assert rc == TU.OK and out5 == want[1]
    assert np.array_equal(got[0], want[2]) and np.array_equal(got[1], want[3])
    torch.cuda.synchronize()
    a.check()
    a.check_frozen()


# ------------------------------------------------------------------ 9. drop-in, end to end
@pytest.fixture(scope="module")
def dropin(pkg):
    d, _ = G.load("syn10k_K8")
    ref = G.codes_to_str(d["ref_codes"])
    m = pkg.ExactMatch("syn10k.fa")
    m.set_reference(ref)
    sm = pkg.SMEM(m, 8)
    rng = np.random.default_rng(17)
    reads = []
    for i in range(200):
        L = int(rng.integers(30, 301))
        at = int(rng.integers(0, len(ref) - L))
        q = list(ref[at:at + L])
        if i % 8 == 3:
            for pos in rng.integers(0, L, int(rng.integers(1, 4))):
                q[int(pos)] = "N"
        reads.append("".join(q))
    pieces = []
    while sum(map(len, pieces)) < 20_000:
        L = int(rng.integers(200, 3000))
        at = int(rng.integers(0, len(ref) - L))
        pieces.append(ref[at:at + L])
    reads.insert(77, "".join(pieces)[:20_000])
    as_lines = "\n".join(reads).encode() + b"\n"
    as_fastq = "".join(f"@read{i} len={len(r)}\n{r}\n+\n{'I' * len(r)}\n" for i, r in enumerate(reads)).encode()
    return sm, reads, {"lines": as_lines, "fastq": as_fastq}


def _np3(t3):
    return tuple(t.cpu().numpy() for t in t3)


def _same3(got, want):
    for g, w, name in zip(got, want, ("offsets", "rows", "status")):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), name


@pytest.mark.parametrize("fmt", ["lines", "fastq"])
def test_dropin_text_equals_list_of_strings(dropin, fmt):
    sm, reads, texts = dropin
    for both in (False, True):
        want = _np3(sm.find_smems_long(reads, 1, both_strands=both, split_breaks=True))
        assert want[0][-1] > len(reads) and not want[2].any()
        _same3(_np3(sm.find_smems_text(texts[fmt], fmt, both_strands=both)), want)
    _same3(_np3(sm.find_smems_text(texts[fmt], fmt, minimum_length=20)), _np3(sm.find_smems_long(reads, 20, split_breaks=True)))
    # without split_breaks a read with an N is flagged, in LUT mode as in any other
    _, _, offs, bases = TU.parse(texts[fmt], TU.LINES if fmt == "lines" else TU.FASTQ, 0, sm.matcher.byte_codes())
    want = _np3(sm.find_smems_long((bases, offs), 1, mode="lut"))
    assert sorted(set(want[2].tolist())) == [0, 1] and int((want[2] == 1).sum()) == 25
    _same3(_np3(sm.find_smems_text(texts[fmt], fmt, mode="lut", split_breaks=False)), want)
    # the text may live on the device, or come as a numpy array
    import torch
    dev = torch.from_numpy(np.frombuffer(texts[fmt], np.uint8).copy()).cuda()
    want = _np3(sm.find_smems_long(reads, 1, split_breaks=True))
    _same3(_np3(sm.find_smems_text(dev, fmt)), want)
    _same3(_np3(sm.find_smems_text(np.frombuffer(texts[fmt], np.uint8), fmt)), want)


def test_dropin_fold_case_and_errors(dropin, pkg):
    sm, reads, texts = dropin
    want = _np3(sm.find_smems_long(reads[:20], 1, split_breaks=True))
    lower = ("\n".join(reads[:20]).lower() + "\n").encode()
    _same3(_np3(sm.find_smems_text(lower, fold_case=True)), want)
    assert _np3(sm.find_smems_text(lower))[0][-1] == 0              # without it every lower-case letter is a break
    with pytest.raises(pkg.text_reads.TextFormatError) as e:
        sm.find_smems_text(b"@a\nACGT\n+\nIIII\n>b\nAC\n+\nII\n", "fastq")
    assert e.value.record == 1
    bases, offs, consumed = pkg.text_reads.reads_from_text(b"ACGT\nAC", partial=True)
    assert (bases.cpu().tolist(), offs.cpu().tolist(), consumed) == ([0, 1, 2, 3], [0, 4], 5)


# ------------------------------------------------------------------ 10. iter_fastq_smems
def test_iter_fastq_smems_joins_to_the_whole_file(dropin, tmp_path):
    sm, reads, texts = dropin
    rng = np.random.default_rng(23)
    some = [r[:int(rng.integers(10, 121))] for r in reads[:50]]
    some[7] = ""
    text = "".join(f"@q{i}\n{r}\n+\n{'I' * len(r)}\n" for i, r in enumerate(some)).encode()[:-1]      # no newline at the end
    path = tmp_path / "reads.fq"
    path.write_bytes(text)
    for both in (False, True):
        want = _np3(sm.find_smems_text(text, "fastq", minimum_length=12, both_strands=both))
        chunks = [_np3(c) for c in sm.iter_fastq_smems(str(path), chunk_bytes=64, minimum_length=12, both_strands=both)]
        assert 10 < len(chunks) <= 50
        offsets = [np.zeros(1, np.int64)]
        for off, _, _ in chunks:
            assert off[0] == 0 and off.size > 1
            offsets.append(off[1:] + offsets[-1][-1])
        _same3((np.concatenate(offsets), np.concatenate([c[1] for c in chunks]), np.concatenate([c[2] for c in chunks])), want)
    whole = [_np3(c) for c in sm.iter_fastq_smems(str(path), minimum_length=12)]
    assert len(whole) == 1
    _same3(whole[0], _np3(sm.find_smems_text(text, "fastq", minimum_length=12)))
