"""GPU tests of genie_reads_from_fasta (run with -m gpu on an MI355X): FASTA text -> base codes back to back, int64 offsets
and record starts on the device.  Expected values come from the Python restatement of the specification in
tests/fasta_util.py; every comparison is exact: status, out5, offsets, bases, starts.  Through the raw C ABI unless a test
says drop-in."""
import numpy as np
import pytest

import fasta_util as FU
import golden_util as G
from guarded import POISONS, Arena, as_numpy

pytestmark = pytest.mark.gpu

TILE = 4096                  # bytes of text per block in csrc/text_reads.inc (tiles lie on the 16-byte grid of the address)
BOTH = (0, FU.PARTIAL)


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


def _sequence(rng, n, alphabet=b"ACGTNacgt"):
    return np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), n)].tobytes()


def _wrap(seq, width, eol=b"\n"):
    return b"".join(seq[i:i + width] + eol for i in range(0, len(seq), width))


# ------------------------------------------------------------------ 1. edge texts
EDGE_TEXTS = [b"", b">", b">\n", b"\n\n", b">a", b">a\n\n\n\n>b\n\n", b">\r\n", b">a\nA\rC\n", b">a\nAC\r", b">a\nAC\r\n", b"\r",
              b"\r\n", b"\n\r\n>a\r\nAC\r\n\r\nGT\r\n>b\r\n", b">a\n>b\n>c", b">a\nA>C\n;x\n >\n", b">a\n\r\r\n\r", b">>\n>\n",
              b">a\nAC\n>b", b">a\nAC\n>b\n", b"\n>a\nACGTNacgtn\x00\xff\n"]


def test_edge_texts(lib):
    for text in EDGE_TEXTS:
        for flags in BOTH:
            want = FU.same_as_model(lib, text, flags)
            assert want[0] == FU.OK or text == b"\r", text
    want = FU.same_as_model(lib, b"")
    assert want[1] == [0, 0, 0, 0, -1] and want[2].tolist() == [0]
    assert FU.same_as_model(lib, b">a\nAC\r")[3].tolist() == [0, 1, 4]         # a '\r' that ends the text is kept ...
    assert FU.same_as_model(lib, b">a\nAC\r", FU.PARTIAL)[1] == [0, 0, 0, 0, -1]   # ... and is tail in a partial text
    # another table: a three-letter alphabet of its own, and entries above 4 clamp to 4
    table = np.full(256, 9, np.uint8)
    table[list(b"XYZ")] = [0, 1, 2]
    table[ord("Q")] = 200
    FU.same_as_model(lib, b">h\nXYZQ\nAX>\n>\nZ", 0, table)


# ------------------------------------------------------------------ 2. tile and vector edges
def _edge_text(rng, pos, kind):
    """About three tiles of FASTA with, at text position `pos`: a header's '>' ("gt"), the '\\n' in front of a header's
    '>' ("nl"), or the '\\r' of a "\\r\\n" ("crlf": at pos = edge - 1 the pair is split across the edge)."""
    body = b">s0 first\n" + _wrap(_sequence(rng, 3 * TILE), 60)
    if kind == "gt":
        head = body[:pos - 1] + b"\n" + b">at the edge\r\n"
    elif kind == "nl":
        head = body[:pos - 1] + b"A\n" + b">behind the edge\n"
    else:
        head = body[:pos - 1] + b"C\r\n"
    assert head[pos] == {"gt": ord(">"), "nl": 0x0A, "crlf": 0x0D}[kind]
    rest = _wrap(_sequence(rng, 3 * TILE + 200 - len(head)), 70, b"\r\n") + b">last\nACGT"
    return head + rest


def _edge_positions():
    return [e + d for e in (TILE, 2 * TILE) for d in range(-15, 17)]


@pytest.mark.parametrize("kind", ["gt", "nl", "crlf"])
def test_tile_and_vector_edges(lib, kind):
    rng = np.random.default_rng(3)
    for pos in _edge_positions():
        text = _edge_text(rng, pos, kind)
        assert 3 * TILE < len(text) < 3 * TILE + 600
        for flags in BOTH:
            want = FU.same_as_model(lib, text, flags)
            assert want[0] == FU.OK and want[1][0] == (3 if kind != "crlf" else 2) - (flags & 1)


def test_odd_addresses(lib):
    """One text with all three kinds of edge, at each of the 16 addresses modulo 16 (the tiles follow the address, so every
    feature meets an edge at some address), with d_bases at an odd address."""
    import torch
    rng = np.random.default_rng(4)
    text = b">s0\n" + _wrap(_sequence(rng, 3 * TILE), 60)
    for at, piece in ((TILE - 9, b"\n>edge one\r\n"), (TILE - 1, b"G\r\n"), (2 * TILE - 8, b"\r\n>edge two\n"), (2 * TILE - 1, b"\n>\n"),
                      (3 * TILE - 7, b"T\r\n>x\r\n")):
        text = text[:at] + piece + text[at + len(piece):]
    stream = torch.cuda.current_stream().cuda_stream
    buf = torch.zeros(len(text) + 64, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    tb = FU.tmp_bytes(lib, len(text), 100)
    tmp = torch.empty(tb, dtype=torch.uint8, device="cuda")
    for flags in BOTH:
        want = FU.parse(text, flags)
        n, total = want[1][0], want[1][1]
        assert want[0] == FU.OK and n >= 4
        for lead in range(16):
            buf.fill_(0x0A)                                          # newlines around the text: never read
            buf[lead:lead + len(text)] = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).cuda()
            offs = torch.full((n + 2,), -77, dtype=torch.int64, device="cuda")
            starts = torch.full((n + 1,), -55, dtype=torch.int64, device="cuda")
            bases = torch.full((total + 10,), 0xA5, dtype=torch.uint8, device="cuda")
            assert bases.data_ptr() % 2 == 0
            rc, out5 = FU.raw_call(lib, buf.data_ptr() + lead, len(text), flags, FU.ACGT4, bases.data_ptr() + 1, total, offs.data_ptr(),
                                   starts.data_ptr(), n, tmp.data_ptr(), tb, stream)
            assert (rc, out5) == (FU.OK, want[1]), lead
            assert offs.cpu().tolist() == want[2].tolist() + [-77], lead
            assert starts.cpu().tolist() == want[4].tolist() + [-55], lead
            b = bases.cpu().numpy()
            assert b[0] == 0xA5 and np.array_equal(b[1:total + 1], want[3]) and (b[total + 1:] == 0xA5).all(), lead


# ------------------------------------------------------------------ 3. long sequences
def test_long_sequences(lib):
    rng = np.random.default_rng(5)
    one_line = b">short\nACG\n>one line\n" + _sequence(rng, 10_000) + b"\n>behind\nTT\n"       # more than two tiles
    want = FU.same_as_model(lib, one_line)
    assert want[1][:3] == [3, 10_005, 10_000]
    FU.same_as_model(lib, one_line, FU.PARTIAL)
    wrapped = b">a\nAC\n>wrapped\n" + _wrap(_sequence(rng, 300 * 60), 60) + b">c\nG\n"
    want = FU.same_as_model(lib, wrapped)
    assert want[1][:3] == [3, 18_003, 18_000]
    assert FU.same_as_model(lib, wrapped, FU.PARTIAL)[1][:3] == [2, 18_002, 18_000]
    assert FU.same_as_model(lib, wrapped[:-5])[1][:3] == [2, 18_002, 18_000]                  # the last read ends with the text


# ------------------------------------------------------------------ 4. many tiny records
@pytest.fixture(scope="module")
def tiny_records():
    """3000 records of 0 .. 3 bases in about 20 kB: more headers than one scan block holds."""
    rng = np.random.default_rng(11)
    recs = []
    for i in range(3000):
        seq = _sequence(rng, int(rng.integers(0, 4)), b"ACGTN\r")
        recs.append(b">%d\n" % (i % 7) + (seq + b"\n" if i % 3 else _wrap(seq, 1, b"\r\n")))
    return b"".join(recs)


def test_many_tiny_records(lib, tiny_records):
    assert 15_000 < len(tiny_records) < 25_000
    want = FU.same_as_model(lib, tiny_records)
    assert want[1][0] == 3000
    assert FU.same_as_model(lib, tiny_records, FU.PARTIAL)[1][0] == 2999


@pytest.mark.parametrize("head", [b"", b">x\nA"])
def test_densest_headers(lib, head):
    """A header every two bytes, TILE / 2 in every full tile -- the most a tile can hold -- at both parities of the headers
    against the tile grid (behind the head the first '>' ends the line "A>", so both texts hold as many records)."""
    text = head + b">\n" * (2 * TILE + 3)
    assert FU.same_as_model(lib, text)[1][0] == 2 * TILE + 3
    assert FU.same_as_model(lib, text, FU.PARTIAL)[1][0] == 2 * TILE + 2


def test_more_than_1024_tiles(lib):
    """A little over 4 MiB: the one-block scans over the tiles take a second round."""
    rng = np.random.default_rng(12)
    seq = _sequence(rng, 100_000)
    parts = []
    for i in range(42):
        parts.append(b">long%d\n" % i + _wrap(seq[i:], 70 + i % 11))
        parts.append(b">e%d\r\n>t%d\nAC\nG\n" % (i, i))
    text = b"".join(parts)
    assert 1024 * TILE < len(text) < 1100 * TILE
    want = FU.same_as_model(lib, text)
    assert want[1][0] == 126 and want[1][2] == 100_000
    FU.same_as_model(lib, text, FU.PARTIAL)


# ------------------------------------------------------------------ 5. GENIE_TEXT_PARTIAL
def test_partial_at_every_prefix(lib):
    from test_fasta_reads_host import _resume_texts
    text = (b"".join(_resume_texts()) * 2)[:300]
    assert len(text) == 300 and FU.parse(text)[0] == FU.OK
    whole = FU.parse(text)
    for p in range(len(text) + 1):
        st, o5, offs, bases, starts = FU.same_as_model(lib, text[:p], FU.PARTIAL)
        assert st == FU.OK and o5[3] <= p, p
    for p in (0, 1, 57, 150, 299, 300):                             # and the rest of the text resumes there, on the device
        _, o5, offs, bases, starts = FU.device_parse(lib, text[:p], FU.PARTIAL)
        st2, _, offs2, bases2, starts2 = FU.device_parse(lib, text[o5[3]:])
        assert st2 == FU.OK
        assert FU.reads_of(offs, bases) + FU.reads_of(offs2, bases2) == FU.reads_of(whole[2], whole[3]), p
        assert starts.tolist() + (starts2 + o5[3]).tolist() == whole[4].tolist(), p


# ------------------------------------------------------------------ 6 .. 8. malformed text, capacity, the memory contract
def _guarded(lib, arena, text, flags, stream, cap_reads=None, cap_bases=None, with_starts=True):
    """The full call on buffers of exactly the bytes the contract names, each at the weakest address it allows."""
    want = FU.parse(text, flags)
    n, total = want[1][0], want[1][1]
    cap_reads = n if cap_reads is None else cap_reads
    cap_bases = total if cap_bases is None else cap_bases
    t = arena.freeze(arena.put("text", np.frombuffer(text, np.uint8), align=1), "text")
    bases = arena.alloc("bases", cap_bases, align=1)
    offs = arena.alloc("offsets", 8 * (cap_reads + 1), align=8)
    starts = arena.alloc("starts", 8 * cap_reads, align=8) if with_starts else None
    tb = FU.tmp_bytes(lib, len(text), cap_reads)
    tmp = arena.alloc("tmp", tb, align=256)
    assert arena.addr("text") % 2 == 1 and arena.addr("bases") % 2 == 1
    assert arena.addr("offsets") % 16 == 8 and arena.addr("tmp") % 512 == 256
    rc, out5 = FU.raw_call(lib, arena.addr("text"), len(text), flags, FU.ACGT4, arena.addr("bases"), cap_bases, arena.addr("offsets"),
                           arena.addr("starts") if with_starts else 0, cap_reads, arena.addr("tmp"), tb, stream)
    del t, tmp
    return want, rc, out5, bases, offs, starts


def test_malformed_text(lib):
    import torch
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(6)
    good = b">a\n" + _wrap(_sequence(rng, 500), 60) + b">b\nACGT\n"
    late = b"\n" * (TILE + 100) + b"\r\n" * 50                       # the offending line starts in the second tile
    for text in (b"AC\n>a\nAC\n", b"AC", b"AC\n", b";comment\n" + good, b" " + good, late + b"N\n" + good, late + b"\r\r\n" + good,
                 b"\n" * (3 * TILE) + b"x"):
        for flags in BOTH:
            want = FU.same_as_model(lib, text, flags)
            assert (want[0] == FU.E_INVALID) == (want[1][4] == 0)
            assert want[0] == FU.E_INVALID or (flags and text in (b"AC", b"\n" * (3 * TILE) + b"x")), (text[:20], flags)
    assert FU.same_as_model(lib, late + good)[0] == FU.OK           # leading empty lines are fine
    # nothing outside the buffers is touched, whatever their sizes, and a malformed text is reported before a capacity
    text = late + b"N\n" + good
    for cap_reads, cap_bases in ((None, None), (0, 0), (1, 3), (50, 5000)):
        a = Arena("cuda", 0x5A, capacity=1 << 20)
        want, rc, out5, bases, offs, starts = _guarded(lib, a, text, 0, stream, cap_reads, cap_bases)
        torch.cuda.synchronize()
        assert rc == FU.E_INVALID and out5 == want[1] and out5[4] == 0 and out5[0] == 2
        a.check()
        a.check_frozen()


def test_sizing_and_capacity(lib):
    import torch
    stream = torch.cuda.current_stream().cuda_stream
    text = b"\n>r0 x\nACGT\nAC\n>r1\n>r2\r\nGG\r\nN\r\n>r3\nA>C\n\nT"
    for flags in BOTH:
        want = FU.same_as_model(lib, text, flags)                    # the sizing call gives the full call's out5
        n, total = want[1][0], want[1][1]
        assert n == 4 - (flags & 1) and total > 8
        for cap_reads, cap_bases in ((n - 1, total), (n, total - 1), (0, 0), (n - 1, total - 1)):
            a = Arena("cuda", 0x5A, capacity=1 << 20)
            _, rc, out5, bases, offs, starts = _guarded(lib, a, text, flags, stream, cap_reads, cap_bases)
            torch.cuda.synchronize()
            assert rc == FU.E_CAPACITY and out5 == want[1], (cap_reads, cap_bases)
            a.check()
            a.check_frozen()
            assert a.holds_poison(bases)                            # no base is stored when the call fails
        # roomy capacities are fine, and what lies behind the outputs stays as it was
        a = Arena("cuda", 0x5A, capacity=1 << 20)
        _, rc, out5, bases, offs, starts = _guarded(lib, a, text, flags, stream, n + 5, total + 100)
        assert rc == FU.OK and out5 == want[1]
        assert np.array_equal(as_numpy(offs, np.int64)[:n + 1], want[2]) and a.holds_poison(offs[8 * (n + 1):])
        assert np.array_equal(as_numpy(starts, np.int64)[:n], want[4]) and a.holds_poison(starts[8 * n:])
        assert np.array_equal(as_numpy(bases, np.uint8)[:total], want[3]) and a.holds_poison(bases[total:])
        a.check()
        # d_record_starts is optional
        a = Arena("cuda", 0x5A, capacity=1 << 20)
        _, rc, out5, bases, offs, _ = _guarded(lib, a, text, flags, stream, with_starts=False)
        assert rc == FU.OK and out5 == want[1]
        assert np.array_equal(as_numpy(offs, np.int64), want[2]) and np.array_equal(as_numpy(bases, np.uint8), want[3])
        a.check()


@pytest.mark.parametrize("which", ["wrapped", "tiny_records"])
def test_memory_contract(lib, tiny_records, which):
    import torch
    stream = torch.cuda.current_stream().cuda_stream
    if which == "wrapped":
        text = _edge_text(np.random.default_rng(8), TILE - 1, "crlf")
    else:
        text = tiny_records
    for flags in BOTH:
        results = []
        for poison in POISONS:
            a = Arena("cuda", poison, capacity=2 << 20)
            want, rc, out5, bases, offs, starts = _guarded(lib, a, text, flags, stream)
            torch.cuda.synchronize()
            assert rc == FU.OK and out5 == want[1]
            a.check()
            a.check_frozen()
            results.append((as_numpy(offs, np.int64), as_numpy(bases, np.uint8), as_numpy(starts, np.int64)))
            for got, exp in zip(results[-1], want[2:]):
                assert np.array_equal(got, exp)
        for res in results[1:]:
            for got, first in zip(res, results[0]):
                assert np.array_equal(got, first)


def test_explicit_stream(lib, tiny_records):
    """Every launch goes to the stream given and the call waits for it: no other synchronisation before the outputs are read."""
    import torch
    text = tiny_records + _edge_text(np.random.default_rng(9), 2 * TILE + 3, "gt")
    want = FU.parse(text)
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()                                        # the default stream is idle
    with torch.cuda.stream(stream):                                 # the arena's fill and the input copy go ahead on that stream
        a = Arena("cuda", 0x5A, capacity=2 << 20)
        _, rc, out5, bases, offs, starts = _guarded(lib, a, text, 0, stream.cuda_stream)
        got = (as_numpy(offs, np.int64), as_numpy(bases, np.uint8), as_numpy(starts, np.int64))
    assert rc == FU.OK and out5 == want[1]
    for g, w in zip(got, want[2:]):
        assert np.array_equal(g, w)
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
    rng = np.random.default_rng(19)
    reads = []
    for i in range(12):
        pieces = []
        L = int(rng.integers(20_000, 30_001))
        while sum(map(len, pieces)) < L:
            n = int(rng.integers(200, 3000))
            at = int(rng.integers(0, len(ref) - n))
            pieces.append(ref[at:at + n])
        q = list("".join(pieces)[:L])
        if i % 3 == 1:
            for pos in rng.integers(0, L, 5):
                q[int(pos)] = "N"
        if i % 4 == 2:
            for pos in rng.integers(0, L, 7):
                q[int(pos)] = q[int(pos)].lower()
        reads.append("".join(q))
    names = [b"read%d" % i for i in range(12)]

    def fasta(width, eol):
        return b"".join(b">" + nm + b" len=%d" % len(r) + eol + _wrap(r.encode(), width, eol) for nm, r in zip(names, reads))

    return sm, reads, names, {"w60": fasta(60, b"\n"), "w80crlf": fasta(80, b"\r\n")}


def _np3(t3):
    return tuple(t.cpu().numpy() for t in t3)


def _same3(got, want):
    for g, w, name in zip(got, want, ("offsets", "rows", "status")):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), name


@pytest.mark.parametrize("which", ["w60", "w80crlf"])
def test_dropin_fasta_equals_list_of_strings(dropin, pkg, which):
    sm, reads, names, texts = dropin
    text = texts[which]
    for both in (False, True):
        want = _np3(sm.find_smems_long(reads, 1, both_strands=both, split_breaks=True))
        assert want[0][-1] > len(reads) and not want[2].any()
        _same3(_np3(sm.find_smems_text(text, "fasta", both_strands=both)), want)
    _same3(_np3(sm.find_smems_text(text, "fasta", minimum_length=20)), _np3(sm.find_smems_long(reads, 20, split_breaks=True)))
    bases, offs, consumed, starts = pkg.text_reads.reads_from_text(text, "fasta", sm.matcher.byte_codes(), return_starts=True)
    assert consumed == len(text) and offs.cpu().tolist() == np.cumsum([0] + [len(r) for r in reads]).tolist()
    assert pkg.text_reads.record_names(text, starts) == names
    with pytest.raises(ValueError):
        pkg.text_reads.reads_from_text(text, "lines", return_starts=True)
    with pytest.raises(ValueError):
        pkg.text_reads.reads_from_text(text, "fastx")


def test_iter_fasta_smems_joins_to_the_whole_file(dropin, pkg, tmp_path):
    sm, reads, names, texts = dropin
    text = texts["w80crlf"][:-2]                                     # no newline at the end
    path = tmp_path / "reads.fa"
    path.write_bytes(text)
    want = _np3(sm.find_smems_text(text, "fasta", minimum_length=15))
    chunks = [_np3(c) for c in sm.iter_fasta_smems(str(path), chunk_bytes=50_000, minimum_length=15)]
    assert 3 < len(chunks) <= 12
    offsets = [np.zeros(1, np.int64)]
    for off, _, _ in chunks:
        assert off[0] == 0 and off.size > 1
        offsets.append(off[1:] + offsets[-1][-1])
    _same3((np.concatenate(offsets), np.concatenate([c[1] for c in chunks]), np.concatenate([c[2] for c in chunks])), want)
    whole = [_np3(c) for c in sm.iter_text_smems(str(path), "fasta", minimum_length=15)]
    assert len(whole) == 1
    _same3(whole[0], want)
    bad = tmp_path / "bad.fa"
    bad.write_bytes(b"ACGT\n" + text)
    with pytest.raises(pkg.text_reads.TextFormatError) as e:
        sm.find_smems_text(bad.read_bytes(), "fasta")
    assert e.value.record == 0
    with pytest.raises(pkg.text_reads.TextFormatError) as e:
        list(sm.iter_fasta_smems(str(bad), chunk_bytes=50_000))
    assert e.value.record == 0
