"""GPU: genie_bam_records against the brute-force encoder of tests/bam_util.py, every byte and every record offset exactly
equal, on the 16 kb three-contig reference of tests/test_sam_text_gpu.py; and, where names have 1 to 254 bytes, reads at least
one base and qualities are 33 or more, the device bytes decoded by bam_util's independent decoder equal to the lines that
GenieIndex.sam_text writes from the same inputs.  Synthetic batches as in the text's tests: names whose lengths put the records
at every alignment mod 4 and around the 254-byte cut, read lengths around the wave's 64 and 128 lanes on both strands, code 4
on strand 1, op counts around 64 and at the 65535 / 65536 edge of the CG convention, reads without records at every place,
mates on different contigs, every tag subset, no qualities, no SEQ, no contig table, single-end mode, POS values at the five
bin boundaries, capacities that cut a record's head and its SEQ, and more records than one grid of waves.  Then the pipeline:
SMEM.bam_records on map_pairs(rescue=True) decodes to SMEM.sam_text's lines, and SMEM.write_bam round-trips through gzip."""
import gzip
import struct

import numpy as np
import pytest

import align_util as AU
import bam_util as BU
import sam_text_util as ST

pytestmark = pytest.mark.gpu

N_REF = 1 << 14
TABLE = np.asarray([0, 6000, 11000, N_REF], np.int64)
ALL = ST.NM | ST.AS | ST.MD | ST.MC | ST.MQ
NO_MD = ALL & ~ST.MD
EQ, X, D, I, S = ST.EQ, ST.X, ST.D, ST.I, ST.S
op = ST.op


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import genie_smem_amd as g

    class Env:
        pass
    e = Env()
    e.g, e.lib = g, g._native.lib()
    e.T = np.random.default_rng(60).integers(0, 4, N_REF).astype(np.uint8)
    e.ix = g.GenieIndex.build(e.T, 0).to("cuda")
    e.rs = g.ReferenceSet(["a", "b", "c"], TABLE, e.T)
    return e


def _np(t):
    import torch
    return (t.view(torch.int32) if t.dtype == torch.uint32 else t).cpu().numpy()


def _decodable(b, flags):
    """Where BAM says what the text says: the restriction on names, reads and qualities, and no contig column past the names
    (the text compares the columns for `=`, BAM has only the clamped indices)."""
    ro = b["read_offsets"]
    return (all(1 <= len(x) <= 254 for x in b["names"]) and (flags & ST.NO_SEQ or (np.diff(ro) >= 1).all()) and
            (b["quals"] is None or (b["quals"] >= 33).all()) and
            (b["records"].shape[0] == 0 or 0 <= b["records"][:, 4].min() <= b["records"][:, 4].max() < len(b["contig_names"])))


def _through_the_wrapper(env, b, tags, flags):
    """GenieIndex.bam_records and GenieIndex.sam_text on the same inputs -> (data, record_offsets, totals, the text's lines)."""
    args = (b["bases"], b["read_offsets"], b["sel_offsets"], b["records"], b["sam"], b["info"], b["cigar_offsets"], b["cigar"].view(np.int32),
            *ST.csr(b["names"]), *ST.csr(b["contig_names"]))
    kw = dict(quals=b["quals"], contigs=env.rs if b.get("contig_offsets") is not None else None, tags=tags, seq=not flags & ST.NO_SEQ)
    data, off, totals = env.ix.bam_records(*args, **kw)
    text = bytes(_np(env.ix.sam_text(*args, **kw)[0])).decode("latin-1").split("\n")
    assert text[-1] == ""
    return _np(data), _np(off), _np(totals), text[:-1]


def _exact(env, b, tags=ALL, flags=0, decode=True, **kw):
    want = BU.host_bam_records(b, env.T, tags, flags, kw.get("n_records"))
    got = BU.call(env.lib, env.ix, b, tags, flags, **kw)
    BU.agrees(got, want, kw.get("cap_data"))
    if decode and not kw and _decodable(b, flags):
        data, off, totals, lines = _through_the_wrapper(env, b, tags, flags)
        assert np.array_equal(data, want["data"]) and np.array_equal(off, want["record_offsets"]) and totals.tolist() == want["totals"].tolist()
        assert BU.bam_to_sam(data, b["contig_names"]) == lines
    return got, want


def _dense_ops(rng, n_ops):
    """n_ops ops that cover little of the reference: = runs of 1 to 3 bases with X, I and D of 1 or 2 between them."""
    return [op(int(rng.integers(1, 4)), EQ) if i % 2 == 0 else op(int(rng.integers(1, 3)), int(rng.choice([X, X, D, I]))) for i in range(n_ops)]


def _head(data, at=0):
    return struct.unpack_from("<iiiBBHHHiiii", data, at)


def test_name_lengths_put_records_at_every_alignment(env):
    rng = np.random.default_rng(161)
    lengths = (1, 2, 3, 4, 5, 253, 254, 255, 300, 0)
    reads, names = [], []
    for k, n in enumerate(lengths):
        reads.append((21 + k, [dict(ops=[op(3, S), op(17 + k, EQ), op(1, X)], contig=k % 3, offset=40 + k, strand=k & 1)]))
        reads.append((20, [] if k % 3 == 2 else [dict(ops=[op(20, EQ)], contig=k % 3, offset=400, strand=1)]))
        names += [bytes(97 + (i + k) % 26 for i in range(n))] * 2
    b = ST.make_batch(rng, reads, names=names, contig_offsets=TABLE)
    got, want = _exact(env, b)
    starts = want["record_offsets"][:-1]
    assert set((starts % 4).tolist()) == {0, 1, 2, 3}                # records at every alignment
    l_names = [want["data"][int(s) + 12] for s in starts]
    assert {2, 3, 4, 5, 6, 254, 255}.issubset(set(l_names)) and max(l_names) == 255
    at = int(starts[-1])
    assert bytes(want["data"][at + 36:at + 38]) == b"*\0"            # the empty name
    # the same without the names that SAM text and BAM write differently: the decoded records are the text's lines
    keep = [k for k, n in enumerate(lengths) if 1 <= n <= 254]
    short = ST.make_batch(rng, [reads[2 * k + i] for k in keep for i in (0, 1)], names=[names[2 * k] for k in keep for _ in (0, 1)],
                          contig_offsets=TABLE)
    assert _decodable(short, 0)
    _exact(env, short)
    _exact(env, short, ST.NM, ST.NO_SEQ)


def test_read_lengths_on_both_strands_and_code_4(env):
    rng = np.random.default_rng(162)
    reads = []
    for k, length in enumerate((0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 5000)):
        reads.append((length, [dict(ops=[op(max(length, 1), EQ)], contig=k % 3, offset=1 + k, strand=0),
                               dict(ops=[op(4, S), op(9, EQ)], contig=2, offset=77, strand=1, kind=1)]))
        reads.append((length, [] if k % 2 else [dict(ops=[op(5, EQ), op(1, X)], contig=k % 3, offset=200, strand=1)]))
    b = ST.make_batch(rng, reads, contig_offsets=TABLE, code4=0.2)
    assert (b["bases"] == 4).sum() > 500
    got, want = _exact(env, b)
    assert 15 in (want["data"] >> 4).tolist()
    _exact(env, dict(b, quals=None))
    _exact(env, b, ALL, ST.NO_SEQ)
    some = ST.make_batch(rng, reads[2:], contig_offsets=TABLE, code4=0.2)      # without the reads of no bases: decodable
    assert _decodable(some, 0)
    got, want = _exact(env, some)
    lines = BU.bam_to_sam(got["data"], some["contig_names"])
    assert sum("N" in ln.split("\t")[9] for ln in lines) >= 8
    _exact(env, dict(some, quals=None))


def test_op_counts(env):
    rng = np.random.default_rng(163)
    reads = []
    for n_ops in (0, 1, 63, 64, 65, 130, 3001):
        ops = _dense_ops(rng, n_ops)
        mate = _dense_ops(rng, 130 if n_ops == 64 else 2)
        reads.append((max(ST.query_length(ops), 1), [dict(ops=ops, contig=1, offset=17, strand=n_ops & 1)]))
        reads.append((40, [dict(ops=mate, contig=1, offset=300, strand=1), dict(ops=_dense_ops(rng, 65), contig=2, offset=9, kind=1)]))
    digits = [op(7, S), op(3, EQ), op(2, X), op(12, D), op(10, EQ), op(1, I)] + [op(10**k + k, EQ) for k in range(1, 8)]
    digits += [op(2**28 - 1, EQ), op(123456789, EQ), op(2**28 - 1, S)]
    reads.append((50, [dict(ops=digits, contig=0, offset=5)]))
    reads.append((50, [dict(ops=[op(100000000, S), op(999999999 >> 2, EQ)], contig=0, offset=900, strand=1)]))
    b = ST.make_batch(rng, reads, contig_offsets=TABLE)
    got, want = _exact(env, b)
    assert max(np.diff(b["cigar_offsets"])) == 3001 and int(np.diff(want["record_offsets"]).max()) > 12000
    _exact(env, b, ST.MD)
    _exact(env, b, ST.MC | ST.NM, ST.NO_SEQ)


def test_65535_ops_fit_the_field_and_65536_use_cg(env):
    rng = np.random.default_rng(164)
    reads = [(131072, [dict(ops=[op(2, EQ)] * 65535, contig=0, offset=11)]),
             (131072, [dict(ops=[op(2, EQ)] * 65536, contig=0, offset=21, strand=1)])]
    b = ST.make_batch(rng, reads, contig_offsets=TABLE)
    got, want = _exact(env, b, NO_MD)                                # one batch: the raw calls, then the wrappers on it
    off = got["record_offsets"]
    h0, h1 = _head(got["data"]), _head(got["data"], int(off[1]))
    assert h0[6] == 65535 and h1[6] == 2 and h0[8] == h1[8] == 131072
    tail = bytes(got["data"][int(off[2]) - 8 - 4 * 65536:int(off[2])])
    assert tail[:8] == b"CGBI" + struct.pack("<i", 65536) and tail[8:] == struct.pack("<I", 2 << 4 | 7) * 65536
    assert b"CGBI" not in bytes(got["data"][int(off[1]) - 4 * 65535 - 200:int(off[1])])
    assert h1[5] == BU.reg2bin(20, 20 + 131072) & 0xffff
    lines = BU.bam_to_sam(got["data"], b["contig_names"])
    assert lines[1].split("\t")[5] == "2=" * 65536                   # the decoder undoes the convention


def test_reads_without_records_everywhere(env):
    rng = np.random.default_rng(165)
    counts = [0, 2, 0, 0, 1, 1, 3, 0, 0, 0, 2, 2, 1, 0]             # at the start, at the end, two in a row, both mates of a pair
    reads = [(max(n, 1), recs) for n, recs in ST.random_reads(rng, counts, TABLE)]
    b = ST.make_batch(rng, reads, contig_offsets=TABLE)
    got, want = _exact(env, b)
    assert want["totals"].tolist()[0::2] == [sum(counts) + counts.count(0), counts.count(0)]
    flags = [_head(got["data"], int(s))[7] for s in got["record_offsets"][:-1]]
    # an unmapped read with a placed mate (0x8 clear) and without one (0x8 set)
    assert sum(f & 4 > 0 for f in flags) == 7 and sum(f & 12 == 12 for f in flags) == 4 and sum(f & 12 == 4 for f in flags) == 3
    for s, f in zip(got["record_offsets"][:-1], flags):
        h = _head(got["data"], int(s))
        if f & 12 == 12:
            assert h[1:3] == (-1, -1) and h[5] == 4680 and h[9:11] == (-1, -1)
        elif f & 4:
            assert h[1] >= 0 and h[2] >= 0 and h[9:11] == h[1:3]
    none = ST.make_batch(rng, [(30, []), (1, []), (7, []), (9, [])], contig_offsets=TABLE)      # no record at all
    got, want = _exact(env, none)
    assert want["totals"].tolist()[0::2] == [4, 4]
    empty = ST.make_batch(rng, [], contig_offsets=TABLE)             # N == 0
    got = BU.call(env.lib, env.ix, empty)
    assert got["record_offsets"].tolist() == [0] and got["totals"].tolist() == [0, 0, 0] and got["data"].size == 0


def test_field_values(env):
    rng = np.random.default_rng(166)
    far = 2147483000
    reads = [(20, [dict(ops=[op(20, EQ)], contig=0, offset=far + 300, strand=0, mapq=60, score=-5, nm=-1)]),
             (20, [dict(ops=[op(20, EQ)], contig=0, offset=far, strand=1)]),                    # a negative TLEN
             (20, [dict(ops=[op(20, EQ)], contig=0, offset=40)]), (20, [dict(ops=[op(20, EQ)], contig=2, offset=50, strand=1)]),
             (20, [dict(ops=[op(9, EQ), op(2, I), op(9, EQ)], contig=1, offset=4000, strand=1),
                   dict(ops=[op(20, EQ)], contig=2, offset=1, kind=2, strand=1)]),
             (20, [dict(ops=[op(20, EQ)], contig=1, offset=3800)])]
    b = ST.make_batch(rng, reads, contig_offsets=TABLE)
    got, want = _exact(env, b, NO_MD)                                # MD off: the far positions are not the reference's
    heads = [_head(got["data"], int(s)) for s in got["record_offsets"][:-1]]
    assert heads[0][2] == far + 299 and heads[0][10] == far - 1 and heads[0][11] == -320 and heads[1][11] == 320
    assert (heads[2][1], heads[2][9]) == (0, 2) and (heads[3][1], heads[3][9]) == (2, 0)        # mates on different contigs
    assert heads[4][1] == heads[4][9] == 1 and (heads[5][1], heads[5][9]) == (2, 1)             # a secondary on another contig
    raw = bytes(got["data"][:int(got["record_offsets"][1])])
    assert b"NMi" + struct.pack("<i", -1) + b"ASi" + struct.pack("<i", -5) in raw


def test_every_tag_subset_and_mode(env):
    rng = np.random.default_rng(167)
    counts = rng.integers(0, 4, 30).tolist()
    reads = [(max(n, 1), recs) for n, recs in ST.random_reads(rng, counts, TABLE, max_ops=70)]
    b = ST.make_batch(rng, reads, contig_offsets=TABLE)
    sizes = []
    for tags in range(32):
        got, want = _exact(env, b, tags, decode=tags in (0, 5, 31))
        sizes.append(int(want["totals"][1]))
    assert all(sizes[t | bit] > sizes[t] for t in range(32) for bit in (1, 2, 4, 8, 16) if not t & bit)      # every tag adds bytes
    for variant in (dict(b, quals=None), dict(b, contig_offsets=None, contig_names=[b"chr"]), dict(b, sam=None)):
        _exact(env, variant)
        _exact(env, variant, ST.NM, ST.NO_SEQ)
    odd = ST.make_batch(rng, [(max(n, 1), recs) for n, recs in ST.random_reads(rng, [2, 0, 1], TABLE)], contig_offsets=TABLE, single=True)
    got, want = _exact(env, odd)                                     # N odd: single-end only
    assert b"MCZ" not in bytes(want["data"]) and want["totals"].tolist()[0::2] == [4, 1]
    BU.call(env.lib, env.ix, dict(odd, sam=np.zeros((3, 4), np.int32)), want_rc=ST.INVALID)


def test_pos_at_the_bin_boundaries(env):
    rng = np.random.default_rng(168)
    reads, want_bins = [], []
    first = {14: 4681, 17: 585, 20: 73, 23: 9, 26: 1}
    for shift in (14, 17, 20, 23, 26):
        edge = 1 << shift
        reads.append((100, [dict(ops=[op(100, EQ)], contig=0, offset=edge - 99)]))                          # [edge - 100, edge)
        reads.append((100, [dict(ops=[op(60, EQ), op(1, D), op(40, X)], contig=0, offset=edge - 99, strand=1)]))      # ... one more
        want_bins += [(4681 + ((edge - 100) >> 14)) & 0xffff, 0 if shift == 26 else first[shift + 3] + ((edge - 100) >> (shift + 3))]
    reads += [(10, [dict(ops=[], contig=0, offset=0)]), (10, [dict(ops=[op(3, S), op(1, I)], contig=0, offset=(1 << 14) + 1)])]
    want_bins += [4680, 4682]
    b = ST.make_batch(rng, reads, contig_offsets=TABLE)
    got, want = _exact(env, b, NO_MD)
    assert [_head(got["data"], int(s))[5] for s in got["record_offsets"][:-1]] == want_bins


def test_capacity_and_n_records(env):
    rng = np.random.default_rng(169)
    counts = [2, 1, 0, 3, 1, 1, 0, 0, 2, 2]
    b = ST.make_batch(rng, ST.random_reads(rng, counts, TABLE), contig_offsets=TABLE)
    full = BU.host_bam_records(b, env.T, ALL)
    total, off = int(full["totals"][1]), full["record_offsets"]
    k = next(i for i in range(off.size - 1) if _head(full["data"], int(off[i]))[8] >= 4)      # a record with some SEQ
    h = _head(full["data"], int(off[k]))
    in_seq = int(off[k]) + 36 + h[3] + 4 * h[6] + 1
    # nothing, a cut through the first head, through a later head, through a SEQ, half, one byte short, exact, room to spare
    for cap in (0, 17, int(off[k]) + 35, in_seq, total // 2, total - 1, total, total + 50):
        got, want = _exact(env, b, cap_data=cap)
        assert got["record_offsets"][-1] == total                    # the true total even when cap_data is smaller
    for n_records in (sum(counts) - 1, 4, 0):                        # R cuts a read's records, then everything
        got, want = _exact(env, b, n_records=n_records)
        assert want["totals"][0] == n_records + sum(1 for k in range(len(counts)) if sum(counts[:k]) >= n_records or counts[k] == 0)
    for key, bad in (("read_offsets", b["read_offsets"][::-1].copy()), ("sel_offsets", -b["sel_offsets"]),
                     ("cigar_offsets", b["cigar_offsets"] + 1), ("read_offsets", b["read_offsets"] + 1)):
        BU.call(env.lib, env.ix, dict(b, **{key: bad}), want_rc=ST.INVALID)


def test_more_records_than_one_grid_of_waves(env):
    import torch
    rng = np.random.default_rng(170)
    waves = 8 * 4 * torch.cuda.get_device_properties(0).multi_processor_count      # eight blocks of four waves per CU
    n = (waves * 5 // 4 + 100) & ~1
    assert n < 30000
    counts = rng.integers(0, 3, n).tolist()
    reads = []
    for c in counts:
        recs = [dict(ops=[op(int(rng.integers(1, 30)), EQ), op(1, X), op(int(rng.integers(1, 30)), EQ)], contig=int(rng.integers(0, 3)),
                     offset=int(rng.integers(1, 4000)), strand=int(rng.integers(0, 2)), kind=0 if i == 0 else 2) for i in range(c)]
        reads.append((int(rng.integers(0, 40)), recs))
    b = ST.make_batch(rng, reads, contig_offsets=TABLE)
    got, want = _exact(env, b, decode=False)
    assert want["totals"][0] > waves and want["totals"][2] > n // 4


# ------------------------------------------------------------------ through the pipeline
def _text(q):
    return "".join("ACGT"[c] for c in q)


def test_map_pairs_rescue_to_bam_and_file(env, tmp_path):
    g, T = env.g, env.T.copy()
    T[9000:9300] = T[2000:2300]                                     # the planted duplication of tests/test_pair_gpu.py
    table = np.asarray([0, 6000, 12000, N_REF], np.int64)
    m = g.ExactMatch("bam_records_planted.fa")
    m.set_reference(_text(T))
    sm, rs = g.SMEM(m, 4), g.ReferenceSet(["a", "b", "c"], table, T)

    def diverged(piece, every=13):
        q = np.asarray(piece, np.uint8).copy()
        q[every - 1::every] = (q[every - 1::every] + 1) % 4
        return q
    gap = np.concatenate([T[3600:3660], T[3663:3750]])             # a deletion of three bases
    reads = [T[3000:3150].copy(), AU.revcomp(T[3250:3400]), T[500:650].copy(), AU.revcomp(diverged(T[750:900])),
             T[13000:13150].copy(), np.random.default_rng(94).integers(0, 4, 150).astype(np.uint8),
             T[2050:2200].copy(), AU.revcomp(T[9400:9550]), gap, AU.revcomp(T[3900:4050])]
    strs = [_text(q) for q in reads]
    names = [f"pair{r // 2}" for r in range(len(strs))]
    quals = ["".join(chr(33 + (7 * r + i) % 60) for i in range(len(s))) for r, s in enumerate(strs)]
    out = sm.map_pairs(strs, 19, rs, rescue=True)
    so = _np(out[1])
    assert 0 in np.diff(so).tolist() and 2 in np.diff(so).tolist()   # an unmapped mate, and one with two records
    for tags in (ST.NM | ST.AS, ALL):
        text = bytes(_np(sm.sam_text(out, strs, names, quals=quals, contigs=rs, tags=tags)[0])).decode().split("\n")
        data, off, totals = sm.bam_records(out, strs, names, quals=quals, contigs=rs, tags=tags)
        assert text[-1] == "" and BU.bam_to_sam(_np(data), rs.names) == text[:-1]
        assert _np(totals).tolist() == [len(text) - 1, data.numel(), int((np.diff(so) == 0).sum())] and _np(off)[-1] == data.numel()
    # the file: BGZF blocks that gzip reads, the header, then the device's bytes
    path = tmp_path / "out.bam"
    totals = sm.write_bam(str(path), out, strs, names, quals=quals, contigs=rs, tags=ALL)
    raw = gzip.decompress(path.read_bytes())
    header = g.bam_header(rs.names, np.diff(table))
    assert raw[:len(header)] == header and raw[len(header):] == bytes(_np(data)) and int(totals[0]) == len(text) - 1
    assert path.read_bytes()[-28:] == g.index.BGZF_EOF
    single = sm.map_records(strs, 19, rs)                           # single-end: map_records' five results
    sdata = _np(sm.bam_records(single, strs, names, contigs=rs, tags=ST.NM | ST.MD)[0])
    stext = bytes(_np(sm.sam_text(single, strs, names, contigs=rs, tags=ST.NM | ST.MD)[0])).decode().split("\n")[:-1]
    assert BU.bam_to_sam(sdata, rs.names) == stext
