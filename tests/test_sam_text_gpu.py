"""GPU: genie_sam_text against the brute force of tests/sam_text_util.py, every byte and every line offset exactly equal, on a
16 kb random reference with three contigs.  Synthetic records, pairing rows, ops and names exercise the call without the
pipeline in front of it: op counts on both sides of the wave's 64 lanes and far beyond, op lengths of one to nine digits, read
and name lengths around 64, reads without records at every place, a 10-digit POS, mates on different contigs, code 4 on strand
1, MD runs across the reference's 32-base words and a contig's first and last base, every tag subset, no qualities, no SEQ, no
contig table, single-end mode, a text capacity below the total, and more lines than one grid of waves.  Then the pipeline:
SMEM.sam_text on map_pairs(rescue=True) equals sam_lines line for line, MD rebuilds the contig's bases from SEQ and CIGAR, and a
FASTQ text goes through reads_from_text, fastq_fields and sam_text."""
import re

import numpy as np
import pytest

import align_util as AU
import sam_text_util as ST

pytestmark = pytest.mark.gpu

N_REF = 1 << 14
TABLE = np.asarray([0, 6000, 11000, N_REF], np.int64)
ALL = ST.NM | ST.AS | ST.MD | ST.MC | ST.MQ
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
    return e


def _exact(env, b, tags=ALL, flags=0, **kw):
    want = ST.expected(b, env.T, tags, flags, kw.get("n_records"))
    got = ST.call(env.lib, env.ix, b, tags, flags, **kw)
    ST.agrees(got, want, kw.get("cap_text"))
    return got, want


def _dense_ops(rng, n_ops):
    """n_ops ops that cover little of the reference: = runs of 1 to 3 bases with X, I and D of 1 or 2 between them."""
    return [op(int(rng.integers(1, 4)), EQ) if i % 2 == 0 else op(int(rng.integers(1, 3)), int(rng.choice([X, X, D, I]))) for i in range(n_ops)]


def test_op_counts_and_lengths(env):
    rng = np.random.default_rng(61)
    reads = []
    for n_ops in (0, 1, 63, 64, 65, 130, 3001):
        ops = _dense_ops(rng, n_ops)
        mate = _dense_ops(rng, 130 if n_ops == 64 else 2)
        reads.append((ST.query_length(ops), [dict(ops=ops, contig=1, offset=17, strand=n_ops & 1)]))
        reads.append((40, [dict(ops=mate, contig=1, offset=300, strand=1), dict(ops=_dense_ops(rng, 65), contig=2, offset=9, kind=1)]))
    # lengths of one to nine digits; the long ones on = and S, behind the ops that load the reference
    digits = [op(7, S), op(3, EQ), op(2, X), op(12, D), op(10, EQ), op(1, I)] + [op(10**k + k, EQ) for k in range(1, 8)]
    digits += [op(2**28 - 1, EQ), op(123456789, EQ), op(2**28 - 1, S)]
    reads.append((50, [dict(ops=digits, contig=0, offset=5)]))
    reads.append((50, [dict(ops=[op(100000000, S), op(999999999 >> 2, EQ)], contig=0, offset=900, strand=1)]))
    b = ST.make_batch(rng, reads, contig_offsets=TABLE)
    got, want = _exact(env, b)
    text = bytes(want["text"]).decode()
    assert f"{2**28 - 1}=123456789={2**28 - 1}S" in text and "MC:Z:100000000S" in text and text.count("MD:Z:") == 22
    assert max(np.diff(b["cigar_offsets"])) == 3001 and int(np.diff(want["line_offsets"]).max()) > 12000
    _exact(env, b, ST.MD)
    _exact(env, b, ST.MC | ST.NM, ST.NO_SEQ)


def test_read_and_name_lengths_and_code_4_on_strand_1(env):
    rng = np.random.default_rng(62)
    reads, names = [], []
    for k, length in enumerate((0, 1, 63, 64, 65, 300, 5000)):
        reads.append((length, [dict(ops=[op(max(length, 1), EQ)], contig=k % 3, offset=1 + k, strand=0),
                               dict(ops=[op(4, S), op(9, EQ)], contig=2, offset=77, strand=1, kind=1)]))
        reads.append((length, [] if k % 2 else [dict(ops=[op(5, EQ), op(1, X)], contig=k % 3, offset=200, strand=1)]))
        names += [b"n" * (1, 64, 65, 300)[k % 4]] * 2
    b = ST.make_batch(rng, reads, names=names, contig_offsets=TABLE, code4=0.2)
    assert (b["bases"] == 4).sum() > 500
    got, want = _exact(env, b)
    lines = bytes(want["text"]).decode().split("\n")
    assert sum("N" in ln.split("\t")[9] for ln in lines[:-1]) >= 8 and any(ln.startswith("n" * 300 + "\t") for ln in lines)
    assert any(ln.split("\t")[9] == "" for ln in lines[:-1])           # a read of no bases: an empty SEQ, as sam_lines writes it
    _exact(env, dict(b, quals=None))
    _exact(env, b, ALL, ST.NO_SEQ)


def test_reads_without_records_everywhere(env):
    rng = np.random.default_rng(63)
    counts = [0, 2, 0, 0, 1, 1, 3, 0, 0, 0, 2, 2, 1, 0]             # at the start, at the end, two in a row, both mates of a pair
    b = ST.make_batch(rng, ST.random_reads(rng, counts, TABLE), contig_offsets=TABLE)
    got, want = _exact(env, b)
    assert want["totals"].tolist()[0::2] == [sum(counts) + counts.count(0), counts.count(0)]
    flags = [int(ln.split("\t")[1]) for ln in bytes(want["text"]).decode().split("\n")[:-1]]
    assert sum(f & 4 > 0 for f in flags) == 7 and sum(f & 12 == 12 for f in flags) == 4 and sum(f & 12 == 4 for f in flags) == 3
    none = ST.make_batch(rng, [(30, []), (0, []), (7, []), (9, [])], contig_offsets=TABLE)      # no record at all
    got, want = _exact(env, none)
    assert want["totals"].tolist()[0::2] == [4, 4] and b"\t77\t*\t0\t0\t*\t*\t0\t0\t" in bytes(want["text"])
    empty = ST.make_batch(rng, [], contig_offsets=TABLE)             # N == 0
    got = ST.call(env.lib, env.ix, empty)
    assert got["line_offsets"].tolist() == [0] and got["totals"].tolist() == [0, 0, 0] and got["text"].size == 0


def test_field_values(env):
    rng = np.random.default_rng(64)
    far = 2147483000
    reads = [(20, [dict(ops=[op(20, EQ)], contig=0, offset=far + 300, strand=0, mapq=60, score=-5, nm=-1)]),
             (20, [dict(ops=[op(20, EQ)], contig=0, offset=far, strand=1)]),                    # a 10-digit POS, a negative TLEN
             (20, [dict(ops=[op(20, EQ)], contig=0, offset=40)]), (20, [dict(ops=[op(20, EQ)], contig=2, offset=50, strand=1)]),
             (20, [dict(ops=[op(9, EQ), op(2, I), op(9, EQ)], contig=1, offset=4000, strand=1),
                   dict(ops=[op(20, EQ)], contig=2, offset=1, kind=2, strand=1)]),
             (20, [dict(ops=[op(20, EQ)], contig=1, offset=3800)])]
    b = ST.make_batch(rng, reads, contig_offsets=TABLE)
    got, want = _exact(env, b)
    rows = [ln.split("\t") for ln in bytes(want["text"]).decode().split("\n")[:-1]]
    assert rows[0][3] == str(far + 300) and rows[0][7] == str(far) and rows[0][8] == "-320" and rows[1][8] == "320"
    assert rows[0][11:13] == ["NM:i:-1", "AS:i:-5"]
    assert rows[2][6] == "c" and rows[3][6] == "a" and rows[2][8] == "0"      # mates on different contigs
    assert rows[4][6] == "=" and rows[5][6] == "b" and rows[6][6] == "="      # a secondary on another contig than the mate


def test_md_across_reference_words_and_contig_ends(env):
    rng = np.random.default_rng(65)
    T = env.T
    recs = [dict(ops=[op(2, EQ), op(1, X), op(1, X), op(2, X), op(20, EQ)], contig=0, offset=29),        # X at 30, 31, 32 and 33
            dict(ops=[op(3, EQ), op(5, D), op(3, EQ)], contig=0, offset=59),                             # D over 61 .. 65
            dict(ops=[op(40, X)], contig=0, offset=40),                                                  # one X op over 39 .. 78
            dict(ops=[op(70, D), op(1, EQ)], contig=0, offset=1),                                        # one D op over 0 .. 69
            dict(ops=[op(1, X), op(10, EQ)], contig=1, offset=1),                                        # a contig's first base
            dict(ops=[op(10, EQ), op(1, X)], contig=1, offset=4990),                                     # ... and its last
            dict(ops=[op(1, D), op(9, EQ)], contig=2, offset=1),
            dict(ops=[op(8, EQ), op(2, D)], contig=2, offset=N_REF - 11000 - 9)]                         # the reference's last base
    reads = [(20, [dict(q, kind=0 if i == 0 else 2) for i, q in enumerate(recs)]), (20, [])]
    b = ST.make_batch(rng, reads, contig_offsets=TABLE)
    got, want = _exact(env, b)
    md = [re.search(r"MD:Z:(\S+)", ln).group(1) for ln in bytes(got["text"]).decode().split("\n")[:len(recs)]]
    L = lambda lo, hi: "".join("ACGT"[c] for c in T[lo:hi])      # noqa: E731
    assert md[0] == f"2{L(30, 31)}0{L(31, 32)}0{L(32, 33)}0{L(33, 34)}20" and md[1] == f"3^{L(61, 66)}3"
    assert md[2] == "0" + "0".join(L(39, 79)) + "0" and md[3] == f"0^{L(0, 70)}1"
    assert md[4] == f"0{L(6000, 6001)}10" and md[5] == f"10{L(10999, 11000)}0"
    assert md[6] == f"0^{L(11000, 11001)}9" and md[7] == f"8^{L(N_REF - 2, N_REF)}0"
    # without a table the offsets count from the reference's start
    flat = dict(b, contig_offsets=None, contig_names=[b"whole"])
    got, want = _exact(env, flat)
    assert f"MD:Z:0{L(0, 1)}10".encode() in bytes(got["text"]) and b"\twhole\t4990\t" in bytes(got["text"])


def test_every_tag_subset_and_mode(env):
    rng = np.random.default_rng(66)
    counts = rng.integers(0, 4, 30).tolist()
    b = ST.make_batch(rng, ST.random_reads(rng, counts, TABLE, max_ops=70), contig_offsets=TABLE)
    sizes = []
    for tags in range(32):
        got, want = _exact(env, b, tags)
        sizes.append(int(want["totals"][1]))
    assert all(sizes[t | bit] > sizes[t] for t in range(32) for bit in (1, 2, 4, 8, 16) if not t & bit)      # every tag adds bytes
    for variant in (dict(b, quals=None), dict(b, contig_offsets=None, contig_names=[b"chr"]), dict(b, sam=None)):
        _exact(env, variant)
        _exact(env, variant, ST.NM, ST.NO_SEQ)
    odd = ST.make_batch(rng, ST.random_reads(rng, [2, 0, 1], TABLE), contig_offsets=TABLE, single=True)      # N odd: single-end only
    got, want = _exact(env, odd)
    assert b"MC:Z" not in bytes(want["text"]) and want["totals"].tolist()[0::2] == [4, 1]
    ST.call(env.lib, env.ix, dict(odd, sam=np.zeros((3, 4), np.int32)), want_rc=ST.INVALID)


def test_capacity_and_n_records(env):
    rng = np.random.default_rng(67)
    counts = [2, 1, 0, 3, 1, 1, 0, 0, 2, 2]
    b = ST.make_batch(rng, ST.random_reads(rng, counts, TABLE), contig_offsets=TABLE)
    total = int(ST.expected(b, env.T, ALL)["totals"][1])
    for cap in (0, 1, 63, 64, 65, total // 2, total - 1, total + 50):
        got, want = _exact(env, b, cap_text=cap)
        assert got["line_offsets"][-1] == total                      # the true total even when cap_text is smaller
    for n_records in (sum(counts) - 1, 4, 0):                        # R cuts a read's records, then everything
        got, want = _exact(env, b, n_records=n_records)
        assert want["totals"][0] == n_records + sum(1 for k in range(len(counts)) if sum(counts[:k]) >= n_records or counts[k] == 0)
    for key, bad in (("read_offsets", b["read_offsets"][::-1].copy()), ("sel_offsets", -b["sel_offsets"]),
                     ("cigar_offsets", b["cigar_offsets"] + 1), ("read_offsets", b["read_offsets"] + 1)):
        ST.call(env.lib, env.ix, dict(b, **{key: bad}), want_rc=ST.INVALID)


def test_more_lines_than_one_grid_of_waves(env):
    import torch
    rng = np.random.default_rng(68)
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
    got, want = _exact(env, b)
    assert want["totals"][0] > waves and want["totals"][2] > n // 4


# ------------------------------------------------------------------ through the pipeline
def _text(q):
    return "".join("ACGT"[c] for c in q)


def _np(t):
    import torch
    return (t.view(torch.int32) if t.dtype == torch.uint32 else t).cpu().numpy()


def _rebuild(seq, cigar, md):
    """The reference segment of an alignment from SEQ, CIGAR and MD alone."""
    aligned, at = [], 0                                              # the read's bases over =, X (and None per deleted base)
    for n, o in re.findall(r"(\d+)([IDS=X])", cigar):
        n = int(n)
        if o in "=X":
            aligned += list(seq[at:at + n])
        if o == "D":
            aligned += [None] * n
        if o != "D":
            at += n
    out, k = [], 0
    for count, dele, sub in re.findall(r"(\d+)|\^([ACGT]+)|([ACGT])", md):
        if count:
            out += aligned[k:k + int(count)]
            k += int(count)
        else:
            out += list(dele or sub)
            k += len(dele or sub)
    assert k == len(aligned) and None not in out
    return "".join(out)


def test_map_pairs_rescue_to_text(env):
    g, T = env.g, env.T.copy()
    T[9000:9300] = T[2000:2300]                                     # the planted duplication of tests/test_pair_gpu.py
    table = np.asarray([0, 6000, 12000, N_REF], np.int64)
    m = g.ExactMatch("sam_text_planted.fa")
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
    want = g.sam_lines(out[0], out[6], out[4], out[2], out[3], names, rs.names, strs, quals)
    text, line_offsets, totals = sm.sam_text(out, strs, names, quals=quals, contigs=rs)
    assert bytes(_np(text)).decode() == "\n".join(want) + "\n"
    assert totals.tolist() == [len(want), text.numel(), int((np.diff(so) == 0).sum())]
    lo = _np(line_offsets)
    assert lo.size == len(want) + 1 and [bytes(_np(text)[lo[i]:lo[i + 1]]).decode() for i in range(len(want))] == [w + "\n" for w in want]
    # MD against the reference: SEQ, CIGAR and MD rebuild the contig's bases
    full = bytes(_np(sm.sam_text(out, strs, names, quals=quals, contigs=rs, tags=ALL)[0])).decode().split("\n")[:-1]
    seen_x = seen_d = 0
    for ln, plain in zip(full, want):
        cols = ln.split("\t")
        assert "\t".join(cols[:len(plain.split("\t"))]) == plain      # the columns, NM and AS stay what they were
        if int(cols[1]) & 4:
            assert not any(c.startswith(("NM", "AS", "MD")) for c in cols[11:])
            continue
        tags = dict(c.split(":", 2)[::2] for c in cols[11:])
        start = int(table[rs.names.index(cols[2])]) + int(cols[3]) - 1
        ref = _rebuild(cols[9], cols[5], tags["MD"])
        assert ref == _text(T[start:start + len(ref)])
        seen_x += "X" in cols[5]
        seen_d += "^" in tags["MD"]
        if not int(cols[1]) & 8:
            assert re.fullmatch(r"(\d+[IDS=X])+", tags["MC"]) and 0 <= int(tags["MQ"]) <= 60
    assert seen_x >= 1 and seen_d >= 1
    # single-end: map_records' five results
    single = sm.map_records(strs, 19, rs)
    stext = bytes(_np(sm.sam_text(single, strs, names, contigs=rs, tags=ST.NM | ST.MD)[0])).decode().split("\n")[:-1]
    assert len(stext) == _np(single[0]).shape[0] + int((np.diff(_np(single[1])) == 0).sum()) and all("\tMC:" not in s for s in stext)
    # a FASTQ text: reads_from_text, fastq_fields, sam_text
    fastq = "".join(f"@pair{r // 2} mate/{r % 2 + 1}\n{s}\n+\n{q}\n" for r, (s, q) in enumerate(zip(strs, quals))).encode()
    bases, read_offsets, _ = g.text_reads.reads_from_text(fastq, "fastq")
    nm, no, qs = g.text_reads.fastq_fields(fastq, read_offsets)
    again = sm.map_pairs((bases, read_offsets), 19, rs, rescue=True)
    t2 = sm.sam_text(again, (bases, read_offsets), (nm, no), quals=qs, contigs=rs)[0]
    assert bytes(_np(t2)).decode() == "\n".join(want) + "\n"


def test_write_sam(env, tmp_path):
    g = env.g
    m = g.ExactMatch("sam_text_plain.fa")
    m.set_reference(_text(env.T))
    sm, rs = g.SMEM(m, 4), g.ReferenceSet(["a", "b", "c"], TABLE, env.T)
    strs = [_text(env.T[100:250]), _text(AU.revcomp(env.T[400:550])), _text(env.T[7000:7100]), "ACGT" * 10]
    out = sm.map_pairs(strs, 19, rs)
    path = tmp_path / "out.sam"
    totals = sm.write_sam(str(path), out, strs, ["x", "x", "y", "y"], contigs=rs, tags=ALL)
    lines = path.read_text().split("\n")
    assert lines[-1] == "" and lines[:5] == g.sam_header(rs.names, np.diff(TABLE)) and len(lines) - 6 == int(totals[0])
    assert lines[5].split("\t")[:4] == ["x", "99", "a", "101"] and lines[5].split("\t")[13] == "MD:Z:150"
