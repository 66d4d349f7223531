"""GPU tests of the contig calls (run with -m gpu on an MI355X): genie_contigs_validate, genie_find_mems_contigs,
genie_locate_contigs and genie_contig_coords on references of several sequences.  Every comparison is exact, against the
brute force of tests/contig_util.py on its shared cases (checked against each other on the host by
tests/test_contigs_host.py): contigs of 0, 1, m - 1, m and m + 1 bases, empty first and last contigs, bridging reads, seed
intervals of more than 32 rows, the three seed paths, and tables of 1 to 30000 contigs (coords and locate answer up to
1023 from LDS, the MEM walks up to 12287; more take the second level of the lookup)."""
import numpy as np
import pytest

import contig_util as CU
import lookup_util as U
import match_stats_util as MS
import mems_util as MM

pytestmark = pytest.mark.gpu

BOTH, SPLIT, FLAGS = CU.BOTH, CU.SPLIT, CU.FLAGS
CASES = list(CU.cases())
_IX = {}


@pytest.fixture(scope="module")
def pkg():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import genie_smem_amd as g
    g._native.lib()
    return g


def _index(pkg, name):
    c = CU.case(name)
    key = (U._bytes(c.ref), c.dir_bits)
    if key not in _IX:
        _IX[key] = pkg.GenieIndex.build(c.ref, 0, dir_bits=c.dir_bits).to("cuda")
    return _IX[key]


def _check(pkg, ix, c, flags, m, tag, max_occ=0):
    """The sizing call and the call with exactly that room against the restated specification -> the call's four outputs."""
    bases, offs = MS.csr(c.reads)
    got = CU.sized_call(pkg._native.lib(), ix, c.off, flags, bases, offs, m, max_occ)
    w_off, w_rows, w_st, w_skip = CU.expected(c.ref, c.off, c.reads, flags, m, max_occ)
    off, rows, st, tt = got
    assert np.array_equal(st, w_st), (tag, "status")
    assert np.array_equal(off, w_off), (tag, "offsets", np.flatnonzero(off != w_off)[:5])
    assert rows.shape == w_rows.shape and np.array_equal(rows, w_rows), (tag, "rows", np.flatnonzero((rows != w_rows).any(1))[:5])
    assert tt.tolist() == [w_rows.shape[0], w_skip], (tag, "totals")
    return got


# ------------------------------------------------------------------ genie_find_mems_contigs
@pytest.mark.parametrize("name", CASES)
def test_every_contig_mem_against_brute_force(pkg, name):
    c = CU.case(name)
    ix = _index(pkg, name)
    most = 0
    for flags in FLAGS:
        most = max(most, _check(pkg, ix, c, flags, c.m, (name, flags))[1].shape[0])
    assert most > (150 if name.startswith("wave") else 8)


def test_one_contig_is_find_mems_byte_for_byte(pkg):
    lib = pkg._native.lib()
    c = CU.case("table1")
    assert c.off.tolist() == [0, len(c.ref)]
    ix = _index(pkg, "table1")
    bases, offs = MS.csr(c.reads + MS.break_reads(c.ref)[2:6])
    for flags in FLAGS:
        for m, occ in ((5, 0), (5, 3), (12, 0), (45, 0)):
            got = CU.sized_call(lib, ix, c.off, flags, bases, offs, m, occ)
            want = MM.sized_call(lib, ix, flags, bases, offs, m, occ)
            for x, y in zip(got, want):
                assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (flags, m, occ)
    assert want[1].shape[0] > 0


def test_union_over_per_contig_indexes(pkg):
    """Property (b): the (start, end, pos) triples are those of genie_find_mems on an index of every contig alone, pos
    shifted by the contig's offset."""
    lib = pkg._native.lib()
    c = CU.case("table5")
    ix = _index(pkg, "table5")
    assert c.n_contigs == 5 and (np.diff(c.off) > 0).all()
    bases, offs = MS.csr(c.reads)
    alone = [pkg.GenieIndex.build(c.ref[a:b], 0, dir_bits=7).to("cuda") for a, b in zip(c.off[:-1], c.off[1:])]
    for flags in (0, BOTH):
        off, rows, _, _ = CU.sized_call(lib, ix, c.off, flags, bases, offs, c.m)
        parts = [MM.sized_call(lib, one, flags, bases, offs, c.m)[:2] for one in alone]
        for q in range(len(off) - 1):
            want = set()
            for k, (o, r) in enumerate(parts):
                want |= {(s, e, p + int(c.off[k])) for s, e, p, _ in r[o[q]:o[q + 1]].tolist()}
            have = [tuple(x) for x in rows[off[q]:off[q + 1], :3].tolist()]
            assert len(have) == len(set(have)) and set(have) == want, (flags, q)
        assert rows.shape[0] >= 4                                   # the four clean reads are cut from the reference: a row each


def test_rows_past_the_capacity_are_dropped(pkg):
    lib = pkg._native.lib()
    c = CU.case("wave20")
    ix = _index(pkg, "wave20")
    bases, offs = MS.csr(c.reads)
    for flags in (0, BOTH | SPLIT):
        w_off, w_rows, w_st, _ = CU.expected(c.ref, c.off, c.reads, flags, c.m)
        total = w_rows.shape[0]
        inside = total // 2
        assert total > 100 and w_rows[inside - 1, 0] == w_rows[inside, 0]       # cut in the middle of a position's rows
        for cap in (0, 1, inside, total - 1, total, total + 5):
            off, rows, st, tt = CU.call(lib, ix, c.off, flags, bases, offs, c.m, cap=cap, spare=70, fill=-9)
            held = min(cap, total)
            assert np.array_equal(off, w_off) and off[-1] == total and tt[0] == total, cap      # the true total
            assert np.array_equal(rows[:held], w_rows[:held]), cap
            assert (rows[held:] == -9).all(), cap


@pytest.mark.parametrize("name,occ,skips", [("wave20", 40, True), ("wave20", 41, False), ("wave5", 40, True), ("edges5", 2, True)])
def test_max_occ_counts_occurrences_in_the_concatenation(pkg, name, occ, skips):
    c = CU.case(name)
    ix = _index(pkg, name)
    for flags in (0, BOTH | SPLIT):
        tt = _check(pkg, ix, c, flags, c.m, (name, occ, flags), max_occ=occ)[3]
        # 41 copies: a seed of the unit occurs 41 times, bridging occurrences and those without room included
        assert (tt[1] > 0) == skips, (name, occ, tt)


def test_no_reads_and_empty_reads(pkg):
    lib = pkg._native.lib()
    c = CU.case("edges12")
    ix = _index(pkg, "edges12")
    for flags in FLAGS:
        strands = 2 if flags & BOTH else 1
        off, rows, st, tt = CU.call(lib, ix, c.off, flags, np.zeros(0, np.uint8), [0], 5, cap=4, fill=-9)
        assert off.tolist() == [0] and tt.tolist() == [0, 0] and st.size == 0 and (rows == -9).all()
        off, rows, st, tt = CU.call(lib, ix, c.off, flags, np.zeros(0, np.uint8), [0, 0, 0], 1, cap=4, fill=-9)
        assert off.tolist() == [0] * (2 * strands + 1) and st.tolist() == [0] * (2 * strands) and tt.tolist() == [0, 0]


# ------------------------------------------------------------------ genie_locate_contigs
def _smem_rows(ix, c, flags, m):
    bases, offs = MS.csr(c.reads)
    _, rows, _ = ix.find_smems_long("bwa", bases, offs, m, both_strands=bool(flags & BOTH), split_breaks=bool(flags & SPLIT))
    return rows.cpu().numpy()


@pytest.mark.parametrize("name", ["edges12", "edges5", "wave20", "table65", "table1500"])
def test_locate_contigs_against_brute_force(pkg, name):
    lib = pkg._native.lib()
    c = CU.case(name)
    ix = _index(pkg, name)
    n, sa = len(c.ref), U.suffix_rows(c.ref)
    bridge = c.bridge
    lo, hi = U.interval(c.ref, sa, bridge)
    assert lo >= 0                                                  # a pattern all of whose occurrences bridge two contigs
    extra = np.asarray([[0, len(bridge), lo, hi], [0, 0, 0, n], [3, 9, -1, -1], [0, 4, 7, 6], [2, 2, 0, 0]], np.int32)
    seen = 0
    for flags in (0, BOTH | SPLIT):
        rows = np.concatenate([_smem_rows(ix, c, flags, 3), extra]).astype(np.int32)
        w_off, w_hits, w_drop = CU.locate_expected(c.ref, c.off, rows)
        S, k = rows.shape[0], rows.shape[0] - 5
        assert w_off[k + 1] == w_off[k] and w_off[k + 2] - w_off[k + 1] == n and w_off[-1] == w_off[k + 2] and w_drop > 0
        off0, none, tt0 = CU.locate_call(lib, ix, c.off, rows, hits=False)      # the sizing call
        assert none is None and np.array_equal(off0, w_off) and tt0.tolist() == [w_hits.shape[0], w_drop]
        total = w_hits.shape[0]
        for cap in (total, total // 2, 1, total + 3):
            off, hits, tt = CU.locate_call(lib, ix, c.off, rows, cap=cap, spare=40, fill=-9, totals=cap != 1)
            held = min(cap, total)
            assert np.array_equal(off, w_off) and (tt is None or tt.tolist() == [total, w_drop]), cap
            assert np.array_equal(hits[:held], w_hits[:held]) and (hits[held:] == -9).all(), cap
        seen += total
        if name == "wave20":
            assert (rows[:, 3] - rows[:, 2] >= 32).any()              # the whole-wave path
    assert seen > 100
    off, hits, tt = CU.locate_call(lib, ix, c.off, np.zeros((0, 4), np.int32), cap=2, fill=-9)
    assert off.tolist() == [0] and tt.tolist() == [0, 0] and (hits == -9).all()


# ------------------------------------------------------------------ genie_contig_coords
@pytest.mark.parametrize("name", ["edges12", "table1", "table1023", "table1024", "table1500", "table2600", "table30000"])
def test_contig_coords_of_every_position(pkg, name):
    lib = pkg._native.lib()
    c = CU.case(name)
    ix = _index(pkg, name)
    n = len(c.ref)
    pos = np.arange(0, n + 2, dtype=np.int32)
    want = CU.coords_expected(c.off, n, pos)
    assert want[0].tolist() == [-1, -1] and want[-1].tolist() == [-1, -1] and (want[1:-1] >= 0).all()
    assert np.array_equal(CU.coords_call(lib, ix, c.off, pos), want)
    wide = np.full((pos.size, 4), -77, np.int32)
    wide[:, 0] = pos
    assert np.array_equal(CU.coords_call(lib, ix, c.off, wide.reshape(-1)[:-3], stride=4), want)
    assert CU.coords_call(lib, ix, c.off, np.asarray([-5, 2**31 - 1, -2**31], np.int32)).tolist() == [[-1, -1]] * 3
    assert CU.coords_call(lib, ix, c.off, np.zeros(0, np.int32)).shape == (0, 2)


# ------------------------------------------------------------------ genie_contigs_validate, and tables it refuses
def _bad_tables(c):
    n, off = len(c.ref), c.off
    first, order, last = off.copy(), off.copy(), off.copy()
    first[0] = 1
    mid = len(off) // 2
    order[mid] = order[mid + 1] + 1
    last[-1] = n + 1
    return {"first": first, "order": order, "last": last}


@pytest.mark.parametrize("name", ["edges12", "table3", "table2600"])
def test_validate_accepts_and_refuses(pkg, name):
    lib = pkg._native.lib()
    c = CU.case(name)
    ix = _index(pkg, name)
    assert CU.validate(lib, ix, c.off) == CU.OK
    for what, off in _bad_tables(c).items():
        assert CU.validate(lib, ix, off) == CU.INVALID, what
    short = c.off.copy()
    short[-1] -= 1
    assert CU.validate(lib, ix, short) == CU.INVALID
    assert CU.validate(lib, ix, c.off) == CU.OK                     # and the next call is fine


@pytest.mark.parametrize("name", ["edges12", "table3", "table2600", "table30000"])
def test_refused_tables_stay_inside_their_buffers(pkg, name):
    """The hot calls do not repeat the check: on a table that genie_contigs_validate refuses the values are undefined, and
    every load and store stays inside the declared sizes.  Outputs, scratch and the table itself are cut from a guarded
    arena; every guard holds its poison afterwards and the inputs are unchanged."""
    import torch
    from guarded import Arena
    lib = pkg._native.lib()
    c = CU.case(name)
    ix = _index(pkg, name)
    n, nc = len(c.ref), c.n_contigs
    rng = np.random.default_rng(nc)
    tables = dict(_bad_tables(c))
    tables["huge"] = np.full(nc + 1, 2**62, np.int64)
    tables["negative"] = -c.off - 1
    tables["noise"] = rng.integers(-2**40, 2**40, nc + 1)
    tables["reversed"] = c.off[::-1].copy()
    tables["zeros"] = np.zeros(nc + 1, np.int64)
    smem = np.concatenate([_smem_rows(ix, c, 0, 3), [[0, 0, 0, n], [0, 5, 0, 2**31 - 1], [0, -3, 2, 40]]]).astype(np.int32)
    pos = np.arange(0, n + 2, dtype=np.int32)
    stream = torch.cuda.Stream()
    for what, off in tables.items():
        assert CU.validate(lib, ix, off) == CU.INVALID, what
        a = Arena("cuda", 0x5A)
        a.freeze(ix.blob, "index image")
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            rcs = CU.guarded_calls(lib, ix, a, stream.cuda_stream, off, BOTH | SPLIT, c.reads, c.m, 64, smem, 64, pos)
        torch.cuda.synchronize()
        assert rcs == [0, 0, 0], (what, rcs)
        a.check()
        a.check_frozen()
    _check(pkg, ix, c, 0, c.m, (name, "after the refused tables"))  # and the next call is fine


# ------------------------------------------------------------------ the Python layer
def test_python_layer_from_fasta_to_coords(pkg):
    c = CU.case("edges12")
    seqs = ["".join("ACGT"[b] for b in c.ref[a:e]) for a, e in zip(c.off[:-1], c.off[1:])]
    names = [f"ctg{i}" for i in range(len(seqs))]
    text = b""
    for i, (name, s) in enumerate(zip(names, seqs)):
        s = s.lower() if i == 3 else s
        text += b">" + name.encode() + b" some description\r\n" + b"".join(s[k:k + 60].encode() + b"\r\n" for k in range(0, len(s), 60))
    rs = pkg.ReferenceSet.from_fasta(text)
    host = pkg.ReferenceSet.from_sequences(seqs, names)
    assert rs.names == host.names == names and np.array_equal(rs.offsets, host.offsets) and np.array_equal(rs.offsets, c.off)
    assert rs.codes.is_cuda and np.array_equal(rs.codes.cpu().numpy(), host.codes) and np.array_equal(host.codes, c.ref)
    bases, offs = MS.csr(c.reads)
    results = []
    for ref_set in (rs, host):
        ix = ref_set.build_index(0)
        assert ref_set.index is ix and ix.n == len(c.ref)
        for both, split in ((False, False), (True, True)):
            flags = (BOTH if both else 0) | (SPLIT if split else 0)
            want = CU.expected(c.ref, c.off, c.reads, flags, c.m)
            off, rows, st, skipped = ix.find_mems_contigs(ref_set, bases, offs, c.m, both, split, rows_hint=3 if both else None)
            assert skipped == 0 and all(np.array_equal(x.cpu().numpy(), y) for x, y in zip((off, rows, st), want))
            results.append(rows)
        where = ref_set.coords(rows[:, 2].contiguous()).cpu().numpy()
        assert np.array_equal(where, CU.coords_expected(c.off, len(c.ref), want[1][:, 2]))
        assert np.array_equal(ix.contig_coords(ref_set, rows.reshape(-1)[2:], stride=4).cpu().numpy(), where)
        assert ref_set.name_of(where[0, 0]) == names[where[0, 0]]
        smem = ix.find_smems_long("bwa", bases, offs, 3)[1]
        ho, hits, dropped = ix.locate_contigs(ref_set, smem)
        w = CU.locate_expected(c.ref, c.off, smem.cpu().numpy())
        assert np.array_equal(ho.cpu().numpy(), w[0]) and np.array_equal(hits.cpu().numpy(), w[1]) and dropped == w[2] > 0
    assert np.array_equal(results[0].cpu().numpy(), results[2].cpu().numpy())
    with pytest.raises(ValueError, match="ctgN"):
        pkg.ReferenceSet.from_fasta(b">ok\nACGT\n>ctgN\nACGNT\n")
    with pytest.raises(ValueError):
        ix.find_mems_contigs(pkg.ReferenceSet.from_sequences(["ACGT"]), bases, offs, c.m)      # the table of another reference


def test_smem_wrapper(pkg):
    c = CU.case("table3")
    seqs = ["".join("ACGT"[b] for b in c.ref[a:e]) for a, e in zip(c.off[:-1], c.off[1:])]
    rs = pkg.ReferenceSet.from_sequences(seqs)
    m = pkg.ExactMatch("contigs.fa")
    m.set_reference("".join(seqs))
    sm = pkg.SMEM(m, 4)
    reads = c.reads[:4]                                             # the clean ones: strings of A, C, G and T
    strs = ["".join("ACGT"[b] for b in r) for r in reads]
    want = CU.expected(c.ref, c.off, reads, BOTH, c.m)
    for given in (strs, MS.csr(reads)):
        off, rows, st, skipped = sm.find_mems_contigs(rs, given, c.m, both_strands=True)
        assert skipped == 0 and all(np.array_equal(x.cpu().numpy(), y) for x, y in zip((off, rows, st), want))
    smem = sm.matcher.index(sm.lut.lut_size).find_smems_long("bwa", *MS.csr(reads), 3)[1]
    ho, hits, dropped = sm.locate_contigs(rs, smem)
    w = CU.locate_expected(c.ref, c.off, smem.cpu().numpy())
    assert np.array_equal(ho.cpu().numpy(), w[0]) and np.array_equal(hits.cpu().numpy(), w[1]) and dropped == w[2]
