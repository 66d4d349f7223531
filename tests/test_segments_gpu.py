"""GPU tests of the segment calls (run with -m gpu on an MI355X): genie_reference_segments and genie_segment_coords, and
ReferenceSet.from_fasta(..., ambiguous="cut") end to end.  Every comparison is exact, against tests/segment_util.py (one
plain loop over the positions, checked on the host by tests/test_segments_host.py): the tile and lane edges of the 4096-byte
tiles at three alignments of the codes, record boundaries with and without breaks on them, empty records, bad tables and
small capacities on guarded buffers, a reference beyond 2^31 given bytes, and both lookups of genie_segment_coords."""
import numpy as np
import pytest

import contig_util as CU
import guarded
import segment_util as SU

pytestmark = pytest.mark.gpu

OK, INVALID, CAPACITY = SU.OK, SU.INVALID, SU.CAPACITY
TILE = SU.TILE


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


# ------------------------------------------------------------------ tile and lane edges
@pytest.mark.parametrize("name", list(SU.patterns(1)))
def test_tile_and_lane_edges(lib, name):
    """One record.  With the codes at an address that is `lead` modulo 16 the tiles' edges lie `lead` bytes earlier."""
    most = 0
    for n in SU.EDGE_SIZES:
        codes = SU.patterns(n)[name]
        want = SU.cut(codes)
        for lead in (0, 1, 15):
            size = SU.segments_call(lib, codes, None, sizing=True, lead=lead)["out4"]
            assert size == [len(want[2]), len(want[0]), want[4], 0], (n, lead)      # the sizing call agrees
            SU.same_as_cut(SU.segments_call(lib, codes, None, size[1], size[0], lead=lead), want)
        most = max(most, len(want[2]))
    if name == "alternating":
        n = SU.EDGE_SIZES[-1]
        assert most == (n + 1) // 2                                 # cap_segs = (n + 1) / 2 is met exactly
        assert SU.segments_call(lib, SU.patterns(n)[name], None, n, (n + 1) // 2)["out4"][0] == (n + 1) // 2
    if name == "spanning":
        assert SU.cut(SU.patterns(SU.EDGE_SIZES[-1])[name])[4] == 3 * TILE + 3      # the longest segment closes across four tiles


@pytest.mark.parametrize("brk", SU.BREAKS)
def test_every_break_value(lib, brk):
    n = TILE + 1
    for name in ("at4095", "alternating", "one_per_tile"):
        codes = SU.patterns(n, brk)[name]
        assert (codes == brk).any()
        SU.same_as_cut(SU.segments_call(lib, codes), SU.cut(codes))


# ------------------------------------------------------------------ record boundaries
@pytest.mark.parametrize("name", list(SU.record_cases()))
def test_record_boundaries(lib, name):
    codes, off = SU.record_cases()[name]
    want = SU.cut(codes, off)
    for lead in (0, 7):
        SU.same_as_cut(SU.segments_call(lib, codes, off, lead=lead), want)
    if name == "touching":
        assert want[1].tolist() == [0, 100, len(codes)]             # two segments that touch in d_bases
    if name == "null_table":
        same = SU.cut(*SU.record_cases()["one_record"])
        assert all(np.array_equal(a, b) for a, b in zip(want[:4], same[:4]))


def test_every_byte_a_start(lib):
    """A record boundary on every byte and no break: TILE starts in every full tile, the most a tile can hold."""
    n = 2 * TILE + 5
    codes = np.random.default_rng(41).integers(0, 4, n).astype(np.uint8)
    off = list(range(n + 1))
    want = SU.cut(codes, off)
    assert len(want[2]) == n and want[4] == 1
    for lead in (0, 5):
        SU.same_as_cut(SU.segments_call(lib, codes, off, lead=lead), want)


@pytest.mark.parametrize("density,seed", SU.RANDOM)
def test_random_references(lib, pkg, density, seed):
    codes, off = SU.random_case(density, seed)
    want = SU.cut(codes, off)
    assert len(want[2]) > 700
    SU.same_as_cut(SU.segments_call(lib, codes, off), want)
    # the Python wrapper makes the same two calls
    got = pkg.reference_segments(codes, off)
    assert all(np.array_equal(g.cpu().numpy(), w) and g.cpu().numpy().dtype == w.dtype for g, w in zip(got[:4], want[:4])) and got[4] == want[4]
    # ... and every kept position maps back to where it stood
    if seed == SU.RANDOM[0][1]:
        ix = pkg.GenieIndex.build(want[0], 0).to("cuda")
        n = len(want[0])
        pos = np.arange(1, n + 1)
        back = SU.coords_call(lib, ix, want[1], want[2], want[3], SU.POSITIONS, pos, 1)
        given = off[back[:, 0]] + back[:, 1] - 1
        assert np.array_equal(given, np.flatnonzero(codes <= 3))
        s = np.searchsorted(want[1], pos - 1, side="right") - 1
        hits = np.stack([s, pos - want[1][s]], 1).astype(np.int32)
        assert np.array_equal(SU.coords_call(lib, ix, want[1], want[2], want[3], SU.HITS, hits, 2), back)


# ------------------------------------------------------------------ call behaviour
def test_small_capacities_and_bad_tables_on_guarded_buffers(lib):
    import torch
    codes, off = SU.record_cases()["tile_edges_holes"]
    n, nrec = len(codes), len(off) - 1
    want = SU.cut(codes, off)
    S, kept = len(want[2]), len(want[0])
    far = [0, 2**40, 2**40 + 5, n + 2**40, n + 2**40, n + 2**40]
    tables = [(off, S, kept, OK, 0), (off, S - 1, kept, CAPACITY, 0), (off, S, kept - 1, CAPACITY, 0), (off, 0, 0, CAPACITY, 0),
              ([3] + off[1:], S, kept, INVALID, 1), (off[:2] + [off[1] - 1] + off[3:], S, kept, INVALID, 2),
              (off[:-1] + [n - 1], S, kept, INVALID, 4), (off[:-1] + [n + 1], S, kept, INVALID, 4),
              (far, S, kept, INVALID, 4), ([2**40] * (nrec + 1), S, kept, INVALID, 1 | 4), ([n, 0] * 3, S, kept, INVALID, 1 | 2 | 4)]
    s = torch.cuda.current_stream().cuda_stream
    for poison in guarded.POISONS:
        for table, cap_segs, cap_bases, want_rc, mask in tables:
            a = guarded.Arena("cuda", poison, capacity=1 << 20)
            rc, out4 = SU.guarded_segments(lib, a, s, codes, table, nrec, cap_bases, cap_segs)
            torch.cuda.synchronize()
            assert rc == want_rc and out4[3] == mask, (table[:3], cap_segs, cap_bases, rc, out4)
            a.check()
            a.check_frozen()
            bufs = {b[0]: a.mem[b[2]:b[3]] for b in a.bufs}
            if want_rc != INVALID:
                assert out4 == [S, kept, want[4], 0]                    # the true values, whatever the capacities
            if want_rc == OK:
                assert np.array_equal(guarded.as_numpy(bufs["bases"], np.uint8), want[0])
                assert np.array_equal(guarded.as_numpy(bufs["seg_offsets"], np.int64), want[1])
                assert np.array_equal(guarded.as_numpy(bufs["seg_record"], np.int32), want[2])
                assert np.array_equal(guarded.as_numpy(bufs["seg_origin"], np.int64), want[3])
            else:                                                       # a failed call stores nothing
                assert all(a.holds_poison(bufs[k]) for k in ("bases", "seg_offsets", "seg_record", "seg_origin"))


# ------------------------------------------------------------------ 64 bits
def test_beyond_two_to_the_31_given_bytes(lib, pkg):
    import ctypes as C
    import torch
    n = 2**31 + 2**20
    starts = [0, 2**30 + 77, 2**30 + 2**29 + 4095, 2**31 - 500, n - 1000]
    rng = np.random.default_rng(31)
    islands = [rng.integers(0, 4, 1000).astype(np.uint8) for _ in starts]
    codes = torch.full((n,), 4, dtype=torch.uint8, device="cuda")
    for at, isl in zip(starts, islands):
        codes[at:at + 1000] = torch.from_numpy(isl).cuda()
    kept = np.concatenate(islands)
    ix = pkg.GenieIndex.build(kept, 0).to("cuda")
    # three records; in the first table the last record holds four islands (origins above 2^31), in the second an inner
    # boundary lies above 2^31
    for off in ([0, 1000, 5000, n], [0, 2**29, 2**31 + 2**19, n]):
        rec = np.searchsorted(off, starts, side="right") - 1
        origin = np.asarray(starts, np.int64) - np.asarray(off, np.int64)[rec]
        bases, so, sr, sg, longest = pkg.reference_segments(codes, np.asarray(off, np.int64))
        assert longest == 1000 and bases.numel() == 5000 and sr.numel() == 5       # n_kept and n_seg
        assert np.array_equal(bases.cpu().numpy(), kept)
        assert so.cpu().tolist() == [0, 1000, 2000, 3000, 4000, 5000]
        assert sr.cpu().tolist() == rec.tolist() and sg.cpu().tolist() == origin.tolist()
        pos = np.asarray([4001, 4500, 5000, 3001, 3501, 1, 0, 5001], np.int32)
        got = SU.coords_call(lib, ix, so.cpu().numpy(), sr.cpu().numpy(), sg.cpu().numpy(), SU.POSITIONS, pos, 1)
        want = SU.coords_expected(so.cpu().numpy(), sr.cpu().numpy(), sg.cpu().numpy(), pos)
        assert np.array_equal(got, want) and want[6:].tolist() == [[-1, -1]] * 2
    assert origin[4] == 2**20 - 1000 - 2**19 and rec.tolist() == [0, 1, 1, 1, 2]
    # the first table again, by hand: the last island's offsets lie above 2^31
    off = [0, 1000, 5000, n]
    bases, so, sr, sg, _ = pkg.reference_segments(codes, np.asarray(off, np.int64))
    assert sg.cpu().tolist()[4] == n - 1000 - 5000 > 2**31
    got = SU.coords_call(lib, ix, so.cpu().numpy(), sr.cpu().numpy(), sg.cpu().numpy(), SU.POSITIONS, [4001, 5000], 1)
    assert got.tolist() == [[2, n - 1000 - 5000 + 1], [2, n - 5000]] and got[0, 1] > 2**31
    # one record, the NULL table: the sizing call alone
    out4 = (C.c_int64 * 4)()
    tb = lib.genie_reference_segments_tmp_bytes(n, 1)
    tmp = torch.empty(tb, dtype=torch.uint8, device="cuda")
    assert lib.genie_reference_segments(codes.data_ptr(), n, None, 1, None, 0, None, None, None, 0, out4, tmp.data_ptr(), tb,
                                        torch.cuda.current_stream().cuda_stream) == OK
    assert list(out4) == [5, 5000, 1000, 0]


# ------------------------------------------------------------------ genie_segment_coords
def _reference_of_segments(n_segs, seed):
    """Given codes with exactly n_segs segments of 1 to 5 bases in 7 records, break runs of 1 to 3 between them."""
    rng = np.random.default_rng(seed)
    parts = []
    for _ in range(n_segs):
        parts += [rng.integers(0, 4, rng.integers(1, 6)).astype(np.uint8), np.full(rng.integers(1, 4), 4, np.uint8)]
    codes = np.concatenate(parts)
    cuts = np.flatnonzero(codes > 3)                                # a boundary on a break adds no segment
    off = np.concatenate([[0], np.sort(rng.choice(cuts, min(6, cuts.size), replace=False)), [codes.size]]).astype(np.int64)
    return codes, off


@pytest.mark.parametrize("n_segs", [1, 1023, 1024, 20000])
def test_segment_coords_both_forms(lib, pkg, n_segs):
    """1023 segments are answered from LDS alone, 1024 take the second level with shift 1, 20 000 with shift 5."""
    codes, off = _reference_of_segments(n_segs, n_segs)
    bases, so, sr, sg, _ = SU.cut(codes, off)
    assert len(sr) == n_segs
    ix = pkg.GenieIndex.build(bases, 0).to("cuda")
    n = len(bases)
    rng = np.random.default_rng(5)
    pos = np.concatenate([[0, n + 1, -1, -2**31, 2**31 - 1, 1, n], rng.integers(1, n + 1, 3000)]).astype(np.int32)
    if n_segs <= 1024:
        pos = np.concatenate([pos, np.arange(1, n + 1, dtype=np.int32)])
    want = SU.coords_expected(so, sr, sg, pos)
    assert want[:5].tolist() == [[-1, -1]] * 5 and (want[5:] >= 0).all()
    assert np.array_equal(SU.coords_call(lib, ix, so, sr, sg, SU.POSITIONS, pos, 1), want)
    rows = np.full((pos.size, 4), 12345, np.int32)                  # MEM rows: the position is column 2
    rows[:, 2] = pos
    assert np.array_equal(SU.coords_call(lib, ix, so, sr, sg, SU.POSITIONS, rows.reshape(-1)[2:], 4, pos.size), want)
    s = rng.integers(0, n_segs, 3000)
    lens = so[s + 1] - so[s]
    hits = np.stack([s, rng.integers(1, lens + 1)], 1)
    hits = np.concatenate([[[n_segs, 1], [-1, 1], [0, 0], [0, so[1] + 1], [n_segs - 1, 0], [n_segs - 1, so[-1] - so[-2] + 1],
                            [0, 1], [n_segs - 1, so[-1] - so[-2]]], hits]).astype(np.int32)
    want = SU.hit_coords_expected(so, sr, sg, hits)
    assert want[:6].tolist() == [[-1, -1]] * 6 and (want[6:] >= 0).all()
    assert np.array_equal(SU.coords_call(lib, ix, so, sr, sg, SU.HITS, hits, 2), want)
    # the Python layer
    rs = pkg.SegmentedReferenceSet([str(i) for i in range(len(off) - 1)], off, bases, so, sr, sg)
    assert np.array_equal(rs.coords(pos, index=ix).cpu().numpy(), SU.coords_expected(so, sr, sg, pos))
    assert np.array_equal(rs.hit_coords(hits, index=ix).cpu().numpy(), want)
    assert np.array_equal(ix.segment_coords(rs, rows.reshape(-1)[2:], "positions", 4).cpu().numpy(), SU.coords_expected(so, sr, sg, pos))


# ------------------------------------------------------------------ end to end
def test_from_fasta_cut_end_to_end(pkg):
    import torch
    strings, names, text, reads = SU.e2e_case()
    host = pkg.ReferenceSet.from_sequences(strings, names, ambiguous="cut")
    rs = pkg.ReferenceSet.from_fasta(text, ambiguous="cut")
    assert isinstance(rs, pkg.SegmentedReferenceSet) and rs.names == host.names == names and len(rs) == 3
    assert isinstance(rs.codes, torch.Tensor) and rs.codes.device.type == "cuda"
    assert np.array_equal(rs.codes.cpu().numpy(), host.codes) and rs.n == host.n and rs.n_given == host.n_given
    for field in ("record_offsets", "offsets", "seg_record", "seg_origin"):
        a, b = getattr(rs, field), getattr(host, field)
        assert a.dtype == b.dtype and np.array_equal(a, b), field
    assert rs.n_segments == host.n_segments >= len(SU.E2E_RUNS) + 1
    with pytest.raises(ValueError, match="chrA"):                   # the default still refuses the text
        pkg.ReferenceSet.from_fasta(text)
    with pytest.raises(ValueError):
        pkg.ReferenceSet.from_fasta(b">a\nNNNN\n>b\n\n", ambiguous="cut")
    ix = rs.build_index(0)
    flags = CU.BOTH | CU.SPLIT
    bases = np.concatenate(reads)
    offs = np.arange(0, 120 * len(reads) + 1, 120, dtype=np.int64)
    w_off, w_rows, w_st, w_skip = CU.expected(host.codes, host.offsets, reads, flags, SU.E2E_M)
    off, rows, st, skipped = ix.find_mems_contigs(rs, bases, offs, SU.E2E_M, both_strands=True, split_breaks=True)
    off, rows = off.cpu().numpy(), rows.cpu().numpy()
    assert np.array_equal(off, w_off) and np.array_equal(st.cpu().numpy(), w_st) and skipped == w_skip
    assert rows.shape == w_rows.shape and np.array_equal(rows, w_rows)
    # every row, over its whole length, reads the given record's letters: no row touches an N
    at = rs.coords(rows[:, 2]).cpu().numpy()
    assert at.dtype == np.int64 and np.array_equal(at, SU.coords_expected(host.offsets, host.seg_record, host.seg_origin, rows[:, 2]))
    strand_reads = CU.MS.strand_reads(reads, 2)
    for q in range(len(strand_reads)):
        for (p, e, _, _), (rec, o) in zip(rows[off[q]:off[q + 1]].tolist(), at[off[q]:off[q + 1]].tolist()):
            letters = strings[rec][o - 1:o - 1 + e - p].upper()
            assert len(letters) == e - p and letters == "".join("ACGT"[c] for c in strand_reads[q][p:e])
    # SMEMs against the set of segments, and their hits in given coordinates
    s_off, s_rows, s_st, _ = ix.find_smems_contigs(rs, "bwa", bases, offs, SU.E2E_M, both_strands=True, split_breaks=True)
    s_rows = s_rows.cpu().numpy()
    assert s_rows.shape[0] >= 72
    h_off, hits, dropped = ix.locate_contigs(rs, s_rows)
    w_hoff, w_hits, w_dropped = CU.locate_expected(host.codes, host.offsets, s_rows)
    assert np.array_equal(h_off.cpu().numpy(), w_hoff) and np.array_equal(hits.cpu().numpy(), w_hits) and dropped == w_dropped
    assert (np.diff(w_hoff) >= 1).all()                             # every row has a hit inside one segment
    named = rs.hit_coords(hits).cpu().numpy()
    assert np.array_equal(named, SU.hit_coords_expected(host.offsets, host.seg_record, host.seg_origin, w_hits))
    s_strand = np.searchsorted(s_off.cpu().numpy(), np.arange(s_rows.shape[0]), side="right") - 1
    for k in range(s_rows.shape[0]):
        p, e = s_rows[k, :2].tolist()
        want = "".join("ACGT"[c] for c in strand_reads[s_strand[k]][p:e])
        for rec, o in named[w_hoff[k]:w_hoff[k + 1]].tolist():
            assert strings[rec][o - 1:o - 1 + e - p].upper() == want
