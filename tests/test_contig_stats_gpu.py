"""GPU tests of genie_match_stats_contigs and genie_find_smems_contigs (run with -m gpu on an MI355X).  Every comparison
is exact and over every read, against the brute force of tests/contig_stats_util.py on its shared cases (checked on the host
by tests/test_contig_stats_host.py): every case of contig_util.cases() (edge, wave and table cases, up to 30000 contigs: the
two-level lookup, in wave5_2600 and wave5_13000 under intervals of more than 32 rows, the whole-wave walk), reads across
every boundary with and without a second copy of the match, tandem references in contigs of 3 to 50
bases (whole-wave walks where no row, or only the last, lies inside a contig), run starts on either side of a window
boundary, a flagged run over three windows, unit passes, one contig against the parents byte for byte, the consequences for
genie_locate_contigs and genie_find_mems_contigs, the LUT and RMI modes, the sizing call, and the memory contract."""
import numpy as np
import pytest

import contig_stats_util as CS
import contig_util as CU
import lookup_util as U
import match_stats_util as MS
import smem_util as SM

pytestmark = pytest.mark.gpu

BOTH, SPLIT, FLAGS = CS.BOTH, CS.SPLIT, CS.FLAGS
CASES = list(CS.cases())
_IX = {}


@pytest.fixture(scope="module")
def pkg():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import genie_smem_amd as g
    g._native.lib()
    return g


def _index(pkg, c, K=0):
    key = (U._bytes(c.ref), c.dir_bits, K)
    if key not in _IX:
        ix = pkg.GenieIndex.build(c.ref, K, dir_bits=c.dir_bits)
        if K:
            ix.train_rmi([16])
        _IX[key] = ix.to("cuda")
    return _IX[key]


def _check_ms(lib, ix, c, flags, tag, **kw):
    bases, offs = MS.csr(c.reads)
    ms, lohi, st, clipped = CS.ms_call(lib, ix, c.off, flags, bases, offs, **kw)
    w_ms, w_lohi, w_st, w_clip = CS.expected_ms(c.ref, c.off, c.reads, flags)
    assert np.array_equal(ms, w_ms), (tag, "ms", np.flatnonzero(ms != w_ms)[:5])
    if lohi is not None:
        assert np.array_equal(lohi, w_lohi), (tag, "lohi", np.flatnonzero((lohi != w_lohi).any(1))[:5])
    if st is not None:
        assert np.array_equal(st, w_st), (tag, "status")
    if clipped is not None:
        assert clipped == w_clip, (tag, "clipped", clipped, w_clip)
    return ms


def _check_smems(lib, ix, c, flags, tag, mode="bwa", min_len=1, K=0, **kw):
    bases, offs = MS.csr(c.reads)
    off, rows, st, clipped = CS.sized_smem_call(lib, ix, c.off, flags, bases, offs, {"bwa": 0, "lut": 1, "rmi": 2}[mode], min_len, **kw)
    w_off, w_rows, w_st, w_clip = CS.expected_smems(c.ref, c.off, c.reads, flags, mode, min_len, K)
    if st is not None:
        assert np.array_equal(st, w_st), (tag, "status")
    assert np.array_equal(off, w_off), (tag, "offsets", np.flatnonzero(off != w_off)[:5])
    assert rows.shape == w_rows.shape and np.array_equal(rows, w_rows), (tag, "rows", np.flatnonzero((rows != w_rows).any(1))[:5])
    if clipped is not None:
        assert clipped == w_clip, (tag, "clipped", clipped, w_clip)
    return rows


@pytest.mark.parametrize("name", CASES)
def test_every_case_against_brute_force(pkg, name):
    """All four flag combinations; intervals on and off, d_status and d_totals null and not."""
    lib = pkg._native.lib()
    c = CS.case(name)
    ix = _index(pkg, c)
    for flags in FLAGS:
        _check_ms(lib, ix, c, flags, (name, flags))
        _check_smems(lib, ix, c, flags, (name, flags))
    _check_ms(lib, ix, c, BOTH, (name, "no intervals"), intervals=False, status=False, totals=False)
    _check_ms(lib, ix, c, SPLIT, (name, "no status"), status=False)
    _check_smems(lib, ix, c, BOTH | SPLIT, (name, "no status, no totals"), status=False, totals=False)
    _check_smems(lib, ix, c, 0, (name, "min_len"), min_len=25, totals=False)


def test_one_contig_is_the_parents_byte_for_byte(pkg):
    lib = pkg._native.lib()
    ref = U.family()["rand4096"][:3000]
    ix = pkg.GenieIndex.build(ref, 0).to("cuda")
    one = np.asarray([0, len(ref)], np.int64)
    for reads in (MS.window_reads(ref), MS.break_reads(ref)):
        bases, offs = MS.csr(reads)
        for flags in FLAGS:
            ms, lohi, st, clipped = CS.ms_call(lib, ix, one, flags, bases, offs)
            p_ms, p_lohi, p_st = MS.call(lib, ix, flags, bases, offs)
            assert ms.tobytes() == p_ms.tobytes() and lohi.tobytes() == p_lohi.tobytes() and st.tobytes() == p_st.tobytes()
            assert clipped == 0
            off, rows, st, clipped = CS.sized_smem_call(lib, ix, one, flags, bases, offs)
            p_off, p_rows, p_st = ix.find_smems_long("bwa", bases, offs, both_strands=bool(flags & BOTH), split_breaks=bool(flags & SPLIT))
            assert off.tobytes() == p_off.cpu().numpy().tobytes() and rows.tobytes() == p_rows.cpu().numpy().tobytes()
            assert st.tobytes() == p_st.cpu().numpy().tobytes() and clipped == 0


def test_every_row_has_a_hit_and_the_concatenation_loses_seeds(pkg):
    c = CS.case("junction")
    rs = pkg.ReferenceSet([str(i) for i in range(c.n_contigs)], c.off, c.ref)
    ix = _index(pkg, c)
    bases, offs = MS.csr(c.reads)
    for flags in (0, BOTH | SPLIT):
        kw = dict(both_strands=bool(flags & BOTH), split_breaks=bool(flags & SPLIT))
        _, rows, _, clipped = ix.find_smems_contigs(rs, "bwa", bases, offs, **kw)
        ho, _, dropped = ix.locate_contigs(rs, rows)
        assert clipped > 0 and rows.shape[0] > 0 and int(ho.diff().min().item()) >= 1
        _, plain, _ = ix.find_smems_long("bwa", bases, offs, **kw)
        ho, _, _ = ix.locate_contigs(rs, plain)
        assert int(ho.diff().min().item()) == 0                    # a row of the concatenation with no hit at all


@pytest.mark.parametrize("name,m", [("junction", 12), ("ctg_wave20", 20), ("tandem3", 8)])
def test_longest_contig_mem_from_a_position_is_ms_c(pkg, name, m):
    c = CS.case(name)
    rs = pkg.ReferenceSet([str(i) for i in range(c.n_contigs)], c.off, c.ref)
    ix = _index(pkg, c)
    bases, offs = MS.csr(c.reads)
    for flags in (0, BOTH | SPLIT):
        kw = dict(both_strands=bool(flags & BOTH), split_breaks=bool(flags & SPLIT))
        ms = ix.match_stats_contigs(rs, bases, offs, **kw)[0].cpu().numpy()
        moff, mems, _, _ = ix.find_mems_contigs(rs, bases, offs, m, **kw)
        moff, mems = moff.cpu().numpy(), mems.cpu().numpy()
        strands = 2 if flags & BOTH else 1
        checked = 0
        for q, read in enumerate(MS.strand_reads(c.reads, strands)):
            i, s = divmod(q, strands)
            v0 = strands * int(offs[i]) + s * len(read)
            rows = mems[moff[q]:moff[q + 1]]
            longest = np.zeros(len(read), np.int64)
            np.maximum.at(longest, rows[:, 0], rows[:, 1] - rows[:, 0])
            want = ms[v0:v0 + len(read)]
            # Rows start where an occurrence is left-maximal.  At a run start of fwd_c one of the longest contig-exact
            # match is: were all of them extendable to the left, ms_c of the position in front would be one more.
            fwd_c = want.astype(np.int64) + np.arange(len(read))
            at = (want >= m) & np.concatenate([[True], fwd_c[1:] != fwd_c[:-1]])
            assert np.array_equal(longest[at], want[at]), (name, flags, q)
            assert (longest <= np.maximum(want, 0)).all(), (name, flags, q)       # and no row anywhere is longer than ms_c
            checked += int(at.sum())
        assert checked > 0


@pytest.mark.parametrize("mode", ["lut", "rmi"])
def test_lut_and_rmi_modes_with_reads_shorter_than_k(pkg, mode):
    lib = pkg._native.lib()
    c = CS.case("short")
    K = 12
    ix = _index(pkg, c, K)
    for flags in (0, BOTH):
        rows = _check_smems(lib, ix, c, flags, (mode, flags), mode=mode, K=K)
        assert rows.shape[0] > 0
    st = CS.expected_smems(c.ref, c.off, c.reads, 0, mode, 1, K)[2]
    assert (st == SM.READ_TOO_SHORT).any() and (st == SM.READ_OK).any()


def test_a_capacity_that_is_too_small(pkg):
    lib = pkg._native.lib()
    c = CS.case("junction")
    ix = _index(pkg, c)
    bases, offs = MS.csr(c.reads)
    for flags in (0, BOTH | SPLIT):
        w_off, w_rows, _, w_clip = CS.expected_smems(c.ref, c.off, c.reads, flags)
        cap = w_rows.shape[0] // 2
        off, rows, _, clipped = CS.smem_call(lib, ix, c.off, flags, bases, offs, cap=cap, spare=3)
        assert np.array_equal(off, w_off) and clipped == w_clip                 # the true totals
        assert np.array_equal(rows[:cap], w_rows[:cap]) and (rows[cap:] == -7).all()


def test_no_reads_and_empty_reads(pkg):
    lib = pkg._native.lib()
    c = CS.case("junction")
    ix = _index(pkg, c)
    for flags in FLAGS:
        strands = 2 if flags & BOTH else 1
        ms, lohi, st, clipped = CS.ms_call(lib, ix, c.off, flags, np.zeros(0, np.uint8), np.zeros(1, np.int64))
        assert ms.size == 0 and st.size == 0 and clipped == 0
        off, rows, st, clipped = CS.smem_call(lib, ix, c.off, flags, np.zeros(0, np.uint8), np.zeros(1, np.int64), cap=4)
        assert off.tolist() == [0] and (rows == -7).all() and clipped == 0
        off, rows, st, clipped = CS.smem_call(lib, ix, c.off, flags, np.zeros(0, np.uint8), np.zeros(4, np.int64), cap=4)
        assert off.tolist() == [0] * (3 * strands + 1) and (rows == -7).all() and clipped == 0 and not st.any()


@pytest.mark.parametrize("name", ["junction", "ctg_table2600"])
def test_memory_contract_and_refused_tables(pkg, name):
    """Buffers of exactly the declared bytes under three poisons give the same, expected, outputs and leave every guard, the
    inputs and the index image alone; on eight tables that genie_contigs_validate refuses the calls return, the values are
    undefined, and nothing outside the buffers is touched."""
    import torch
    from guarded import POISONS, Arena
    lib = pkg._native.lib()
    c = CS.case(name)
    ix = _index(pkg, c)
    flags = BOTH | SPLIT
    want_ms = CS.expected_ms(c.ref, c.off, c.reads, flags, lead=5, tail=3)
    want_sm = CS.expected_smems(c.ref, c.off, c.reads, flags)
    cap = want_sm[1].shape[0] + 7
    stream = torch.cuda.Stream()

    def run(off, poison):
        a = Arena("cuda", poison)
        a.freeze(ix.blob, "index image")
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            rcs, collect = CS.guarded_calls(lib, ix, a, stream.cuda_stream, off, flags, c.reads, cap)
        torch.cuda.synchronize()
        assert rcs == [0, 0], rcs
        a.check()
        a.check_frozen()
        return collect

    for poison in POISONS:
        got = run(c.off, poison)()
        assert np.array_equal(got["ms"], want_ms[0]) and np.array_equal(got["lohi"], want_ms[1]), poison
        assert np.array_equal(got["ms_status"], want_ms[2]) and got["ms_totals"].tolist() == [want_ms[3]], poison
        assert np.array_equal(got["offsets"], want_sm[0]) and np.array_equal(got["rows"], want_sm[1]), poison
        assert np.array_equal(got["status"], want_sm[2]) and got["totals"].tolist() == [want_sm[3]], poison
    for what, off in CS.bad_tables(c).items():
        assert CU.validate(lib, ix, off) == CU.INVALID, what
        run(off, 0x5A)
    _check_ms(lib, ix, c, 0, (name, "after the refused tables"))    # and the next call is fine


def test_smem_wrapper_with_strings_and_a_rerun(pkg):
    """SMEM.match_stats_contigs / find_smems_contigs on list[str] and on (bases, read_offsets); a rows_hint that is too small
    makes find_smems_contigs run twice, and `clipped` counts once."""
    c = CS.case("junction")
    seqs = ["".join("ACGT"[b] for b in c.ref[a:e]) for a, e in zip(c.off[:-1], c.off[1:])]
    rs = pkg.ReferenceSet.from_sequences(seqs)
    assert np.array_equal(rs.offsets, c.off)
    m = pkg.ExactMatch("contig_stats.fa")
    m.set_reference("".join(seqs))
    sm = pkg.SMEM(m, 4)
    reads = c.reads
    strs = ["".join("ACGT"[b] for b in r) for r in reads]
    w_ms = CS.expected_ms(c.ref, c.off, reads, BOTH)
    w_sm = CS.expected_smems(c.ref, c.off, reads, BOTH, min_len=5)
    assert w_ms[3] > 0 and w_sm[1].shape[0] > 3
    for given in (strs, MS.csr(reads)):
        ms, lohi, st, clipped = sm.match_stats_contigs(rs, given, both_strands=True)
        assert clipped == w_ms[3] and all(np.array_equal(x.cpu().numpy(), y) for x, y in zip((ms, lohi, st), w_ms))
        off, rows, st, clipped = sm.find_smems_contigs(rs, given, 5, both_strands=True)
        assert clipped == w_sm[3] and all(np.array_equal(x.cpu().numpy(), y) for x, y in zip((off, rows, st), w_sm))
    ix = sm.matcher.index(sm.lut.lut_size)
    off, rows, st, clipped = ix.find_smems_contigs(rs, "bwa", *MS.csr(reads), 5, rows_hint=2, both_strands=True)
    assert clipped == w_sm[3] and all(np.array_equal(x.cpu().numpy(), y) for x, y in zip((off, rows, st), w_sm))
