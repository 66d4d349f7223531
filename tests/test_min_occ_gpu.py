"""GPU tests of genie_match_stats_min_occ and genie_find_smems_min_occ (run with -m gpu on an MI355X).  Every comparison is
exact and over every read, against the brute force of tests/min_occ_util.py on its shared cases (checked on the host by
tests/test_min_occ_host.py), for k in 1, 2, 3, 11, 32, 33, 65, 1000 -- both sides of the switch between the two ways a
position is resolved -- and every flag combination: an i.i.d. reference (window reads, run starts at positions 255 and 256, a
failed run over three windows, a failed run that keeps its later positions), tandem references (intervals of hundreds of
rows), twelve bases with a base that occurs once, empty reads and no reads, unit passes; both table forms, two table_bits, a
device-built image; k = 1 against the parents byte for byte, both strands against the explicit batch, the intervals against
genie_exact_match; the LUT and RMI modes, the sizing call, a capacity that is too small, a rerun; the memory contract."""
import numpy as np
import pytest

import lookup_util as U
import match_stats_util as MS
import min_occ_util as MO
import smem_util as SM

pytestmark = pytest.mark.gpu

BOTH, SPLIT, FLAGS, KS = MO.BOTH, MO.SPLIT, MO.FLAGS, MO.KS
CASES = list(MO.cases())
_IX = {}


@pytest.fixture(scope="module")
def pkg():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import genie_smem_amd as g
    g._native.lib()
    return g


def _index(pkg, c, K=0, form="auto", knobs=None):
    dir_bits, table_bits = knobs or (c.dir_bits, 0)
    key = (U._bytes(c.ref), dir_bits, table_bits, K, form)
    if key not in _IX:
        ix = pkg.GenieIndex.build(c.ref, K, dir_bits=dir_bits, table_bits=table_bits, table_format=form)
        if K:
            ix.train_rmi([16])
        _IX[key] = ix.to("cuda")
    return _IX[key]


def _check_ms(lib, ix, c, flags, k, tag, **kw):
    bases, offs = MS.csr(c.reads)
    ms, lohi, st, short = MO.ms_call(lib, ix, flags, k, bases, offs, **kw)
    w_ms, w_lohi, w_st, w_short = MO.expected_ms(c.ref, c.reads, flags, k)
    assert np.array_equal(ms, w_ms), (tag, "ms", np.flatnonzero(ms != w_ms)[:5])
    if lohi is not None:
        assert np.array_equal(lohi, w_lohi), (tag, "lohi", np.flatnonzero((lohi != w_lohi).any(1))[:5])
    if st is not None:
        assert np.array_equal(st, w_st), (tag, "status")
    if short is not None:
        assert short == w_short, (tag, "shortened", short, w_short)
    return ms


def _check_smems(lib, ix, c, flags, k, tag, mode="bwa", min_len=1, K=0, **kw):
    bases, offs = MS.csr(c.reads)
    off, rows, st, short = MO.sized_smem_call(lib, ix, flags, k, bases, offs, {"bwa": 0, "lut": 1, "rmi": 2}[mode], min_len, **kw)
    w_off, w_rows, w_st, w_short = MO.expected_smems(c.ref, c.reads, flags, k, mode, min_len, K)
    if st is not None:
        assert np.array_equal(st, w_st), (tag, "status")
    assert np.array_equal(off, w_off), (tag, "offsets", np.flatnonzero(off != w_off)[:5])
    assert rows.shape == w_rows.shape and np.array_equal(rows, w_rows), (tag, "rows", np.flatnonzero((rows != w_rows).any(1))[:5])
    assert ((rows[:, 3] - rows[:, 2] + 1) >= k).all(), (tag, "a row of fewer than k occurrences")
    if short is not None:
        assert short == w_short, (tag, "shortened", short, w_short)
    return rows


def test_the_example_of_the_header(pkg):
    """ACGTACGTTT and the read ACGTT: the known answer of tests/test_min_occ_host.py, from both calls."""
    import test_min_occ_host as H
    lib = pkg._native.lib()
    c = MO.Case(U._codes(H.KNOWN_REF), [U._codes(H.KNOWN_READ)], dir_bits=2)
    ix = _index(pkg, c)
    bases, offs = MS.csr(c.reads)
    for k, (want_ms, want_rows) in H.KNOWN.items():
        ms, lohi, st, short = MO.ms_call(lib, ix, 0, k, bases, offs)
        assert ms.tolist() == want_ms and st.tolist() == [0] and short == (0 if k == 1 else 3)
        off, rows, st, short = MO.sized_smem_call(lib, ix, 0, k, bases, offs)
        assert rows[:, :2].tolist() == want_rows and off.tolist() == [0, len(want_rows)] and st.tolist() == [0]
        assert ((rows[:, 3] - rows[:, 2] + 1) >= k).all()


@pytest.mark.parametrize("name", CASES)
def test_every_case_against_brute_force(pkg, name):
    """Every k and all four flag combinations; intervals on and off, d_status and d_totals null and not."""
    lib = pkg._native.lib()
    c = MO.case(name)
    ix = _index(pkg, c)
    for k in KS:
        for flags in FLAGS:
            _check_ms(lib, ix, c, flags, k, (name, k, flags))
            _check_smems(lib, ix, c, flags, k, (name, k, flags))
    _check_ms(lib, ix, c, BOTH, 3, (name, "no intervals"), intervals=False, status=False, totals=False)
    _check_ms(lib, ix, c, SPLIT, 2, (name, "no status"), status=False)
    _check_smems(lib, ix, c, BOTH | SPLIT, 2, (name, "no status, no totals"), status=False, totals=False)
    _check_smems(lib, ix, c, 0, 2, (name, "min_len"), min_len=5, totals=False)


@pytest.mark.parametrize("form", ["compact", "wide"])
def test_table_forms_table_bits_and_a_device_built_image(pkg, form):
    lib = pkg._native.lib()
    for name in ("iid", "tandem3"):
        c = MO.case(name)
        for knobs in ((7, 0), (3, 4)):
            ix = _index(pkg, c, form=form, knobs=knobs)
            for k in (2, 33):
                for flags in (0, BOTH | SPLIT):
                    _check_ms(lib, ix, c, flags, k, (name, form, knobs, k, flags))
                    _check_smems(lib, ix, c, flags, k, (name, form, knobs, k, flags))
        ix = pkg.GenieIndex.build_on_device(c.ref, 0, dir_bits=7, table_format=form)
        for k in (2, 33):
            _check_ms(lib, ix, c, BOTH | SPLIT, k, (name, form, "device-built", k))
            _check_smems(lib, ix, c, BOTH, k, (name, form, "device-built", k))


def test_k_1_is_the_parents_byte_for_byte(pkg):
    lib = pkg._native.lib()
    ref = U.family()["rand4096"][:3000]
    ix = pkg.GenieIndex.build(ref, 0).to("cuda")
    for reads in (MS.window_reads(ref), MS.break_reads(ref)):
        bases, offs = MS.csr(reads)
        for flags in FLAGS:
            ms, lohi, st, short = MO.ms_call(lib, ix, flags, 1, bases, offs)
            p_ms, p_lohi, p_st = MS.call(lib, ix, flags, bases, offs)
            assert ms.tobytes() == p_ms.tobytes() and lohi.tobytes() == p_lohi.tobytes() and st.tobytes() == p_st.tobytes()
            assert short == 0
            off, rows, st, short = MO.sized_smem_call(lib, ix, flags, 1, bases, offs)
            p_off, p_rows, p_st = ix.find_smems_long("bwa", bases, offs, both_strands=bool(flags & BOTH), split_breaks=bool(flags & SPLIT))
            assert off.tobytes() == p_off.cpu().numpy().tobytes() and rows.tobytes() == p_rows.cpu().numpy().tobytes()
            assert st.tobytes() == p_st.cpu().numpy().tobytes() and short == 0


def test_both_strands_is_the_explicit_batch(pkg):
    lib = pkg._native.lib()
    c = MO.case("iid")
    ix = _index(pkg, c)
    bases, offs = MS.csr(c.reads)
    both, both_offs = MS.csr(MS.strand_reads(c.reads, 2))
    for k in (2, 33):
        for split in (0, SPLIT):
            a, b = MO.ms_call(lib, ix, BOTH | split, k, bases, offs), MO.ms_call(lib, ix, split, k, both, both_offs)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3])) and a[3] == b[3]
            a = MO.sized_smem_call(lib, ix, BOTH | split, k, bases, offs)
            b = MO.sized_smem_call(lib, ix, split, k, both, both_offs)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


@pytest.mark.parametrize("name", ["iid", "tandem7"])
def test_intervals_are_those_of_exact_match_and_one_base_more_is_rarer(pkg, name):
    """d_lohi of every position with ms_k > 0 is genie_exact_match of those bases and has k rows; where ms_k < ms the
    substring one base longer has fewer."""
    c = MO.case(name)
    ix = _index(pkg, c)
    reads = [r for r in c.reads if len(r) and int(r.max()) < 4]
    bases, offs = MS.csr(reads)
    ms = ix.match_stats(bases, offs)[0].cpu().numpy()
    for k in (2, 11, 65):
        ms_k, lohi, _, _ = ix.match_stats_min_occ(bases, offs, k)
        ms_k, lohi = ms_k.cpu().numpy(), lohi.cpu().numpy()
        at = np.flatnonzero(ms_k > 0)
        longer = np.flatnonzero(ms_k < ms)
        pats = [bases[v:v + ms_k[v]] for v in at] + [bases[v:v + ms_k[v] + 1] for v in longer]
        pb, po = MS.csr(pats)
        got = ix.exact_match(pb, po)[0].cpu().numpy().reshape(-1, 2)
        assert np.array_equal(got[:len(at)], lohi[at]) and ((lohi[at, 1] - lohi[at, 0] + 1) >= k).all()
        more = got[len(at):]
        assert len(longer) > 0 and (np.where(more[:, 0] < 0, 0, more[:, 1] - more[:, 0] + 1) < k).all()


@pytest.mark.parametrize("mode", ["lut", "rmi"])
def test_lut_and_rmi_modes_with_reads_shorter_than_k(pkg, mode):
    lib = pkg._native.lib()
    c = MO.case("short")
    K = 12
    ix = _index(pkg, c, K)
    for flags in (0, BOTH):
        rows = _check_smems(lib, ix, c, flags, 2, (mode, flags), mode=mode, K=K)
        assert rows.shape[0] > 0
    st = MO.expected_smems(c.ref, c.reads, 0, 2, mode, 1, K)[2]
    assert (st == SM.READ_TOO_SHORT).any() and (st == SM.READ_OK).any()


def test_a_capacity_that_is_too_small(pkg):
    lib = pkg._native.lib()
    c = MO.case("iid")
    ix = _index(pkg, c)
    bases, offs = MS.csr(c.reads)
    for flags in (0, BOTH | SPLIT):
        w_off, w_rows, _, w_short = MO.expected_smems(c.ref, c.reads, flags, 2)
        cap = w_rows.shape[0] // 2
        off, rows, _, short = MO.smem_call(lib, ix, flags, 2, bases, offs, cap=cap, spare=3)
        assert np.array_equal(off, w_off) and short == w_short                  # the true totals
        assert np.array_equal(rows[:cap], w_rows[:cap]) and (rows[cap:] == -7).all()


def test_no_reads_and_empty_reads(pkg):
    lib = pkg._native.lib()
    c = MO.case("once")
    ix = _index(pkg, c)
    for flags in FLAGS:
        strands = 2 if flags & BOTH else 1
        ms, lohi, st, short = MO.ms_call(lib, ix, flags, 2, np.zeros(0, np.uint8), np.zeros(1, np.int64))
        assert ms.size == 0 and st.size == 0 and short == 0
        off, rows, st, short = MO.smem_call(lib, ix, flags, 2, np.zeros(0, np.uint8), np.zeros(1, np.int64), cap=4)
        assert off.tolist() == [0] and (rows == -7).all() and short == 0
        off, rows, st, short = MO.smem_call(lib, ix, flags, 2, np.zeros(0, np.uint8), np.zeros(4, np.int64), cap=4)
        assert off.tolist() == [0] * (3 * strands + 1) and (rows == -7).all() and short == 0 and not st.any()


@pytest.mark.parametrize("name,k", [("iid", 2), ("tandem3", 33)])
def test_memory_contract(pkg, name, k):
    """Buffers of exactly the declared bytes under three poisons give the same, expected, outputs and leave every guard, the
    inputs and the index image alone."""
    import torch
    from guarded import POISONS, Arena
    lib = pkg._native.lib()
    c = MO.case(name)
    ix = _index(pkg, c)
    flags = BOTH | SPLIT
    want_ms = MO.expected_ms(c.ref, c.reads, flags, k, lead=5, tail=3)
    want_sm = MO.expected_smems(c.ref, c.reads, flags, k)
    cap = want_sm[1].shape[0] + 7
    stream = torch.cuda.Stream()
    for poison in POISONS:
        a = Arena("cuda", poison)
        a.freeze(ix.blob, "index image")
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            rcs, collect = MO.guarded_calls(lib, ix, a, stream.cuda_stream, flags, k, c.reads, cap)
        torch.cuda.synchronize()
        assert rcs == [0, 0], rcs
        a.check()
        a.check_frozen()
        got = collect()
        assert np.array_equal(got["ms"], want_ms[0]) and np.array_equal(got["lohi"], want_ms[1]), poison
        assert np.array_equal(got["ms_status"], want_ms[2]) and got["ms_totals"].tolist() == [want_ms[3]], poison
        assert np.array_equal(got["offsets"], want_sm[0]) and np.array_equal(got["rows"], want_sm[1]), poison
        assert np.array_equal(got["status"], want_sm[2]) and got["totals"].tolist() == [want_sm[3]], poison


def test_smem_wrapper_with_strings_and_a_rerun(pkg):
    """SMEM.match_stats_min_occ / find_smems_min_occ on list[str] and on (bases, read_offsets); a rows_hint that is too small
    makes find_smems_min_occ run twice, and `shortened` counts once."""
    c = MO.case("iid")
    m = pkg.ExactMatch("min_occ.fa")
    m.set_reference("".join("ACGT"[b] for b in c.ref))
    sm = pkg.SMEM(m, 4)
    reads = [r for r in c.reads if len(r) == 0 or int(r.max()) < 4]
    strs = ["".join("ACGT"[b] for b in r) for r in reads]
    w_ms = MO.expected_ms(c.ref, reads, BOTH, 2)
    w_sm = MO.expected_smems(c.ref, reads, BOTH, 2, min_len=5)
    assert w_ms[3] > 0 and w_sm[1].shape[0] > 3
    for given in (strs, MS.csr(reads)):
        ms, lohi, st, short = sm.match_stats_min_occ(given, 2, both_strands=True)
        assert short == w_ms[3] and all(np.array_equal(x.cpu().numpy(), y) for x, y in zip((ms, lohi, st), w_ms))
        off, rows, st, short = sm.find_smems_min_occ(given, 2, 5, both_strands=True)
        assert short == w_sm[3] and all(np.array_equal(x.cpu().numpy(), y) for x, y in zip((off, rows, st), w_sm))
        off, rows, st, short = sm.find_smems_min_occ(given, 2, 5, both_strands=True, rows_hint=2)
        assert short == w_sm[3] and all(np.array_equal(x.cpu().numpy(), y) for x, y in zip((off, rows, st), w_sm))
