"""GPU tests of genie_find_smems_long_ex (run with -m gpu on an MI355X): both strands and breaks for reads of any length.
Every comparison is exact (np.array_equal on offsets, rows and status): against genie_find_smems_long on the explicit
interleaved batch, against genie_find_smems_both / genie_find_smems_split on reads those calls accept, against the CPU
oracle run segment by segment (tests/split_util.py), and through the drop-in batched API."""
import ctypes as C

import numpy as np
import pytest

import golden_util as G
import split_util as SU
import test_long_reads_gpu as LR

pytestmark = pytest.mark.gpu

BOTH, SPLIT = 1, 2
MODES = {"bwa": 0, "lut": 1, "rmi": 2}


@pytest.fixture(scope="module")
def pkg():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import genie_smem_amd as g
    g._native.lib()
    return g


def _rc(read):
    from genie_smem_amd import packing
    read = np.asarray(read, np.uint8)
    return packing.reverse_complement(read) if read.size else read.copy()


def _inter(reads):
    """[r0, rc(r0), r1, rc(r1), ...]"""
    out = []
    for r in reads:
        out += [np.asarray(r, np.uint8), _rc(r)]
    return out


def _ex_raw(pkg, ix, mode, flags, reads, min_len=1, cap=None, ws_mult=1, offs=None, want_rc=0):
    """One or two raw calls of genie_find_smems_long_ex with exactly the workspace its size function returns (times
    ws_mult) -> (offsets, rows, status) as numpy.  cap None: a first call with no room for rows learns the total."""
    import torch
    lib = pkg._native.lib()
    bases, o = LR._csr(reads)
    if offs is not None:
        o = np.asarray(offs, np.int64)
    n = o.size - 1
    strands = 2 if flags & BOTH else 1
    total = int(bases.size)
    max_len = max([len(r) for r in reads] + [0])
    b = torch.as_tensor(bases if total else np.zeros(1, np.uint8)).cuda()
    of = torch.as_tensor(o).cuda()
    ws_bytes = lib.genie_find_smems_long_ex_workspace_bytes(n, total, max_len, flags)
    assert ws_bytes > 0
    ws_bytes *= ws_mult
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    out_off = torch.full((strands * n + 1,), -9, dtype=torch.int64, device="cuda")
    st = torch.full((max(strands * n, 1),), -9, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run(c, fill=-7):
        rows = torch.full((max(c, 1) + 4, 4), fill, dtype=torch.int32, device="cuda")
        rc = lib.genie_find_smems_long_ex(ix._h, MODES[mode], flags, p(b), p(of), n, total, max_len, min_len, p(out_off), p(rows), c,
                                          p(st), p(ws), ws_bytes, s)
        torch.cuda.synchronize()
        return rc, rows

    if cap is None:
        rc, _ = run(0)
        assert rc == want_rc
        if rc:
            return None
        cap = int(out_off[-1].item())
    rc, rows = run(cap)
    assert rc == want_rc
    if rc:
        return None
    return out_off.cpu().numpy(), rows.cpu().numpy(), st.cpu().numpy()[:strands * n], cap


def _ex(pkg, ix, mode, flags, reads, min_len=1, ws_mult=1):
    off, rows, st, cap = _ex_raw(pkg, ix, mode, flags, reads, min_len, ws_mult=ws_mult)
    assert off[0] == 0 and off[-1] == cap and (rows[cap:] == -7).all()
    return off, rows[:cap], st


def _same(a, b):
    assert np.array_equal(a[0], b[0]), "offsets"
    assert np.array_equal(a[2], b[2]), "status"
    assert a[1].shape == b[1].shape and np.array_equal(a[1], b[1]), "rows"


def _ragged(codes):
    from genie_smem_amd import synth
    rng = np.random.default_rng(3)
    short_lens = [0, 1, 2, 14, 15, 16, 31, 32, 33, 150, 255, 256, 257, 1000, 4095, 8191, 8192] + \
        [int(x) for x in rng.integers(0, 8193, 40)]
    pool = synth.reads_from_ref_fast(codes, len(short_lens), 8192, 4)
    return [pool[i, :L].copy() for i, L in enumerate(short_lens)]


def _strided(reads, width=None):
    width = width or max(max(len(r) for r in reads), 1)
    mat = np.zeros((len(reads), width), np.uint8)
    lens = np.zeros(len(reads), np.int32)
    for j, r in enumerate(reads):
        mat[j, :len(r)] = r
        lens[j] = len(r)
    return mat, lens


def _np(t3):
    return tuple(t.cpu().numpy() for t in t3)


# ------------------------------------------------------------------ property 1: flags == 0
def test_no_flags_is_the_long_call(pkg, oracle_mod):
    codes, ix, o = LR._ref(pkg, oracle_mod, 100_000)
    shorts = _ragged(codes)
    longs = [LR._from_ref(codes, 30000, 8), LR._mosaic(codes, 40000, 9, 3000, 8000)]
    reads = shorts[:20] + [longs[0]] + shorts[20:] + [longs[1]]
    for mode, ml in (("bwa", 1), ("bwa", 20), ("lut", 1), ("rmi", 1)):
        _same(_ex(pkg, ix, mode, 0, reads, ml), LR._long(ix, mode, reads, ml))
    # the wrapper's defaults are the long call
    got = _np(ix.find_smems_long("bwa", *LR._csr(reads), both_strands=False, split_breaks=False))
    _same(got, LR._long(ix, "bwa", reads))


# ------------------------------------------------------------------ property 2: both strands
def test_both_strands_matches_find_smems_both(pkg, oracle_mod):
    codes, ix, o = LR._ref(pkg, oracle_mod, 100_000)
    reads = _ragged(codes)
    mat, lens = _strided(reads, 8192)
    for mode, ml in (("bwa", 1), ("bwa", 20), ("lut", 1), ("lut", 20), ("rmi", 1), ("rmi", 20)):
        want = _np(ix.find_smems_both(mode, mat, lens, ml))
        _same(_ex(pkg, ix, mode, BOTH, reads, ml), want)
        _same(_ex(pkg, ix, mode, BOTH, reads, ml), LR._long(ix, mode, _inter(reads), ml))


@pytest.mark.parametrize("name", [100_000, 1_000_000])
def test_both_strands_long_reads_match_interleaved_batch(pkg, oracle_mod, name):
    codes, ix, o = LR._ref(pkg, oracle_mod, name)
    reads = [LR._from_ref(codes, 10_000, 1), LR._mosaic(codes, 10_000, 2, 300, 3000), np.zeros(0, np.uint8),
             LR._from_ref(codes, 100_000, 3), LR._mosaic(codes, 100_000, 4, 3000, 20000), LR._from_ref(codes, 33, 5),
             _rc(LR._mosaic(codes, 100_000, 6, 3000, 20000)), LR._from_ref(codes, 1_000_000, 99)]
    if name == 1_000_000:
        reads.append(LR._mosaic(codes, 1_000_000, 98, 3000, 4000))
    for mode, ml in (("bwa", 1), ("bwa", 20), ("lut", 1), ("rmi", 1)):
        want = LR._long(ix, mode, _inter(reads), ml)
        _same(_ex(pkg, ix, mode, BOTH, reads, ml), want)
        assert (want[2] == (0 if mode == "bwa" else 2) * (np.arange(want[2].size) // 2 == 2)).all()   # the empty read is too short for K
    # strand 0 of the forward reads is what the oracle gives (the 10 kb ones: the oracle is the slow part)
    off, sm, st = _ex(pkg, ix, "bwa", BOTH, reads[:2])
    for i in range(2):
        for s, r in enumerate((reads[i], _rc(reads[i]))):
            rc, want = LR._oracle_rows(o, r, 1)
            assert np.array_equal(sm[off[2 * i + s]:off[2 * i + s + 1]], want)
    # through the wrapper
    got = _np(ix.find_smems_long("lut", *LR._csr(reads[:6]), both_strands=True))
    _same(got, LR._long(ix, "lut", _inter(reads[:6])))


def test_both_strands_status_per_strand(pkg, oracle_mod):
    rng = np.random.default_rng(2)
    ref = rng.integers(0, 3, 50000).astype(np.uint8)              # a reference without T
    ix2 = pkg.GenieIndex.build(ref, 15).to("cuda")
    r_a = ref[1000:21000].copy()                                   # holds A: its reverse complement holds T
    r_cg = np.where(r_a == 0, 1, r_a).astype(np.uint8)             # only C and G: both strands are fine (maybe no rows)
    r_t = r_a.copy()
    r_t[15000] = 3
    r_bad = r_cg.copy()
    r_bad[77] = 9
    reads = [r_a, r_cg, r_t, r_bad, np.asarray([0, 1, 2, 1, 0], np.uint8), np.zeros(0, np.uint8)]
    got = _ex(pkg, ix2, "bwa", BOTH, reads)
    _same(got, LR._long(ix2, "bwa", _inter(reads)))
    assert got[2].tolist() == [0, 3, 0, 0, 3, 3, 1, 1, 0, 3, 0, 0]
    got = _ex(pkg, ix2, "lut", BOTH, reads)
    _same(got, LR._long(ix2, "lut", _inter(reads)))
    assert got[2].tolist()[8:] == [2, 2, 2, 2]                     # shorter than K on both strands


# ------------------------------------------------------------------ property 3: breaks
def _inject(reads, rate, seed, values=(4,)):
    rng = np.random.default_rng(seed)
    out = reads.copy()
    hit = rng.random(out.shape) < rate
    out[hit] = rng.choice(np.asarray(values, np.uint8), size=int(hit.sum()))
    return out


def _split_batches(codes):
    """(name, reads [N, L], lens or None) of the kinds test_split_reads_gpu.py uses."""
    from genie_smem_amd import synth
    base = np.concatenate([synth.reads_from_ref(codes, 300, 150, 11), synth.reads_random(100, 150, 12)])
    out = [("rate%g" % r, _inject(base, r, 13), None) for r in (0.0, 0.01, 0.1)]
    every = synth.reads_from_ref(codes, 252, 150, 31)
    for v in range(4, 256):
        every[v - 4, (v * 7) % 150] = v
        every[v - 4, (v * 13) % 150] = v
    out.append(("every_break_byte", every, None))
    runs = synth.reads_from_ref(codes, 64, 150, 21)
    runs[0, 0] = 4
    runs[1, -1] = 4
    runs[2, 0] = runs[2, -1] = 78
    runs[3, 40:60] = 4
    runs[4, ::2] = 4
    runs[5, 63:65] = 4
    runs[8, 128:] = 4
    runs[9, :] = 4
    runs[10, 1::3] = 200
    lens = np.full(64, 150, np.int32)
    lens[[0, 7, 63]] = 0                                           # empty reads, the first and the last among them
    lens[11] = 1
    runs[12] = 255
    out.append(("runs_empty_all_break", runs, lens))
    long_ = _inject(synth.reads_from_ref(codes, 8, 8192, 71), 0.005, 72)
    long_[0, :] = synth.reads_from_ref(codes, 1, 8192, 73)[0]
    out.append(("len8192", long_, None))
    return out


def _rows_list(mat, lens):
    return [mat[r, :(mat.shape[1] if lens is None else int(lens[r]))].copy() for r in range(mat.shape[0])]


@pytest.mark.parametrize("min_len", [1, 20])
def test_split_matches_find_smems_split(pkg, oracle_mod, min_len):
    codes, ix, o = LR._ref(pkg, oracle_mod, 100_000)
    for name, mat, lens in _split_batches(codes):
        want = _np(ix.find_smems_split(mat, lens, min_len))
        reads = _rows_list(mat, lens)
        got = _ex(pkg, ix, "bwa", SPLIT, reads, min_len)
        _same(got, want)
        assert not got[2].any()
        # property 4 on the same batch
        _same(_ex(pkg, ix, "bwa", BOTH | SPLIT, reads, min_len), _ex(pkg, ix, "bwa", SPLIT, _inter(reads), min_len))


def test_split_on_reference_lacking_a_base(pkg, oracle_mod):
    from genie_smem_amd import synth
    rng = np.random.default_rng(2)
    ref = rng.integers(0, 3, 50000).astype(np.uint8)              # no T: T is a break, and on strand 1 A is
    ix2 = pkg.GenieIndex.build(ref, 15).to("cuda")
    o2 = oracle_mod.Oracle(ref, 15)
    mat = synth.reads_from_ref(ref, 200, 150, 5)
    mat = _inject(mat, 0.03, 6, values=(3, 4, 200))
    want = _np(ix2.find_smems_split(mat))
    reads = _rows_list(mat, None)
    got = _ex(pkg, ix2, "bwa", SPLIT, reads)
    _same(got, want)
    for r in (0, 1, 2, 199):
        assert np.array_equal(got[1][got[0][r]:got[0][r + 1]], SU.split_rows(o2, reads[r], 1, 0x7))
    both = _ex(pkg, ix2, "bwa", BOTH | SPLIT, reads)
    _same(both, _ex(pkg, ix2, "bwa", SPLIT, _inter(reads)))
    for r in (0, 1, 199):                                          # strand 1: the segments of the reversed read, A absent
        assert np.array_equal(both[1][both[0][2 * r + 1]:both[0][2 * r + 2]], SU.split_rows(o2, _rc(reads[r]), 1, 0x7))
    # a long read on that reference: the two strands have different segment counts
    lr = np.concatenate([ref[2000:32000], [3], ref[100:5100], [0, 0, 3, 0], ref[7000:19000]]).astype(np.uint8)
    assert len(SU.segments(lr, 0x7)) != len(SU.segments(_rc(lr), 0x7))
    both = _ex(pkg, ix2, "bwa", BOTH | SPLIT, [lr])
    _same(both, _ex(pkg, ix2, "bwa", SPLIT, [lr, _rc(lr)]))


def _with_breaks(read, seed):
    """Single breaks and runs of 1 .. 10^4 of them, at position 0, at the last position and around multiples of 32 and 256."""
    rng = np.random.default_rng(seed)
    r = read.copy()
    L = r.size
    r[0] = 4
    r[L - 1] = 255
    for pos in (31, 32, 33, 64, 255, 256, 257, 511, 512, 1023, 1025, 2047, 2048, 2049, 4096, 8191, 8192):
        if pos < L:
            r[pos] = rng.integers(4, 256)
    at = L // 8
    for run in (1, 2, 31, 32, 33, 255, 256, 257, 1000, 10_000):
        if at + run + 300 >= L:
            break
        a = at - at % 256 + int(rng.integers(-1, 2))              # begins on a window edge or one off it
        r[a:a + run] = 4
        at = a + run + max(300, L // 16)
    for pos in rng.integers(0, L, max(2, L // 5000)):
        r[pos] = 4
    return r


def test_split_long_reads_vs_segment_oracle(pkg, oracle_mod):
    codes, ix, o = LR._ref(pkg, oracle_mod, 100_000)
    reads = [_with_breaks(LR._from_ref(codes, 10_000, 1), 11), np.full(3000, 4, np.uint8),
             _with_breaks(LR._from_ref(codes, 100_000, 3), 12), np.zeros(0, np.uint8),
             _with_breaks(LR._mosaic(codes, 60_000, 4, 300, 3000), 13)]
    for ml in (1, 20):
        off, sm, st = _ex(pkg, ix, "bwa", SPLIT, reads, ml)
        assert not st.any() and off[2] == off[1] and off[4] == off[3]
        for r, read in enumerate(reads):
            parts = []
            for s, l in SU.segments(read):
                rc, rows = LR._oracle_rows(o, read[s:s + l].copy(), ml)
                assert rc >= 0
                rows = rows.copy()
                rows[:, :2] += s
                parts.append(rows)
            want = np.concatenate(parts).astype(np.int32) if parts else np.zeros((0, 4), np.int32)
            assert np.array_equal(sm[off[r]:off[r + 1]], want), (ml, r)
        # property 4 on the same batch
        _same(_ex(pkg, ix, "bwa", BOTH | SPLIT, reads, ml), _ex(pkg, ix, "bwa", SPLIT, _inter(reads), ml))
    got = _np(ix.find_smems_long("bwa", *LR._csr(reads), min_len=20, both_strands=True, split_breaks=True))
    _same(got, _ex(pkg, ix, "bwa", BOTH | SPLIT, reads, 20))


@pytest.mark.parametrize("name", [100_000, 1_000_000])
def test_split_million_base_read_vs_long_call_on_segments(pkg, oracle_mod, name):
    codes, ix, o = LR._ref(pkg, oracle_mod, name)
    reads = [_with_breaks(LR._from_ref(codes, 1_000_000, 99), 21), _with_breaks(LR._from_ref(codes, 20_000, 98), 22)]
    if name == 1_000_000:
        reads.append(_with_breaks(LR._mosaic(codes, 1_000_000, 98, 3000, 4000), 23))
    for flags in (SPLIT, BOTH | SPLIT):
        sreads = _inter(reads) if flags & BOTH else reads
        segs, shift, first = [], [], [0]
        for r in sreads:
            for s, l in SU.segments(r):
                segs.append(r[s:s + l])
                shift.append(s)
            first.append(len(segs))
        for ml in (1, 20):
            soff, ssm, sst = LR._long(ix, "bwa", segs, ml)          # the host-cut segments, the shift added on the host
            assert not sst.any()
            want = ssm.copy()
            want[:, :2] += np.repeat(np.asarray(shift, np.int32), np.diff(soff))[:, None]
            off, sm, st = _ex(pkg, ix, "bwa", flags, reads, ml)
            assert not st.any()
            assert np.array_equal(off, soff[np.asarray(first)])
            assert np.array_equal(sm, want)


# ------------------------------------------------------------------ passes
@pytest.mark.parametrize("flags", [SPLIT, BOTH | SPLIT])
def test_more_units_than_the_workspace_holds(pkg, oracle_mod, flags):
    from genie_smem_amd import synth
    codes, ix, o = LR._ref(pkg, oracle_mod, 100_000)
    mat = _inject(synth.reads_from_ref_fast(codes, 12, 30_000, 5), 0.1, 6)
    reads = _rows_list(mat, None) + [_inject(LR._from_ref(codes, 200_000, 7)[None, :], 0.1, 8)[0]]
    strands = 2 if flags & BOTH else 1
    units = strands * sum(len(SU.segments(r)) for r in reads)
    held = strands * len(reads) + strands * sum(len(r) for r in reads) // 32      # what the size function provides for
    assert units > 2 * held                                        # several passes with the exact workspace
    exact = _ex(pkg, ix, "bwa", flags, reads, 1)
    roomy = _ex(pkg, ix, "bwa", flags, reads, 1, ws_mult=4)
    _same(exact, roomy)
    if flags == SPLIT:
        for r in (0, 5):
            assert np.array_equal(exact[1][exact[0][r]:exact[0][r + 1]], SU.split_rows(o, reads[r]))
    else:
        _same(exact, _ex(pkg, ix, "bwa", SPLIT, _inter(reads), 1))
    _same(_ex(pkg, ix, "bwa", flags, reads, 20), _ex(pkg, ix, "bwa", flags, reads, 20, ws_mult=4))


# ------------------------------------------------------------------ property 5
@pytest.mark.parametrize("flags", [0, BOTH, SPLIT, BOTH | SPLIT])
def test_row_capacity_no_reads_and_bad_offsets(pkg, oracle_mod, flags):
    codes, ix, o = LR._ref(pkg, oracle_mod, 100_000)
    reads = [LR._from_ref(codes, 20000, 21), LR._from_ref(codes, 9000, 22), LR._from_ref(codes, 3000, 23)]
    if flags & SPLIT:
        reads = [_with_breaks(r, 30 + i) for i, r in enumerate(reads)]
    full = _ex(pkg, ix, "bwa", flags, reads)
    total = int(full[0][-1])
    for cap in (total // 3, 1, total - 1):
        off, rows, st, _ = _ex_raw(pkg, ix, "bwa", flags, reads, cap=cap)
        assert np.array_equal(off, full[0]) and np.array_equal(st, full[2])
        assert np.array_equal(rows[:cap], full[1][:cap]) and (rows[cap:] == -7).all()
    # the wrapper reruns with the exact size
    got = _np(ix.find_smems_long("bwa", *LR._csr(reads), rows_hint=5, both_strands=bool(flags & BOTH),
                                 split_breaks=bool(flags & SPLIT)))
    _same(got, full)
    # no reads
    off, rows, st, _ = _ex_raw(pkg, ix, "bwa", flags, [], cap=4)
    assert off.tolist() == [0] and (rows == -7).all()
    # offsets the call rejects by contract (found on the device)
    L = sum(len(r) for r in reads)
    for offs in ([0, 20000, 10000, L], [0, 20000, 29000, L + 1], [-5, 20000, 29000, L]):
        assert _ex_raw(pkg, ix, "bwa", flags, reads, cap=16, offs=offs, want_rc=-1) is None
    _same(_ex(pkg, ix, "bwa", flags, reads), full)                 # and the next call is fine


def test_nonzero_first_offset(pkg, oracle_mod):
    """The reads need not start at d_bases[0]: offsets [lead, ...] inside [0, total_bases]."""
    codes, ix, o = LR._ref(pkg, oracle_mod, 100_000)
    reads = [_with_breaks(LR._from_ref(codes, 5000, 41), 42), LR._from_ref(codes, 700, 43)]
    lead = np.full(1234, 4, np.uint8)
    for flags in (BOTH, SPLIT, BOTH | SPLIT):
        want = _ex(pkg, ix, "bwa", flags, reads)
        _, o2 = LR._csr(reads)
        off, rows, st, cap = _ex_raw(pkg, ix, "bwa", flags, [np.concatenate([lead, reads[0]]), reads[1]], offs=[1234, 1234 + 5000, 1234 + 5700])
        _same((off, rows[:cap], st), want)


def test_nonzero_first_offset_whole_reads_on_one_strand(pkg, oracle_mod):
    """Where the units are whole reads on one strand -- no flags, and SPLIT_BREAKS on reads without a break -- the caller's
    offsets serve as the unit offsets: a lead that is no multiple of 32 must not show in offsets, rows or status."""
    codes, ix, o = LR._ref(pkg, oracle_mod, 100_000)
    reads = [LR._from_ref(codes, L, 50 + i) if L else np.zeros(0, np.uint8) for i, L in enumerate((0, 1, 31, 32, 33, 300, 5000))]
    lead = np.full(1234, 4, np.uint8)
    offs = 1234 + LR._csr(reads)[1]
    got = {}
    for mode, flags in (("bwa", 0), ("lut", 0), ("bwa", SPLIT)):
        off, rows, st, cap = _ex_raw(pkg, ix, mode, flags, [np.concatenate([lead, reads[0]])] + reads[1:], offs=offs)
        got[mode, flags] = (off, rows[:cap], st)
        _same(got[mode, flags], LR._long(ix, mode, reads))
    _same(got["bwa", SPLIT], got["bwa", 0])


# ------------------------------------------------------------------ drop-in
def test_dropin_strings_with_n_on_both_strands(pkg, oracle_mod):
    from genie_smem_amd import synth
    codes = synth.synth_ref(100_000, 100_000)
    ref = G.codes_to_str(codes)
    m = pkg.ExactMatch("long_ex.fa")
    m.set_reference(ref)
    sm = pkg.SMEM(m, 15)
    o = oracle_mod.Oracle(codes, 15)
    qs = []
    for i, L in enumerate((20000, 300, 9000)):
        q = list(G.codes_to_str(LR._from_ref(codes, L, 61 + i)))
        for pos in (0, 77, 256, L // 2, L - 1):
            q[pos] = "N"
        q[L // 3:L // 3 + 40] = "N" * 40
        qs.append("".join(q))
    qs.append("")
    qs.append("NNNN")
    for ml in (1, 20):
        off, rows, st = _np(sm.find_smems_long(qs, ml, both_strands=True, split_breaks=True))
        assert off.size == 2 * len(qs) + 1 and not st.any()
        for i, q in enumerate(qs):
            fwd = np.asarray(m.encode_lenient(q), np.uint8)
            for s, strand in enumerate((fwd, _rc(fwd))):
                want = SU.split_rows(o, strand, ml)
                assert np.array_equal(rows[off[2 * i + s]:off[2 * i + s + 1]], want), (ml, i, s)
    off1, rows1, st1 = _np(sm.find_smems_long(qs, 1, split_breaks=True))
    off2, rows2, _ = _np(sm.find_smems_long(qs, 1, both_strands=True, split_breaks=True))
    for i in range(len(qs)):
        assert np.array_equal(rows1[off1[i]:off1[i + 1]], rows2[off2[2 * i]:off2[2 * i + 1]])
