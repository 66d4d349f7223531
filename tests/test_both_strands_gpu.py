"""GPU tests of genie_find_smems_both (run with -m gpu on an MI355X): SMEMs of both strands of every read in one call.
The defining property -- the output equals genie_find_smems_csr on the interleaved batch [r0, rc(r0), r1, rc(r1), ...]
built on the host -- is checked byte for byte; the reverse-strand rows are also checked against the CPU oracle and
against the reference's own golden rows."""
import ctypes as C

import numpy as np
import pytest

import golden_util as G

pytestmark = pytest.mark.gpu

MODES = ("bwa", "lut", "rmi")


@pytest.fixture(scope="module")
def pkg():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import genie_smem_amd as g
    g._native.lib()
    return g


_REFS = {}


def _ref(pkg, n, K=15):
    """(codes, GenieIndex with an RMI on the device) of a synthetic reference of n bases."""
    if (n, K) not in _REFS:
        from genie_smem_amd import synth
        codes = synth.synth_ref(n, n)
        m = pkg.ExactMatch(f"both{n}.fa", device="cuda")
        m.set_reference("".join("ACGT"[c] for c in codes))
        rl = pkg.RMI_LUT([1000], K, f"both{n}.fa", matcher=m)
        rl.train_RMI()
        _REFS[(n, K)] = (codes, rl._index(), rl)
    return _REFS[(n, K)]


def _interleave(pkg, reads, lens):
    """The host-built batch [r0, rc(r0), r1, rc(r1), ...] and its lengths (None stays None)."""
    rc = pkg.packing.reverse_complement(reads, lens)
    out = np.empty((2 * reads.shape[0], reads.shape[1]), np.uint8)
    out[0::2], out[1::2] = reads, rc
    return out, (None if lens is None else np.repeat(np.asarray(lens, np.int32), 2))


def _mixed_reads(pkg, codes, n, L, seed):
    """n reads of L bases: half from the forward strand of the reference, half from its reverse strand, a few random."""
    from genie_smem_amd import synth
    a = synth.reads_from_ref(codes, n, L, seed)
    a[1::2] = pkg.packing.reverse_complement(a[1::2])
    k = max(1, n // 16)
    a[-k:] = synth.reads_random(k, L, seed + 1)
    return a


def _same(pkg, ix, mode, reads, lens=None, min_len=1, rows_hint=None):
    """find_smems_both == find_smems on the interleaved batch, all three outputs, byte for byte."""
    import torch
    inter, ilens = _interleave(pkg, reads.cpu().numpy() if isinstance(reads, torch.Tensor) else reads, lens)
    a = ix.find_smems_both(mode, reads, lens, min_len, rows_hint=rows_hint)
    b = ix.find_smems(mode, inter, ilens, min_len)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape, (mode, x.shape, y.shape)
        assert torch.equal(x, y), mode
    return a


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("L", [1, 14, 15, 16, 17, 31, 32, 33, 100, 150, 255, 256, 1000, 8192])
def test_fixed_lengths_equal_interleaved(pkg, mode, L):
    codes, ix, _ = _ref(pkg, 100_000)
    n = 400 if L <= 1000 else 24
    reads = _mixed_reads(pkg, codes, n, L, 7 + L)
    _same(pkg, ix, mode, reads)
    # the same reads with every length given (d_lens path: the strand-reads' lengths come from K_A)
    _same(pkg, ix, mode, reads, np.full(n, L, np.int32))


@pytest.mark.parametrize("mode", MODES)
def test_ragged_lengths_equal_interleaved(pkg, mode):
    codes, ix, _ = _ref(pkg, 100_000)
    rng = np.random.default_rng(3)
    special = [0, 1, 14, 15, 16, 17, 31, 32, 33, 150, 255]
    # the points where the packed read gains a piece (16-base dwords, 32-base words) and their neighbours
    special += [x + d for x in range(16, 256, 16) for d in (-1, 0, 1) if 0 <= x + d <= 255]
    for width, extra in ((255, []), (8192, [256, 257, 1000, 1023, 1024, 1025, 4096, 8191, 8192])):
        ls = np.asarray(special + extra + list(rng.integers(0, width + 1, size=150)), np.int32)
        reads = _mixed_reads(pkg, codes, len(ls), width, 31 + width)
        reads[ls == 0] = 0
        _same(pkg, ix, mode, reads, ls)


def test_min_len_bwa(pkg):
    codes, ix, _ = _ref(pkg, 100_000)
    for L, min_len in ((150, 19), (150, 40), (1000, 25)):
        reads = _mixed_reads(pkg, codes, 300, L, L + min_len)
        _same(pkg, ix, "bwa", reads, min_len=min_len)
        _same(pkg, ix, "bwa", reads, np.full(300, L, np.int32), min_len=min_len)


@pytest.mark.parametrize("mode", MODES)
def test_reverse_strand_equals_oracle(pkg, oracle_mod, mode):
    """Independent of the device path: the strand-1 rows are the oracle's rows of the reverse-complemented reads."""
    codes, ix, rl = _ref(pkg, 100_000)
    o = oracle_mod.Oracle(codes, 15)
    coefs, icpts = rl.rmi.coefficients()
    o.set_rmi([1000], coefs, icpts)
    for L, n in ((150, 3000), (1000, 200)):
        reads = _mixed_reads(pkg, codes, n, L, 41 + L)
        off, sm, st = ix.find_smems_both(mode, reads)
        off, sm, st = off.cpu().numpy(), sm.cpu().numpy(), st.cpu().numpy()
        assert (st == 0).all()
        for s, batch in ((0, reads), (1, pkg.packing.reverse_complement(reads))):
            counts, want = o.find_smems_batch(mode, batch, nthreads=8)
            for r in range(n):
                v = 2 * r + s
                assert off[v + 1] - off[v] == counts[r], (L, s, r)
                assert sm[off[v]:off[v + 1]].tolist() == want[r, :counts[r]].tolist(), (L, s, r)


@pytest.mark.parametrize("ds", [d for d in ("medium_K6", "syn100k_K15") if G.have(d)])
def test_reverse_strand_equals_golden(pkg, ds):
    """Golden read q passed in as rc(q): its strand-1 rows are the reference's own rows of q."""
    d, _ = G.load(ds)
    ix = pkg.GenieIndex.build(d["ref_codes"], int(d["K"])).to("cuda")
    checked = 0
    for tag, algos in G.groups(ds):
        rd = G.reads(ds, tag)
        for algo in ("bwa", "lut"):
            if algo not in algos:
                continue
            status = G.ref_status(ds, tag, algo)
            trace = G.ref_trace(ds, tag, algo)
            q = rd[:len(status)]
            off, sm, st = ix.find_smems_both(algo, pkg.packing.reverse_complement(q))
            off, sm, st = off.cpu().numpy(), sm.cpu().numpy(), st.cpu().numpy()
            for r in range(len(status)):
                if status[r] != 0:
                    continue
                rows = sm[off[2 * r + 1]:off[2 * r + 2]]
                assert st[2 * r + 1] == 0, (tag, algo, r)
                if algo == "bwa":
                    assert rows.tolist() == trace[r].tolist(), (tag, r)
                else:
                    assert rows[:, :2].tolist() == trace[r][:len(rows)].tolist(), (tag, r)
                checked += 1
    assert checked > 100


def test_per_strand_status(pkg):
    from genie_smem_amd import synth
    rng = np.random.default_rng(9)
    ref = rng.integers(0, 3, size=20_000).astype(np.uint8)             # no T (code 3)
    ix = pkg.GenieIndex.build(ref, 8).to("cuda")
    reads = synth.reads_from_ref(ref, 64, 100, 10)                      # A, C, G only
    reads[1, :] = np.where(reads[1] == 0, 1, reads[1])                 # no A: OK on both strands (rc: C and G only)
    reads[2, 50] = 4                                                    # a bad code: flagged on both strands
    reads[3, 0] = 77
    reads[4, 99] = 255
    for mode in ("bwa", "lut"):
        _, _, st = _same(pkg, ix, mode, reads)
        st = st.cpu().numpy()
        for r in range(64):
            has_a = (reads[r] == 0).any()
            if r in (2, 3, 4):
                assert st[2 * r] == st[2 * r + 1] == 1, (mode, r)       # GENIE_READ_BAD_BASE
            else:
                assert st[2 * r] == 0, (mode, r)                        # GENIE_READ_OK
                assert st[2 * r + 1] == (3 if has_a else 0), (mode, r)  # GENIE_READ_ABSENT_BASE: A -> T
    assert (reads[5:] == 0).any(axis=1).all() and not (reads[1] == 0).any()     # both cases above were exercised


def test_capacity(pkg):
    import torch
    from genie_smem_amd.index import _ptr, _stream
    codes, ix, _ = _ref(pkg, 100_000)
    reads = _mixed_reads(pkg, codes, 200, 150, 51)
    full_off, full_sm, _ = ix.find_smems_both("lut", reads)
    total = int(full_off[-1].item())
    L = pkg._native.lib()
    rd = torch.as_tensor(reads).cuda()
    cap = total // 3
    rows = torch.full((total, 4), -7, dtype=torch.int32, device="cuda")
    off = torch.empty(401, dtype=torch.int64, device="cuda")
    st = torch.empty(400, dtype=torch.int32, device="cuda")
    wsb = int(L.genie_find_smems_both_workspace_bytes(200, 150))
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    rc = L.genie_find_smems_both(ix._h, 1, _ptr(rd), C.c_void_p(0), 200, 150, 150, 1, _ptr(off), _ptr(rows), cap, _ptr(st),
                                 _ptr(ws), wsb, _stream(torch.device("cuda", torch.cuda.current_device())))
    assert rc == 0
    assert off.cpu().tolist() == full_off.cpu().tolist()
    assert rows[:cap].cpu().tolist() == full_sm[:cap].cpu().tolist()
    assert (rows[cap:].cpu().numpy() == -7).all()
    # the Python wrapper's retry from a too small first guess gives the full result
    a = ix.find_smems_both("lut", reads, rows_hint=5)
    assert all(torch.equal(x, y) for x, y in zip(a, (full_off, full_sm, a[2])))


def test_zero_and_one_read(pkg):
    import torch
    codes, ix, _ = _ref(pkg, 100_000)
    off, sm, st = ix.find_smems_both("lut", np.zeros((0, 150), np.uint8))
    assert off.cpu().tolist() == [0] and sm.shape[0] == 0 and st.numel() == 0
    off, sm, st = ix.find_smems_both("bwa", np.zeros((3, 0), np.uint8))
    assert off.cpu().tolist() == [0] * 7 and sm.shape[0] == 0 and not st.cpu().numpy().any()
    # N = 1, the read the very first row of its allocation: the last reverse piece's window would start before the
    # buffer (lengths that are not a multiple of 16), so it must take the guarded loads
    for L in (1, 5, 15, 17, 100, 150, 255, 256, 1000):
        read = _mixed_reads(pkg, codes, 2, L, 61 + L)[:1]
        for mode in MODES:
            buf = torch.as_tensor(read).cuda()
            _same(pkg, ix, mode, buf)
            # stride > L: the row has bytes behind the read that are not part of it
            wide = np.full((1, L + 9), 2, np.uint8)
            wide[0, :L] = read[0]
            _same(pkg, ix, mode, wide, np.asarray([L], np.int32))


def test_million_reads_1mb(pkg):
    import torch
    from genie_smem_amd import synth
    codes = synth.synth_ref(1_000_000, 1_000_000)
    ix = pkg.GenieIndex.build(codes, 15).to("cuda")
    n = 1_000_000
    reads = synth.reads_from_ref_device(codes, n, 150, 71, device="cuda")
    reads[1::2] = torch.flip(reads[1::2], dims=[1]) ^ 3                 # half of them from the reverse strand
    inter = torch.empty((2 * n, 150), dtype=torch.uint8, device="cuda")
    inter[0::2] = reads
    inter[1::2] = torch.flip(reads, dims=[1]) ^ 3
    a = ix.find_smems_both("lut", reads)
    b = ix.find_smems("lut", inter)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not a[2].any() and int(a[0][-1].item()) > 2 * n


def test_dropin_strings(pkg):
    from genie_smem_amd import synth
    codes = synth.synth_ref(20_000, 81)
    m = pkg.ExactMatch("both_s.fa", device="cuda")
    m.set_reference("".join("ACGT"[c] for c in codes))
    s = pkg.SMEM(m, lut_size=8)
    rd = _mixed_reads(pkg, codes, 24, 100, 82)
    strs = ["".join("ACGT"[c] for c in r) for r in rd]
    strs[0] = strs[0][:30]                                              # ragged
    strs[1] = strs[1][:8]
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    for mode in ("bwa", "lut"):
        off, sm, st = s.find_smems_both(strs, mode=mode, minimum_length=3 if mode == "bwa" else 1)
        off, sm, st = off.cpu().numpy(), sm.cpu().numpy(), st.cpu().numpy()
        assert not st.any()
        for i, q in enumerate(strs):
            rq = "".join(comp[c] for c in reversed(q))
            for strand, qq in ((0, q), (1, rq)):
                want = s.get_SMEMS(qq, 3) if mode == "bwa" else s.get_smems_lut(qq)
                v = 2 * i + strand
                got = {}
                for a, b, lo, hi in sm[off[v]:off[v + 1]].tolist():
                    got[qq[a:b]] = (lo, hi)
                assert list(got.items()) == list(want.items()), (mode, i, strand)
    # numpy and torch inputs give the same result
    import torch
    a = s.find_smems_both(rd, mode="lut")
    b = s.find_smems_both(torch.as_tensor(rd).cuda(), mode="lut")
    assert all(torch.equal(x.cpu(), y.cpu()) for x, y in zip(a, b))
