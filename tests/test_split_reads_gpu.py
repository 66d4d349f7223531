"""GPU tests of genie_find_smems_split (run with -m gpu on an MI355X): SMEMs of reads with breaks (codes > 3, bases the
reference lacks) against the CPU oracle run segment by segment on the host (tests/split_util.py), and against the
reference's own golden rows where a segment is itself a golden read.  Every comparison is bit-exact."""
import numpy as np
import pytest

import golden_util as G
import split_util as SU

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import genie_smem_amd as g
    g._native.lib()
    return g


_REFS = {}


def _ref(pkg, oracle_mod, n, seed=None):
    """(codes, GenieIndex on the device, Oracle) of a synthetic reference of n bases (K = 15)."""
    if n not in _REFS:
        from genie_smem_amd import synth
        codes = synth.synth_ref(n, seed or n)
        ix = pkg.GenieIndex.build(codes, 15).to("cuda")
        _REFS[n] = (codes, ix, oracle_mod.Oracle(codes, 15))
    return _REFS[n]


def _inject(reads, rate, seed, values=(4,)):
    """Replace about `rate` of the positions by break bytes drawn from `values`."""
    rng = np.random.default_rng(seed)
    out = reads.copy()
    hit = rng.random(out.shape) < rate
    out[hit] = rng.choice(np.asarray(values, np.uint8), size=int(hit.sum()))
    return out


def _check(ix, o, reads, lens=None, min_len=1, present=0xF, rows_hint=None):
    off, sm, st = ix.find_smems_split(reads, lens, min_len, rows_hint=rows_hint)
    off, sm, st = off.cpu().numpy(), sm.cpu().numpy(), st.cpu().numpy()
    assert (st == 0).all()
    assert off[0] == 0 and off[-1] == sm.shape[0]
    for r in range(reads.shape[0]):
        L = reads.shape[1] if lens is None else int(lens[r])
        want = SU.split_rows(o, reads[r, :L], min_len, present)
        assert sm[off[r]:off[r + 1]].tolist() == want.tolist(), r
    return off, sm


@pytest.mark.parametrize("n", [100_000, 1_000_000])
@pytest.mark.parametrize("rate", [0.0, 0.001, 0.01, 0.1])
def test_break_rates_vs_split_oracle(pkg, oracle_mod, n, rate):
    from genie_smem_amd import synth
    codes, ix, o = _ref(pkg, oracle_mod, n)
    reads = np.concatenate([synth.reads_from_ref(codes, 300, 150, 11), synth.reads_random(100, 150, 12)])
    _check(ix, o, _inject(reads, rate, 13))


def test_runs_and_ends(pkg, oracle_mod):
    from genie_smem_amd import synth
    codes, ix, o = _ref(pkg, oracle_mod, 100_000)
    reads = synth.reads_from_ref(codes, 64, 150, 21)
    reads[0, 0] = 4
    reads[1, -1] = 4
    reads[2, 0] = reads[2, -1] = 78
    reads[3, 40:60] = 4                                       # a run of breaks
    reads[4, ::2] = 4                                         # every other base: 75 segments of one base
    reads[5, 63:65] = 4                                       # across the first 64-base boundary
    reads[6, 64] = 4
    reads[7, 63] = 4
    reads[8, 128:] = 4
    reads[9, :] = 4                                           # only breaks
    reads[10, 1::3] = 200
    for r in range(11, 64):                                   # segments shorter than K
        reads[r, (r % 13) + 1::(r % 13) + 2] = 4
    _check(ix, o, reads)


def test_every_break_byte(pkg, oracle_mod):
    from genie_smem_amd import synth
    codes, ix, o = _ref(pkg, oracle_mod, 100_000)
    reads = synth.reads_from_ref(codes, 252, 150, 31)
    for v in range(4, 256):
        r = v - 4
        reads[r, (v * 7) % 150] = v
        reads[r, (v * 13) % 150] = v
    _check(ix, o, reads)


def test_empty_and_all_break_reads(pkg, oracle_mod):
    from genie_smem_amd import synth
    codes, ix, o = _ref(pkg, oracle_mod, 100_000)
    reads = synth.reads_from_ref(codes, 40, 150, 41)
    reads[5] = 4
    reads[6] = 255
    lens = np.full(40, 150, np.int32)
    lens[[0, 7, 39]] = 0
    lens[8] = 1
    off, _ = _check(ix, o, reads, lens)
    assert off[1] == off[0] and off[-1] == off[-2]
    # a batch of nothing but breaks / empty reads, and of no reads at all
    off, sm, st = ix.find_smems_split(np.full((5, 30), 4, np.uint8))
    assert off.cpu().tolist() == [0] * 6 and sm.shape[0] == 0 and not st.cpu().numpy().any()
    off, sm, st = ix.find_smems_split(np.zeros((3, 0), np.uint8))
    assert off.cpu().tolist() == [0] * 4 and sm.shape[0] == 0
    off, sm, st = ix.find_smems_split(np.zeros((0, 150), np.uint8))
    assert off.cpu().tolist() == [0] and sm.shape[0] == 0


@pytest.mark.parametrize("L", [150, 255])
def test_fixed_lengths(pkg, oracle_mod, L):
    from genie_smem_amd import synth
    codes, ix, o = _ref(pkg, oracle_mod, 100_000)
    reads = _inject(synth.reads_from_ref(codes, 200, L, 51 + L), 0.02, 52)
    _check(ix, o, reads)


def test_ragged_lengths(pkg, oracle_mod):
    from genie_smem_amd import synth
    codes, ix, o = _ref(pkg, oracle_mod, 100_000)
    reads = _inject(synth.reads_from_ref(codes, 300, 200, 61), 0.02, 62)
    lens = np.random.default_rng(63).integers(0, 201, 300).astype(np.int32)
    _check(ix, o, reads, lens)


@pytest.mark.parametrize("L", [300, 1000, 8192])
def test_long_reads(pkg, oracle_mod, L):
    from genie_smem_amd import synth
    codes, ix, o = _ref(pkg, oracle_mod, 100_000)
    n = 8 if L == 8192 else 24
    reads = _inject(synth.reads_from_ref(codes, n, L, 71), 0.005, 72)
    reads[0, :] = synth.reads_from_ref(codes, 1, L, 73)[0]     # one read with no break among them
    _check(ix, o, reads)


@pytest.mark.parametrize("min_len", [5, 20, 40])
def test_min_len(pkg, oracle_mod, min_len):
    from genie_smem_amd import synth
    codes, ix, o = _ref(pkg, oracle_mod, 100_000)
    reads = _inject(synth.reads_from_ref(codes, 200, 150, 81), 0.01, 82)
    _check(ix, o, reads, min_len=min_len)


def test_reference_missing_a_base(pkg, oracle_mod):
    from genie_smem_amd import synth
    rng = np.random.default_rng(91)
    codes = rng.choice(np.asarray([0, 1, 3], np.uint8), 20_000)          # no G
    ix = pkg.GenieIndex.build(codes, 8).to("cuda")
    o = oracle_mod.Oracle(codes, 8)
    reads = synth.reads_random(200, 150, 92)                              # G is everywhere: a break
    reads[:50] = synth.reads_from_ref(codes, 50, 150, 93)
    reads[10:20, 70] = 2
    _check(ix, o, _inject(reads, 0.01, 94), present=SU.present_mask(codes))
    # a base that occurs only in the last bases of the reference is not a break
    tail = np.concatenate([rng.choice(np.asarray([0, 1], np.uint8), 5000), np.asarray([2, 0, 0], np.uint8)])
    ix2 = pkg.GenieIndex.build(tail, 8).to("cuda")
    o2 = oracle_mod.Oracle(tail, 8)
    rd = np.asarray([[0, 1, 2, 0, 0, 3, 1, 0, 2, 0]], np.uint8)
    _check(ix2, o2, rd, present=SU.present_mask(tail))


def test_row_capacity_exceeded(pkg, oracle_mod):
    from genie_smem_amd import synth
    import torch
    codes, ix, o = _ref(pkg, oracle_mod, 100_000)
    reads = _inject(synth.reads_random(100, 150, 101), 0.05, 102)
    full_off, full_sm, _ = ix.find_smems_split(reads)
    total = int(full_off[-1].item())
    assert total > 50
    L = pkg._native.lib()
    import ctypes as C
    from genie_smem_amd.index import _ptr, _stream
    rd = torch.as_tensor(reads).cuda()
    cap = total // 2
    rows = torch.full((total, 4), -7, dtype=torch.int32, device="cuda")
    off = torch.empty(101, dtype=torch.int64, device="cuda")
    wsb = int(L.genie_find_smems_split_workspace_bytes(100, 150))
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    rc = L.genie_find_smems_split(ix._h, _ptr(rd), C.c_void_p(0), 100, 150, 150, 1, _ptr(off), _ptr(rows), cap,
                                  C.c_void_p(0), _ptr(ws), wsb, _stream(torch.device("cuda", torch.cuda.current_device())))
    assert rc == 0
    assert int(off[-1].item()) == total
    assert off.cpu().tolist() == full_off.cpu().tolist()
    assert rows[:cap].cpu().tolist() == full_sm[:cap].cpu().tolist()
    assert (rows[cap:].cpu().numpy() == -7).all()


def test_many_passes(pkg, oracle_mod):
    """Far more segments than reads: the batch goes through the pipeline in several passes."""
    from genie_smem_amd import synth
    codes, ix, o = _ref(pkg, oracle_mod, 100_000)
    reads = synth.reads_from_ref(codes, 64, 1000, 111)
    reads[:, ::3] = 4
    reads[0] = synth.reads_from_ref(codes, 1, 1000, 112)[0]
    _check(ix, o, reads)


def test_no_breaks_equals_csr_byte_for_byte(pkg):
    from genie_smem_amd import synth
    codes, ix, _ = _REFS.get(100_000) or (None, None, None)
    if ix is None:
        codes = synth.synth_ref(100_000, 100_000)
        ix = pkg.GenieIndex.build(codes, 15).to("cuda")
    for L, n in ((150, 5000), (255, 500), (1000, 100)):
        reads = np.concatenate([synth.reads_from_ref(codes, n, L, L), synth.reads_random(n // 4, L, L + 1)])
        for min_len in (1, 25):
            a = ix.find_smems_split(reads, min_len=min_len)
            b = ix.find_smems("bwa", reads, min_len=min_len)
            for x, y in zip(a, b):
                assert x.dtype == y.dtype and x.shape == y.shape
                assert torch_equal(x, y), (L, min_len)


def torch_equal(x, y):
    import torch
    return bool(torch.equal(x, y))


def test_golden_medium_with_breaks(pkg, oracle_mod):
    """Two golden reads joined by breaks: each segment's rows are the reference's own golden rows of that read."""
    d, _ = G.load("medium_K6")
    ix = pkg.GenieIndex.build(d["ref_codes"], int(d["K"])).to("cuda")
    o = oracle_mod.Oracle(d["ref_codes"], int(d["K"]))
    for tag in ("fromref100", "random100", "edge60"):
        rd = G.reads("medium_K6", tag)
        trace = G.ref_trace("medium_K6", tag, "bwa")
        status = G.ref_status("medium_K6", tag, "bwa")
        ok = [r for r in range(len(status)) if status[r] == 0]
        pairs = [(ok[i], ok[(i * 7 + 3) % len(ok)]) for i in range(len(ok))]
        L = rd.shape[1]
        joined = np.full((len(pairs), 2 * L + 3), 4, np.uint8)
        for i, (a, b) in enumerate(pairs):
            joined[i, 1:1 + L] = rd[a]
            joined[i, L + 3:] = rd[b]
            joined[i, L + 1] = 78                               # 'N'
        off, sm, st = ix.find_smems_split(joined)
        off, sm = off.cpu().numpy(), sm.cpu().numpy()
        assert not st.cpu().numpy().any()
        for i, (a, b) in enumerate(pairs):
            ta = trace[a].astype(np.int64).copy()
            tb = trace[b].astype(np.int64).copy()
            ta[:, :2] += 1
            tb[:, :2] += L + 3
            assert sm[off[i]:off[i + 1]].tolist() == ta.tolist() + tb.tolist(), (tag, i)
        # N inside the golden reads: compare with the split oracle
        _check(ix, o, _inject(rd, 0.05, 121, values=(4, 78, 110)))


def test_smem_api_strings(pkg, oracle_mod):
    m = pkg.ExactMatch("s.fa")
    from genie_smem_amd import synth
    codes = synth.synth_ref(20_000, 131)
    m.set_reference("".join("ACGT"[c] for c in codes))
    s = pkg.SMEM(m, lut_size=8)
    o = oracle_mod.Oracle(codes, 8)
    rd = synth.reads_from_ref(codes, 20, 100, 132)
    strs = ["".join("ACGT"[c] for c in r) for r in rd]
    strs[0] = "N" + strs[0][1:]
    strs[1] = strs[1][:50] + "NNnRY" + strs[1][55:]
    strs[2] = strs[2][:30]                                      # ragged
    strs[3] = ""
    strs[4] = "NNNN"
    off, sm, st = s.find_smems_split(strs, minimum_length=3)
    off, sm = off.cpu().numpy(), sm.cpu().numpy()
    assert not st.cpu().numpy().any()
    for i, q in enumerate(strs):
        want = SU.split_rows(o, m.encode_lenient(q), 3)
        assert sm[off[i]:off[i + 1]].tolist() == want.tolist(), i
    # numpy and torch inputs give the same rows
    mat = np.full((3, 100), 4, np.uint8)
    for i in range(3):
        e = m.encode_lenient(strs[i + 5])
        mat[i, :len(e)] = e
    a = s.find_smems_split(mat, 3)
    import torch
    b = s.find_smems_split(torch.as_tensor(mat).cuda(), 3)
    assert all(torch.equal(x.cpu(), y.cpu()) for x, y in zip(a, b))
