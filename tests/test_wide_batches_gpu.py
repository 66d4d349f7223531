"""GPU tests of the CSR calls on wide batches (run with -m gpu on an MI355X): more than 2^24 and 2^26 windows (shape A: the
launches of one block per window, and per four windows, reach 2^32 threads), more than 2^31 bases and bytes and more than 2^32
virtual positions (shape B).  The method is tests/wide_util.py's: the call on a block is compared with the CPU (brute force for
the tiny blocks, the oracle for the large one), the wide batch is c copies of the block, and the wide result must be the
block's result tiled -- checked on the device, copy by copy; test_wide_batches_host.py proves that rule against the brute
force.  Every wide call's return code is looked at first.  Shape A always runs; a shape B test skips only when the device
has less free memory than 1.15 times what its workspace, outputs and inputs take.
Before the launches of one block per window were cut into slices, shape A did not come back with an error: the runtime took
the grid of 2^32 threads or more without an error and ran a part of it, most windows were never walked, and the call did
not return."""
import ctypes as C
import gc

import numpy as np
import pytest

import fasta_util as FU
import lookup_util as U
import match_stats_util as MS
import text_util as TU
import wide_util as W

pytestmark = pytest.mark.gpu

BOTH, SPLIT = W.BOTH, W.SPLIT
FAMILY = U.family()
COMPARE_BYTES = 3 << 30                                           # what the slab-wise comparisons may hold at once, generously


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


@pytest.fixture(autouse=True)
def _free_device_memory():
    yield
    import torch
    gc.collect()
    torch.cuda.empty_cache()


_IX, _BRUTE = {}, {}


def _edge_index(pkg, name):
    if name not in _IX:
        _IX[name] = pkg.GenieIndex.build(FAMILY[name], W.A1_K).to("cuda")
    return _IX[name]


def _device(reads):
    import torch
    bases, off = W.csr(reads)
    return torch.as_tensor(bases).cuda(), torch.as_tensor(off).cuda()


def _host(tensors):
    return tuple(None if t is None else t.cpu().numpy() for t in tensors)


# a call: (kind, mode or None, flags, genie_find_smems_long instead of _long_ex)
CALLS = {
    "long-bwa": ("smems", "bwa", 0, True), "long-lut": ("smems", "lut", 0, True), "long_ex-both": ("smems", "bwa", BOTH, False),
    "long_ex-split": ("smems", "bwa", SPLIT, False), "long_ex-both-split": ("smems", "bwa", BOTH | SPLIT, False),
    "match_stats": ("ms", None, 0, False), "match_stats-both": ("ms", None, BOTH, False),
    "match_stats-split": ("ms", None, SPLIT, False), "match_stats-both-split": ("ms", None, BOTH | SPLIT, False),
    "exact": ("em", None, 0, False), "exact-both": ("em", None, BOTH, False),
}
NAMES = {"smems": ("offsets", "rows", "status"), "ms": ("ms", "lohi", "status"), "em": ("lohi", "counts", "status")}


def _brute(name, shape, reads, call):
    key = (name, shape, call)
    if key not in _BRUTE:
        kind, mode, flags, _ = CALLS[call]
        ref = FAMILY[name]
        _BRUTE[key] = (W.brute_smems(ref, reads, mode, flags) if kind == "smems" else
                       W.brute_match_stats(ref, reads, flags) if kind == "ms" else W.brute_exact(ref, reads, flags))
    return _BRUTE[key]


def _run(lib, ix, call, bases, offs, max_len, cap_rows, ws_units, what):
    kind, mode, flags, long_call = CALLS[call]
    if kind == "smems":
        return W.run_smems(lib, ix, mode, flags, bases, offs, max_len, cap_rows, ws_units, long_call, what)
    if kind == "ms":
        return W.run_match_stats(lib, ix, flags, bases, offs, max_len, True, ws_units, what)
    return W.run_exact(lib, ix, flags, bases, offs, max_len, what)


def _block_then_wide(pkg, lib, name, shape, reads, call, c, units_of_block=0):
    """The call on the block against the brute force, then on c copies against the block's result tiled."""
    kind, _, flags, _ = CALLS[call]
    S = 2 if flags & BOTH else 1
    ix = _edge_index(pkg, name)
    bases, offs = _device(reads)
    max_len = max(len(r) for r in reads)
    blk = _run(lib, ix, call, bases, offs, max_len, S * (bases.numel() + 1), 0, f"{call} on the block")
    for got, want, field in zip(_host(blk), _brute(name, shape, reads, call), NAMES[kind]):
        assert got.dtype == want.dtype and np.array_equal(got, want), (call, name, "block", field)
    wide_bases, wide_offs = W.tile_csr(bases, offs, c)
    rows = int(blk[0][-1]) if kind == "smems" else 0
    wide = _run(lib, ix, call, wide_bases, wide_offs, max_len, c * rows, c * units_of_block, f"{call} on {c} copies")
    if kind == "smems":
        W.assert_tiled_csr(wide, blk, c, f"{call} {name}")
    else:
        W.assert_tiled_all(wide, blk, c, f"{call} {name}", NAMES[kind])


# ------------------------------------------------------------------ shape A: 2^24 windows and more
@pytest.mark.parametrize("call", ["long-bwa", "long-lut", "long_ex-both", "match_stats", "match_stats-both", "exact", "exact-both"])
@pytest.mark.parametrize("name", ["rand4096", "noT"])
def test_a1_tiny_reads_past_2_24_windows(pkg, lib, name, call):
    """16 805 900 reads of 0 .. 5 bases: one block per window is more than 2^32 threads."""
    _block_then_wide(pkg, lib, name, "a1", W.a1_block(name), call, W.A1_COPIES)


@pytest.mark.parametrize("call", ["long-bwa", "match_stats"])
@pytest.mark.parametrize("name", ["rand4096", "noT"])
def test_a1_tiny_reads_past_2_26_windows(pkg, lib, name, call):
    """67 223 600 reads: one block per FOUR windows is more than 2^32 threads, too."""
    _block_then_wide(pkg, lib, name, "a1", W.a1_block(name), call, W.A1_COPIES_FWD)


@pytest.mark.parametrize("call", ["long_ex-split", "long_ex-both-split", "match_stats-split", "match_stats-both-split"])
@pytest.mark.parametrize("name", ["rand4096", "noT"])
def test_a2_dense_breaks_past_2_24_units(pkg, lib, name, call):
    """4100 segments of 1 .. 3 bases per block, 4100 copies: more than 2^24 units from breaks.  The wide call's workspace is
    the size function's for as many reads as there are units, so every unit fits ONE pass (the minimum workspace holds one
    unit per 32 positions and would keep every pass under the limit); the block's call takes the minimum one, in passes."""
    reads = W.a2_block(name)
    flags = CALLS[call][2]
    units = W.forward_segments(FAMILY[name], MS.strand_reads(reads, 2 if flags & BOTH else 1))
    assert units >= W.A2_SEGMENTS and units * W.A2_COPIES > 1 << 24
    _block_then_wide(pkg, lib, name, "a2", reads, call, W.A2_COPIES, units_of_block=units)


# ------------------------------------------------------------------ shape B: bases past 2^31, positions past 2^32
def _gate(need):
    """Skip only if the device's free memory is below 1.15 times the test's need."""
    import torch
    gc.collect()
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    if free < 1.15 * need:
        pytest.skip(f"needs 1.15 x {need} bytes of device memory, {free} are free")


@pytest.fixture(scope="module")
def big(pkg, oracle_mod):
    """The large block on the 100 000-base synthetic reference, its index and oracle, and the oracle's rows of every read."""
    import test_long_reads_gpu as LR
    codes, ix, o = LR._ref(pkg, oracle_mod, W.B_REF)
    reads = W.b_block(codes)
    rows = []
    for r in reads:
        rows.append(None if (r > 3).any() else LR._oracle_rows(o, r, 1)[1])
    return {"codes": codes, "ix": ix, "oracle": o, "reads": reads, "rows": rows, "max_len": max(len(r) for r in reads)}


def _inputs_bytes(big, c):
    return c * W.B_BASES + 8 * (c * len(big["reads"]) + 1) + COMPARE_BYTES


def _interval(o, pat):
    if (pat > 3).any():
        return (-2, -2)
    return tuple(int(x) for x in o.back_prop(pat))


@pytest.mark.parametrize("flags", [0, BOTH], ids=["one-strand", "both-strands"])
def test_b_exact_match_past_2_31_bases(pkg, lib, big, flags):
    """The block's reads as patterns (max_len 300 000: the packed-stream path).  Block: the oracle's backward search of every
    strand-pattern."""
    c, n, S = W.B_COPIES, len(big["reads"]), 2 if flags & BOTH else 1
    _gate(W.exact_bytes(lib, flags, c * n, c * W.B_BASES, big["max_len"])[1] + _inputs_bytes(big, c))
    bases, offs = _device(big["reads"])
    blk = W.run_exact(lib, big["ix"], flags, bases, offs, big["max_len"], "exact_match on the block")
    lohi, counts, st = _host(blk)
    want = np.asarray([_interval(big["oracle"], p) for p in MS.strand_reads(big["reads"], S)], np.int32)
    assert np.array_equal(lohi, want), np.flatnonzero((lohi != want).any(1))[:5]
    assert np.array_equal(counts, np.where(want[:, 0] >= 0, want[:, 1] - want[:, 0] + 1, 0))
    assert np.array_equal(st, (want[:, 0] == -2).astype(np.int32)) and st.sum() == S and (counts > 0).sum() >= 1000
    wide_bases, wide_offs = W.tile_csr(bases, offs, c)
    assert wide_bases.numel() > 1 << 31
    wide = W.run_exact(lib, big["ix"], flags, wide_bases, wide_offs, big["max_len"], f"exact_match on {c} copies")
    W.assert_tiled_all(wide, blk, c, "exact_match", NAMES["em"])


def _check_block_match_stats(big, flags, ms, lohi, st):
    """The block's matching statistics against the CPU: at every start of an oracle SMEM the length and the interval are the
    row's (forward strand-reads); at sampled positions of every strand-read the match occurs in the reference and one base
    more does not (bytes.find), and its interval is the oracle's backward search; everywhere ms[p + 1] >= ms[p] - 1."""
    S = 2 if flags & BOTH else 1
    o, ref = big["oracle"], big["codes"].tobytes()
    rng = np.random.default_rng(5)
    at = sampled = 0
    for q, r in enumerate(MS.strand_reads(big["reads"], S)):
        L = len(r)
        m = ms[at:at + L]
        if (r > 3).any():
            assert st[q] == MS.READ_BAD_BASE and (m == -1).all() and (lohi is None or (lohi[at:at + L] == -1).all()), q
            at += L
            continue
        assert st[q] == MS.READ_OK and (m >= 1).all() and (m <= L - np.arange(L)).all() and (m[1:] >= m[:-1] - 1).all(), q
        rows = big["rows"][q // S] if q % S == 0 else None
        if rows is not None and len(rows):
            assert np.array_equal(m[rows[:, 0]], rows[:, 1] - rows[:, 0]), q
            assert lohi is None or np.array_equal(lohi[at + rows[:, 0]], rows[:, 2:4]), q
        rb = r.tobytes()
        for p in {0, L - 1} | set(rng.integers(0, L, 2 if L <= 150 else 200).tolist()):
            l = int(m[p])
            assert rb[p:p + l] in ref and (p + l == L or rb[p:p + l + 1] not in ref), (q, p, l)
            assert lohi is None or tuple(lohi[at + p]) == _interval(o, r[p:p + l]), (q, p, l)
            sampled += 1
        at += L
    assert at == ms.size and sampled > 9000 * S


@pytest.mark.parametrize("flags,intervals", [(0, True), (BOTH, False)], ids=["one-strand-intervals", "both-strands-lengths"])
def test_b_match_stats_past_2_31_bases_2_32_positions(pkg, lib, big, flags, intervals):
    c, n = W.B_COPIES, len(big["reads"])
    _gate(W.match_stats_bytes(lib, flags, c * n, c * W.B_BASES, big["max_len"], intervals)[1] + _inputs_bytes(big, c))
    bases, offs = _device(big["reads"])
    blk = W.run_match_stats(lib, big["ix"], flags, bases, offs, big["max_len"], intervals, what="match_stats on the block")
    _check_block_match_stats(big, flags, *_host(blk))
    wide_bases, wide_offs = W.tile_csr(bases, offs, c)
    wide = W.run_match_stats(lib, big["ix"], flags, wide_bases, wide_offs, big["max_len"], intervals, what=f"match_stats on {c} copies")
    assert wide[0].numel() > (1 << 32 if flags & BOTH else 1 << 31)
    W.assert_tiled_all(wide, blk, c, "match_stats", NAMES["ms"])


def test_b_find_smems_long_past_2_31_bases(pkg, lib, big):
    """Block: the oracle's rows of every read, bit for bit.  Wide: rows_hint is c times the block's rows."""
    c, n = W.B_COPIES, len(big["reads"])
    bases, offs = _device(big["reads"])
    blk = W.run_smems(lib, big["ix"], "bwa", 0, bases, offs, big["max_len"], W.B_BASES, long_call=True, what="find_smems_long on the block")
    off, sm, st = _host(blk)
    assert off[0] == 0 and off[-1] == sm.shape[0]
    for r, want in enumerate(big["rows"]):
        got = sm[off[r]:off[r + 1]]
        if want is None:
            assert st[r] == MS.READ_BAD_BASE and got.shape[0] == 0
        else:
            assert st[r] == 0 and got.shape == want.shape and (got == want).all(), (r, len(big["reads"][r]))
    rows = int(off[-1])
    _gate(W.smems_bytes(lib, 0, c * n, c * W.B_BASES, big["max_len"], c * rows)[1] + _inputs_bytes(big, c))
    wide_bases, wide_offs = W.tile_csr(bases, offs, c)
    wide = W.run_smems(lib, big["ix"], "bwa", 0, wide_bases, wide_offs, big["max_len"], c * rows, long_call=True,
                       what=f"find_smems_long on {c} copies")
    W.assert_tiled_csr(wide, blk, c, "find_smems_long")


# ------------------------------------------------------------------ text past 2^31 bytes
def _tiled_text(lib, text, c, fasta):
    """The wide call on c copies of `text` -> (status, out5, bases, offsets, record starts or None) on the device."""
    import torch
    want = FU.same_as_model(lib, text) if fasta else TU.same_as_model(lib, text, TU.LINES)
    assert want[0] == TU.OK
    n, total = want[1][0], want[1][1]
    T = c * len(text)
    util = FU if fasta else TU
    tmp_bytes = util.tmp_bytes(lib, T, c * n)
    _gate(T + c * total + 8 * (c * n + 1) * (2 if fasta else 1) + tmp_bytes + COMPARE_BYTES)
    wide_text = torch.as_tensor(np.frombuffer(text, np.uint8).copy()).cuda().repeat(c)
    bases = torch.full((c * total,), 0xA5, dtype=torch.uint8, device="cuda")
    offs = torch.full((c * n + 1,), -7, dtype=torch.int64, device="cuda")
    starts = torch.full((c * n,), -7, dtype=torch.int64, device="cuda") if fasta else None
    tmp = torch.empty(tmp_bytes, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    if fasta:
        rc, out5 = FU.raw_call(lib, wide_text.data_ptr(), T, 0, FU.ACGT4, bases.data_ptr(), c * total, offs.data_ptr(), starts.data_ptr(),
                               c * n, tmp.data_ptr(), tmp_bytes, stream)
    else:
        rc, out5 = TU.raw_call(lib, wide_text.data_ptr(), T, TU.LINES, 0, TU.ACGT4, bases.data_ptr(), c * total, offs.data_ptr(), c * n,
                               tmp.data_ptr(), tmp_bytes, stream)
    torch.cuda.synchronize()
    W.ok(lib, rc, f"reads_from_{'fasta' if fasta else 'text'} on {c} copies (out5 {out5})")
    assert T > 1 << 31 and c * total > 1 << 31
    assert out5 == [c * n, c * total, want[1][2], T, -1], out5
    W.assert_tiled(bases, want[3], c, "bases")
    W.assert_tiled_offsets(offs, want[2], c, "read offsets")
    if fasta:
        W.assert_tiled_offsets(torch.cat([starts, torch.tensor([T], dtype=torch.int64, device="cuda")]),
                               np.append(want[4], len(text)), c, "record starts")


def test_b_reads_from_text_past_2_31_bytes(pkg, lib):
    _tiled_text(lib, W.lines_block(), W.TEXT_COPIES, fasta=False)


def test_b_reads_from_fasta_past_2_31_bytes(pkg, lib):
    _tiled_text(lib, W.fasta_block(), W.TEXT_COPIES, fasta=True)


# ------------------------------------------------------------------ locate past 2^31 positions
def test_b_locate_past_2_31_positions(pkg, lib):
    """The interval (0, n) of an all-A reference of 2^20 bases, 2100 times: every interval's slice is the whole suffix
    array, which for such a reference is n + 1, n, ..., 1 (the shorter suffix sorts first)."""
    import torch
    n, c = W.LOCATE_N, W.LOCATE_COPIES
    cap = c * (n + 1)
    tmp_bytes = lib.genie_locate_tmp_bytes(c)
    _gate(4 * cap + tmp_bytes + COMPARE_BYTES + (64 << 20))
    ix = pkg.GenieIndex.build(np.zeros(n, np.uint8), 0).to("cuda")
    lohi = torch.tensor([[0, n]] * c, dtype=torch.int32, device="cuda")
    offs = torch.full((c + 1,), -7, dtype=torch.int64, device="cuda")
    pos = torch.full((cap,), -7, dtype=torch.int32, device="cuda")
    tmp = torch.empty(tmp_bytes, dtype=torch.uint8, device="cuda")
    rc = lib.genie_locate(ix._h, C.c_void_p(lohi.data_ptr()), 2, c, C.c_void_p(offs.data_ptr()), C.c_void_p(pos.data_ptr()), cap,
                          C.c_void_p(tmp.data_ptr()), tmp_bytes, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    W.ok(lib, rc, f"locate of {c} intervals of {n + 1} rows")
    assert cap > 1 << 31
    want = torch.arange(0, (c + 1) * (n + 1), n + 1, dtype=torch.int64, device="cuda")
    assert torch.equal(offs, want)
    first = pos[:n + 1]
    assert torch.equal(first, torch.arange(n + 1, 0, -1, dtype=torch.int32, device="cuda"))
    sa = np.ctypeslib.as_array(lib.genie_index_suffix_array(ix._h), (n + 1,))
    assert np.array_equal(first.cpu().numpy(), sa)
    W.assert_tiled(pos, first, c, "positions")


# ------------------------------------------------------------------ what one launch still cannot cover: a clean error
def test_remaining_limits_are_clean_errors(pkg, lib):
    """include/genie_smem.h, "Batch sizes": a text of 2^36 bytes (one 256-thread block per 4096 bytes: 2^24 blocks) and 2^32
    intervals (one thread each) are GENIE_E_TOO_LONG.  The check comes before the first launch, so the sizing call of the text
    entry points and a locate over buffers of the declared scratch size return at once and touch nothing."""
    import torch
    E_TOO_LONG = -6
    T = 1 << 36
    text = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for util, call in ((TU, lambda tmp, nb: TU.raw_call(lib, text.data_ptr(), T, TU.LINES, 0, TU.ACGT4, 0, 0, 0, 0, tmp.data_ptr(), nb, stream)),
                       (FU, lambda tmp, nb: FU.raw_call(lib, text.data_ptr(), T, 0, FU.ACGT4, 0, 0, 0, 0, 0, tmp.data_ptr(), nb, stream))):
        nb = util.tmp_bytes(lib, T, 0)
        _gate(nb)
        tmp = torch.empty(nb, dtype=torch.uint8, device="cuda")
        rc, out5 = call(tmp, nb)
        assert rc == E_TOO_LONG, (rc, lib.genie_strerror(rc), out5)
        del tmp
        # two tiles fewer is a launch that HIP accepts at any alignment of the text: the limit is stated where it is
        assert ((T - 8192 + 15 + 4095) // 4096) * 256 < W.LAUNCH_LIMIT <= ((T + 4095) // 4096) * 256
    S = 1 << 32
    nb = lib.genie_locate_tmp_bytes(S)
    _gate(nb)
    ix = _edge_index(pkg, "rand4096")
    tmp = torch.empty(nb, dtype=torch.uint8, device="cuda")
    small = torch.zeros(16, dtype=torch.int64, device="cuda")
    rc = lib.genie_locate(ix._h, C.c_void_p(small.data_ptr()), 2, S, C.c_void_p(small.data_ptr()), C.c_void_p(small.data_ptr()), 0,
                          C.c_void_p(tmp.data_ptr()), nb, C.c_void_p(stream))
    torch.cuda.synchronize()
    assert rc == E_TOO_LONG, (rc, lib.genie_strerror(rc))
    assert ((S - 256 + 255) // 256) * 256 < W.LAUNCH_LIMIT <= ((S + 255) // 256) * 256
