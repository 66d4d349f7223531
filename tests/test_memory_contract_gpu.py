"""GPU tests of the memory promises of include/genie_smem.h (run with -m gpu on an MI355X), through the raw C ABI on guarded
buffers (tests/guarded.py, tests/contract_calls.py):

  - no call depends on what its caller-owned output and scratch buffers held before: every case runs three times, with all of
    them -- guards included -- filled with 0x00, then 0xFF, then 0x5A, and the defined outputs must be the same bytes;
  - no call writes outside the sizes it declares: every buffer has exactly the bytes asked for, the weakest alignment the
    header allows and 4 KiB of guard on each side, and whatever the header says is dropped still holds the poison;
  - inputs and the opened index image are not written;
  - a read past the end of an input would see a different guard under each poison, and change the result.

Every result is also compared with the CPU oracle (or with the host builder's image).  All comparisons are exact; the
escape list of the packed calls is compared as a set."""
import ctypes as C

import numpy as np
import pytest

import contract_calls as CC
import split_util as SU
from guarded import POISONS, Arena, as_numpy

pytestmark = pytest.mark.gpu

K = 11
BOTH, SPLIT = CC.BOTH, CC.SPLIT


class Ref:
    """A reference: its codes, its index on `device` (K-mer table and a natively trained RMI), the CPU oracle."""

    def __init__(self, g, oracle_mod, codes, k=K, rmi=True, device="cuda"):
        self.codes = codes
        ix = g.GenieIndex.build(codes, k)
        if rmi:
            ix.train_rmi([100])
        self.lut = tuple(x.copy() for x in ix.lut_arrays())
        self.ix = ix.to(device) if device else ix
        self.o = oracle_mod.Oracle(codes, k)
        self.present = SU.present_mask(codes)


@pytest.fixture(scope="module")
def env(oracle_mod):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import genie_smem_amd as g
    from genie_smem_amd import synth

    class Env:
        pass
    e = Env()
    e.g, e.lib = g, g._native.lib()
    e.main = Ref(g, oracle_mod, synth.synth_ref(50_000, 50_000))
    e.no_t = Ref(g, oracle_mod, np.random.default_rng(7).integers(0, 3, 30_000).astype(np.uint8))    # a reference without T
    e.oracle_mod = oracle_mod
    return e


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def three(ref, case, partial=()):
    """Run `case(arena, stream) -> Call` under each poison in turn: status, guards, frozen inputs and `ref`'s image; the defined
    outputs are the same under all three (keys in `partial` excepted: a truncated, unordered list).  Returns them."""
    import torch
    results = []
    for poison in POISONS:
        a = Arena("cuda", poison)
        if ref is not None:
            a.freeze(ref.ix.blob, "index image")
        call = case(a, _stream())
        torch.cuda.synchronize()
        res = call.result()
        a.check()
        a.check_frozen()
        results.append(res)
    for other in results[1:]:
        CC.same({k: v for k, v in results[0].items() if k not in partial}, {k: v for k, v in other.items() if k not in partial})
    return results[0]


# ------------------------------------------------------------------ what the oracle says
def _status(ref, mode, read):
    """The GENIE_READ_* code of include/genie_smem.h for this read (the inputs here never meet two conditions at once)."""
    read = np.asarray(read, np.uint8)
    if (read > 3).any():
        return 1
    if mode != "bwa" and read.size < K:
        return 2
    if any(not (ref.present >> int(b)) & 1 for b in np.unique(read)):
        return 3
    return 0


def expect_csr(ref, mode, reads, min_len=1):
    """(offsets, rows, status) of a batch: the oracle's BWA traversal is the specification of every mode (min_len applies in
    BWA mode only); flagged reads contribute no rows."""
    parts, status = [], []
    for read in reads:
        st = _status(ref, mode, read)
        status.append(st)
        if st == 0:
            rc, rows = ref.o.find_smems("bwa", np.asarray(read, np.uint8), min_len if mode == "bwa" else 1)
            assert rc >= 0
            parts.append(rows.astype(np.int32).reshape(-1, 4))
        else:
            parts.append(np.zeros((0, 4), np.int32))
    offsets = np.zeros(len(reads) + 1, np.int64)
    offsets[1:] = np.cumsum([len(p) for p in parts])
    rows = np.concatenate(parts) if parts else np.zeros((0, 4), np.int32)
    return offsets, rows, np.asarray(status, np.int32)


def expect_split(ref, reads, min_len=1):
    parts = [SU.split_rows(ref.o, r, min_len, ref.present) for r in reads]
    offsets = np.zeros(len(reads) + 1, np.int64)
    offsets[1:] = np.cumsum([len(p) for p in parts])
    rows = np.concatenate(parts).astype(np.int32) if parts else np.zeros((0, 4), np.int32)
    return offsets, rows, np.zeros(len(reads), np.int32)


def _rc(read):
    read = np.asarray(read, np.uint8)
    out = read[::-1].copy()
    out[out < 4] ^= 3
    return out


def _interleave(reads):
    out = []
    for r in reads:
        out += [np.asarray(r, np.uint8), _rc(r)]
    return out


def _rows_list(mat, lens):
    return [mat[i, :(mat.shape[1] if lens is None else int(lens[i]))] for i in range(mat.shape[0])]


def check_csr(res, want, cap_rows, with_status=True):
    off, rows, st = want
    assert np.array_equal(res["offsets"], off)
    assert np.array_equal(res["rows"], rows[:min(len(rows), cap_rows)])
    if with_status:
        assert np.array_equal(res["status"], st)


def _ragged(ref, n, width, seed, short=(0, 1, 5, K - 1, K)):
    """n reads from the reference in a matrix `width` bytes wide (the bytes past a read's length are other bases), ragged
    lengths that include 0 and lengths below K."""
    from genie_smem_amd import synth
    rng = np.random.default_rng(seed)
    mat = synth.reads_from_ref_fast(ref.codes, n, width, seed)
    lens = rng.integers(K, width + 1, n).astype(np.int32)
    lens[:len(short)] = short
    lens[len(short)] = width
    return mat, lens


# ------------------------------------------------------------------ genie_sa_interval
def test_sa_interval(env):
    from genie_smem_amd import synth
    ref = env.main
    rng = np.random.default_rng(1)
    pats = np.concatenate([synth.reads_from_ref_fast(ref.codes, 200, 40, 2), synth.reads_random(100, 40, 3)])

    def want(lens):
        out = []
        for i in range(pats.shape[0]):
            p = pats[i, :lens[i]]
            out.append((-2, -2) if (p > 3).any() else ref.o.back_prop(p))
        return np.asarray(out, np.int32)

    # fixed length 24 in rows 40 wide (a stride wider than the longest pattern), then ragged with length 0 and a code > 3
    res = three(ref, lambda a, s: CC.sa_interval(env.lib, ref.ix, a, s, pats, None, 24))
    assert np.array_equal(res["lohi"], want([24] * 300))
    lens = rng.integers(0, 31, 300).astype(np.int32)
    lens[:3] = [0, 1, 30]
    bad = pats.copy()
    bad[7, 3] = 4
    bad[8, 29] = 255
    lens[7:9] = 30
    pats = bad
    res = three(ref, lambda a, s: CC.sa_interval(env.lib, ref.ix, a, s, pats, lens, 30))
    assert np.array_equal(res["lohi"], want(lens))
    assert res["lohi"][0].tolist() == [0, ref.codes.size] and res["lohi"][7].tolist() == [-2, -2]


# ------------------------------------------------------------------ genie_seed_lookup
def test_seed_lookup(env):
    ref = env.main
    codes, lo, hi = ref.lut
    rng = np.random.default_rng(4)
    sel = rng.choice(len(codes), 500, replace=False)
    present = ((codes[sel, None].astype(np.int64) >> (2 * (K - 1 - np.arange(K)))) & 3).astype(np.uint8)
    kmers = np.concatenate([present, rng.integers(0, 4, (500, K)).astype(np.uint8)])      # the random ones are mostly absent
    w = 4 ** np.arange(K - 1, -1, -1, dtype=np.int64)
    key = (kmers.astype(np.int64) * w).sum(1)
    at = np.searchsorted(codes.astype(np.int64), key)
    found = (at < len(codes)) & (codes.astype(np.int64)[np.minimum(at, len(codes) - 1)] == key)
    assert found[:500].all() and (~found).sum() > 100
    res = three(ref, lambda a, s: CC.seed_lookup(env.lib, ref.ix, a, s, "lut", kmers, False))
    want = np.where(found[:, None], np.stack([lo[np.minimum(at, len(lo) - 1)], hi[np.minimum(at, len(hi) - 1)]], 1), -1)
    assert np.array_equal(res["lohi"], want.astype(np.int32))
    plain = three(ref, lambda a, s: CC.seed_lookup(env.lib, ref.ix, a, s, "rmi", kmers, False))
    full = three(ref, lambda a, s: CC.seed_lookup(env.lib, ref.ix, a, s, "rmi", kmers, True))
    assert np.array_equal(plain["lohi"], full["lohi"])
    got = full["lohi"]
    assert np.array_equal(got[found], want[found].astype(np.int32))          # the true interval
    assert (got[~found, 0] > got[~found, 1]).all()                             # absent: lower > upper
    assert np.array_equal(full["pred"], _rmi_predict(env, ref, key))          # float64, bit for bit


def _rmi_predict(env, ref, keys):
    """RMI_LUT.rmi_predict of the exported two-level model (1 + 100 linear models), by the oracle's own implementation."""
    coef, icpt = np.empty(101, np.float64), np.empty(101, np.float64)
    assert env.lib.genie_index_rmi_models(ref.ix._h, coef.ctypes.data_as(C.c_void_p), icpt.ctypes.data_as(C.c_void_p), None) == 0
    ref.o.set_rmi([100], [coef[:1], coef[1:]], [icpt[:1], icpt[1:]])
    return np.asarray([ref.o.rmi_predict(int(k)) for k in keys], np.float64)


# ------------------------------------------------------------------ genie_find_smems (slots) and genie_compact_smems
def _slots_want(ref, mode, reads, min_len, cap):
    off, rows, st = expect_csr(ref, mode, reads, min_len)
    counts = np.diff(off).astype(np.int32)
    st = np.where((st == 0) & (counts > cap), 4, st).astype(np.int32)
    kept = [rows[off[r]:off[r] + min(int(counts[r]), cap)] for r in range(len(reads))]
    return {"counts": counts, "slots": np.concatenate(kept), "status": st}


@pytest.mark.parametrize("mode", ["bwa", "lut", "rmi"])
def test_find_smems_slots(env, mode):
    ref = env.main
    mat, lens = _ragged(ref, 200, 150, 11)
    mat[9, 20] = 6
    lens[9] = 100
    reads = _rows_list(mat, lens)
    min_len = 12 if mode == "bwa" else 1
    want = _slots_want(ref, mode, reads, min_len, 150)
    assert want["status"][9] == 1 and want["counts"].max() > 2
    res = three(ref, lambda a, s: CC.find_slots(env.lib, ref.ix, a, s, mode, mat, lens, 150, min_len, 150))
    CC.same(res, want)
    # no status array: the rest is the same
    res = three(ref, lambda a, s: CC.find_slots(env.lib, ref.ix, a, s, mode, mat, lens, 150, min_len, 150, with_status=False))
    want.pop("status")
    CC.same(res, want)
    # two slots per read: GENIE_READ_OVERFLOW, d_counts keeps the true count, the neighbours' slots are untouched by it
    want = _slots_want(ref, mode, reads, 1, 2)
    assert (want["status"] == 4).sum() > 50 and (want["status"] == 0).sum() > 2
    res = three(ref, lambda a, s: CC.find_slots(env.lib, ref.ix, a, s, mode, mat, lens, 150, 1, 2))
    CC.same(res, want)


def test_compact_smems(env):
    ref = env.main
    mat, lens = _ragged(ref, 700, 60, 12)            # more than one scan block of reads
    reads = _rows_list(mat, lens)
    off, rows, _ = expect_csr(ref, "bwa", reads)
    cap = 9
    counts = np.diff(off).astype(np.int32)
    assert counts.max() > cap and off[-1] - off[-2] > 1
    slots = np.full((700, cap, 4), 0x11111111, np.int32)
    kept = []
    for r in range(700):
        k = min(int(counts[r]), cap)
        slots[r, :k] = rows[off[r]:off[r] + k]
        kept.append(rows[off[r]:off[r] + k])
    want_rows = np.concatenate(kept)
    want_off = np.zeros(701, np.int64)
    want_off[1:] = np.cumsum(np.minimum(counts, cap))
    total = int(want_off[-1])

    def run(out_cap):
        return three(None, lambda a, s: CC.compact(env.lib, a, s, counts, slots, out_cap))     # (the call takes no index)

    res = run(None)                                  # the sizing call
    assert np.array_equal(res["offsets"], want_off) and "rows" not in res
    for out_cap in (total, total - 1):
        res = run(out_cap)
        assert np.array_equal(res["offsets"], want_off)
        assert np.array_equal(res["rows"], want_rows[:out_cap])


# ------------------------------------------------------------------ genie_find_smems_csr
GEOMETRIES = [(150, 151, 300), (600, 601, 40), (8192, 8193, 12)]      # (longest read, odd stride, reads): one per launch geometry


@pytest.mark.parametrize("mode", ["bwa", "lut", "rmi"])
@pytest.mark.parametrize("max_len,stride,n", GEOMETRIES)
def test_find_smems_csr(env, mode, max_len, stride, n):
    """Ragged reads at an odd address with an odd stride, lengths 0 and below K among them, one read with a code > 3 and one
    with a base the reference lacks (a reference without T): flagged reads contribute no rows."""
    ref = env.no_t
    mat, lens = _ragged(ref, n, stride, 20 + max_len)
    lens = np.minimum(lens, max_len).astype(np.int32)
    lens[5] = max_len
    mat[7, 13] = 9
    mat[8, 14] = 3                                   # T
    lens[7:9] = max_len // 2
    reads = _rows_list(mat, lens)
    min_len = 15 if mode == "bwa" else 1
    want = expect_csr(ref, mode, reads, min_len)
    total = int(want[0][-1])
    assert want[2][7] == 1 and want[2][8] == 3 and want[2][0] == (0 if mode == "bwa" else 2) and total > 10
    for cap in (total, total - 1, 0):
        res = three(ref, lambda a, s: CC.find_csr(env.lib, ref.ix, a, s, "csr", mode, mat, lens, max_len, min_len, cap))
        check_csr(res, want, cap)
    res = three(ref, lambda a, s: CC.find_csr(env.lib, ref.ix, a, s, "csr", mode, mat, lens, max_len, min_len, total,
                                              with_status=False))
    check_csr(res, want, total, with_status=False)


def test_find_smems_csr_fixed_length(env):
    ref = env.main
    from genie_smem_amd import synth
    for L, n in ((150, 400), (255, 100), (256, 100)):
        mat = synth.reads_from_ref_fast(ref.codes, n, L + 1, L)
        want = expect_csr(ref, "lut", _rows_list(mat[:, :L], None))
        total = int(want[0][-1])
        res = three(ref, lambda a, s: CC.find_csr(env.lib, ref.ix, a, s, "csr", "lut", mat, None, L, 1, total))
        check_csr(res, want, total)


# ------------------------------------------------------------------ genie_find_smems_both
@pytest.mark.parametrize("mode", ["bwa", "lut", "rmi"])
def test_find_smems_both(env, mode):
    ref = env.main
    from genie_smem_amd import synth
    for L, n, ragged in ((150, 200, False), (149, 200, True), (601, 30, True), (1003, 20, False)):   # not multiples of 16
        mat = synth.reads_from_ref_fast(ref.codes, n, L, 30 + L)
        lens = None
        if ragged:
            lens = np.random.default_rng(L).integers(K, L + 1, n).astype(np.int32)
            lens[:4] = [0, 1, K - 1, L]
        want = expect_csr(ref, mode, _interleave(_rows_list(mat, lens)), 14 if mode == "bwa" else 1)
        total = int(want[0][-1])
        for cap in (total, total - 1):
            res = three(ref, lambda a, s: CC.find_csr(env.lib, ref.ix, a, s, "both", mode, mat, lens, L, 14 if mode == "bwa" else 1, cap))
            check_csr(res, want, cap)


# ------------------------------------------------------------------ genie_find_smems_split
def _inject(reads, rate, seed, values=(4, 78, 255)):
    rng = np.random.default_rng(seed)
    out = reads.copy()
    hit = rng.random(out.shape) < rate
    out[hit] = rng.choice(np.asarray(values, np.uint8), size=int(hit.sum()))
    return out


@pytest.mark.parametrize("rate", [0.0, 0.002, 0.03, 0.2])
def test_find_smems_split(env, rate):
    """No breaks at all (the pass-through to the CSR pipeline), then breaks at several rates, an all-break read and an
    empty read among them."""
    ref = env.main
    from genie_smem_amd import synth
    mat = _inject(synth.reads_from_ref_fast(ref.codes, 300, 151, 41), rate, 42)
    lens = None
    if rate > 0:
        lens = np.random.default_rng(43).integers(1, 152, 300).astype(np.int32)
        lens[3] = 0
        mat[4] = 4
        lens[4] = 151
    want = expect_split(ref, _rows_list(mat, lens), 10)
    total = int(want[0][-1])
    for cap in (total, total - 1, 0):
        res = three(ref, lambda a, s: CC.find_csr(env.lib, ref.ix, a, s, "split", None, mat, lens, 151, 10, cap))
        check_csr(res, want, cap)
    res = three(ref, lambda a, s: CC.find_csr(env.lib, ref.ix, a, s, "split", None, mat, lens, 151, 10, total, with_status=False))
    check_csr(res, want, total, with_status=False)


def test_find_smems_split_many_passes(env):
    """Far more segments than reads, at exactly the workspace the size function returns: several passes (the construction
    of test_split_reads_gpu.py::test_many_passes)."""
    ref = env.main
    from genie_smem_amd import synth
    mat = synth.reads_from_ref_fast(ref.codes, 64, 1000, 111)
    mat[:, ::3] = 4
    mat[0] = synth.reads_from_ref_fast(ref.codes, 1, 1000, 112)[0]
    want = expect_split(ref, _rows_list(mat, None))
    total = int(want[0][-1])
    assert sum(len(SU.segments(r)) for r in mat) > 20 * 64
    for cap in (total, total // 2):
        res = three(ref, lambda a, s: CC.find_csr(env.lib, ref.ix, a, s, "split", None, mat, None, 1000, 1, cap))
        check_csr(res, want, cap)


# ------------------------------------------------------------------ genie_find_smems_long and _long_ex
def _long_batch(ref, breaks):
    from genie_smem_amd import synth
    pool = synth.reads_from_ref_fast(ref.codes, 12, 12_000, 51)
    sizes = [0, 1, 300, 9000, 0, 417, 12_000, 8193, 150, 1, 10_001, 640]
    reads = [pool[i, :L].copy() for i, L in enumerate(sizes)]
    if breaks:
        reads = [_inject(r[None, :], 0.004, 60 + i)[0] for i, r in enumerate(reads)]
        reads[2][:] = 4                              # an all-break read
    return reads


def _long_want(ref, flags, mode, reads, min_len):
    flags = flags or 0
    units = _interleave(reads) if flags & BOTH else reads
    if flags & SPLIT:
        return expect_split(ref, units, min_len)
    return expect_csr(ref, mode, units, min_len if mode == "bwa" else 1)


@pytest.mark.parametrize("flags", [None, 0, BOTH, SPLIT, BOTH | SPLIT])
def test_find_smems_long(env, flags):
    """A ragged batch mixing lengths 0 and 1, a few hundred, and several above 8192, with a nonzero first offset and
    total_bases larger than the last offset."""
    ref = env.main
    reads = _long_batch(ref, bool((flags or 0) & SPLIT))
    modes = ("bwa",) if (flags or 0) & SPLIT else ("bwa", "lut", "rmi")
    for mode in modes:
        min_len = 17 if mode == "bwa" else 1
        want = _long_want(ref, flags, mode, reads, min_len)
        total = int(want[0][-1])
        for cap in ((total, total - 1, 0) if mode == "bwa" else (total,)):
            res = three(ref, lambda a, s: CC.find_long(env.lib, ref.ix, a, s, flags, mode, reads, min_len, cap, first=37, slack=501))
            check_csr(res, want, cap)
    want = _long_want(ref, flags, "bwa", reads, 17)
    total = int(want[0][-1])
    res = three(ref, lambda a, s: CC.find_long(env.lib, ref.ix, a, s, flags, "bwa", reads, 17, total, with_status=False))
    check_csr(res, want, total, with_status=False)


def test_find_smems_long_flagged_reads(env):
    ref = env.no_t
    from genie_smem_amd import synth
    pool = synth.reads_from_ref_fast(ref.codes, 4, 9000, 71)
    reads = [pool[0], pool[1].copy(), pool[2].copy(), pool[3][:5]]
    reads[1][8500] = 7
    reads[2][8999] = 3
    for flags in (None, 0):
        for mode in ("bwa", "lut"):
            want = expect_csr(ref, mode, reads)
            assert want[2].tolist() == [0, 1, 3, 0 if mode == "bwa" else 2]
            total = int(want[0][-1])
            res = three(ref, lambda a, s: CC.find_long(env.lib, ref.ix, a, s, flags, mode, reads, 1, total))
            check_csr(res, want, total)


@pytest.mark.parametrize("flags", [SPLIT, BOTH | SPLIT])
def test_find_smems_long_ex_more_units_than_the_workspace_holds(env, flags):
    """One break in ten positions: about three times the units the size function provides for, so several passes at
    exactly that workspace (the construction of test_long_ex_gpu.py::test_more_units_than_the_workspace_holds, smaller)."""
    ref = env.main
    from genie_smem_amd import synth
    pool = _inject(synth.reads_from_ref_fast(ref.codes, 5, 20_000, 81), 0.1, 82, values=(4,))
    reads = [pool[i, :L] for i, L in enumerate((9000, 300, 9000, 20_000, 9000))]
    strands = 2 if flags & BOTH else 1
    units = strands * sum(len(SU.segments(r)) for r in reads)
    held = strands * len(reads) + strands * sum(len(r) for r in reads) // 32
    assert units > 2 * held
    want = _long_want(ref, flags, "bwa", reads, 1)
    total = int(want[0][-1])
    for cap in (total, total - 1):
        res = three(ref, lambda a, s: CC.find_long(env.lib, ref.ix, a, s, flags, "bwa", reads, 1, cap))
        check_csr(res, want, cap)


# ------------------------------------------------------------------ genie_find_smems_packed and _packed6
@pytest.fixture(scope="module")
def low_complexity(env):
    """A reference in which every A is followed by C: a read 'AG...' ends an SMEM on a single A, whose interval spans more
    than 65535 rows -- escapes in the 8-byte rows as well as in the 6-byte ones."""
    rng = np.random.default_rng(5)
    toks = [np.array(t, np.uint8) for t in ([0, 1], [1], [2], [3])]
    codes = np.concatenate([toks[i] for i in rng.choice(4, 400_000, p=[0.3, 0.2, 0.25, 0.25])])

    return Ref(env.g, env.oracle_mod, codes, k=2, rmi=False)


def _packed_check(res, want, row_bytes, cap_rows, cap_escapes):
    from genie_smem_amd import packing
    off, rows, st = want
    total = int(off[-1])
    top = 0xFFFF if row_bytes == 8 else 0xFF
    wide = np.nonzero(rows[:, 3] - rows[:, 2] >= top)[0]
    wide = wide[wide < cap_rows]                     # a dropped row has no escape
    assert np.array_equal(res["counts8"], np.diff(off).astype(np.uint8))
    assert np.array_equal(res["status8"], st.astype(np.uint8))
    assert res["totals"].tolist() == [total, len(wide)]
    want_esc = {(int(t), int(rows[t, 3])) for t in wide}
    if cap_rows >= total and cap_escapes is not None and cap_escapes >= len(wide):
        goff, grows = packing.unpack_rows(res["counts8"], res["rows"], res["escapes"], row_bytes=row_bytes)
        assert np.array_equal(goff, off) and np.array_equal(grows, rows)
        assert {tuple(e) for e in res["escapes"].tolist()} == want_esc
    else:
        # the rows that fit, span field included; the escapes that fit are some of the true ones
        raw = res["rows"]
        assert raw.shape[0] == min(total, cap_rows)
        got = raw.astype(np.int64)
        assert np.array_equal(got[:, 0], rows[:len(raw), 0]) and np.array_equal(got[:, 1], rows[:len(raw), 1])
        span = np.minimum(rows[:len(raw), 3] - rows[:len(raw), 2], top)
        if row_bytes == 8:
            assert np.array_equal(got[:, 2] | got[:, 3] << 8, span)
            assert np.array_equal(got[:, 4] | got[:, 5] << 8 | got[:, 6] << 16 | got[:, 7] << 24, rows[:len(raw), 2])
        else:
            assert np.array_equal(got[:, 2] | got[:, 3] << 8 | got[:, 4] << 16, rows[:len(raw), 2]) and np.array_equal(got[:, 5], span)
        if "escapes" in res:
            assert {tuple(e) for e in res["escapes"].tolist()} <= want_esc and len(res["escapes"]) == min(len(wide), cap_escapes)


@pytest.mark.parametrize("row_bytes", [8, 6])
def test_find_smems_packed(env, low_complexity, row_bytes):
    """d_counts8, d_status8 and d_totals poisoned, not zeroed; escapes in both row widths; an escape list that is large
    enough, of one entry, and absent; and the same call twice on the same buffers with nothing cleared in between."""
    ref = low_complexity
    rng = np.random.default_rng(6)
    codes = rng.integers(0, 4, (300, 40)).astype(np.uint8)
    codes[:, 0::7] = 0
    codes[:, 1::7] = 2
    lens = rng.integers(2, 41, 300).astype(np.int32)
    lens[:3] = [0, 1, 40]
    for ln in (None, lens):
        want = expect_csr(ref, "bwa", _rows_list(codes, ln))
        total = int(want[0][-1])
        n_esc = int((want[1][:, 3] - want[1][:, 2] >= (0xFFFF if row_bytes == 8 else 0xFF)).sum())
        assert n_esc > 100
        for cap_rows, cap_esc in ((total, n_esc), (total, 1), (total, None), (total - 1, n_esc), (0, 0)):
            partial = ("escapes",) if cap_esc is not None and 0 < cap_esc < n_esc else ()
            res = three(ref, lambda a, s: CC.find_packed(env.lib, ref.ix, a, s, row_bytes, "bwa", codes, ln, 1, cap_rows, cap_esc),
                        partial=partial)
            _packed_check(res, want, row_bytes, cap_rows, cap_esc)
        once = three(ref, lambda a, s: CC.find_packed(env.lib, ref.ix, a, s, row_bytes, "bwa", codes, ln, 1, total, n_esc))
        twice = three(ref, lambda a, s: CC.find_packed(env.lib, ref.ix, a, s, row_bytes, "bwa", codes, ln, 1, total, n_esc, calls=2))
        CC.same(once, twice)


@pytest.mark.parametrize("mode", ["bwa", "lut", "rmi"])
def test_find_smems_packed_modes(env, mode):
    ref = env.main
    from genie_smem_amd import synth
    codes = np.concatenate([synth.reads_from_ref_fast(ref.codes, 300, 150, 91), synth.reads_random(100, 150, 92)])
    lens = np.random.default_rng(93).integers(0, 151, 400).astype(np.int32)
    want = expect_csr(ref, mode, _rows_list(codes, lens), 13 if mode == "bwa" else 1)
    total = int(want[0][-1])
    assert (want[2] == 2).any() == (mode != "bwa")
    for row_bytes in (8, 6):
        res = three(ref, lambda a, s: CC.find_packed(env.lib, ref.ix, a, s, row_bytes, mode, codes, lens, 13 if mode == "bwa" else 1,
                                                     total, 64))
        _packed_check(res, want, row_bytes, total, 64)


# ------------------------------------------------------------------ genie_locate
@pytest.mark.parametrize("stride", [2, 4])
def test_locate(env, stride):
    ref = env.main
    from genie_smem_amd import synth
    sa = ref.o.suffix_array
    reads = _rows_list(np.concatenate([synth.reads_from_ref_fast(ref.codes, 150, 100, 95), synth.reads_random(20, 100, 96)]), None)
    rows = expect_csr(ref, "bwa", reads)[1]
    rng = np.random.default_rng(97)
    rows = rows[rng.permutation(len(rows))[:3000]].copy()
    rows[::9, 2:4] = -1                              # absent
    rows[4::11, 3] = rows[4::11, 2] - 1              # hi < lo
    rows[5, 2:4] = (100, 199)                        # more than 32 rows: copied by the whole wave
    lohi = np.ascontiguousarray(rows[:, 2:4] if stride == 2 else np.concatenate([rows[:, 2:4], rows[:, 0:2]], 1))
    cnt = np.where((rows[:, 2] >= 0) & (rows[:, 3] >= rows[:, 2]), rows[:, 3] - rows[:, 2] + 1, 0)
    off = np.zeros(len(rows) + 1, np.int64)
    off[1:] = np.cumsum(cnt)
    pos = np.concatenate([sa[lo:lo + c] for lo, c in zip(rows[:, 2], cnt) if c]).astype(np.int32)
    total = int(off[-1])
    assert (cnt == 0).sum() > 300 and total > len(rows) // 2
    res = three(ref, lambda a, s: CC.locate(env.lib, ref.ix, a, s, lohi, None))
    assert np.array_equal(res["pos_offsets"], off) and "positions" not in res
    for cap in (total, total - 1, total // 3, 0):
        res = three(ref, lambda a, s: CC.locate(env.lib, ref.ix, a, s, lohi, cap))
        assert np.array_equal(res["pos_offsets"], off) and np.array_equal(res["positions"], pos[:cap])


# ------------------------------------------------------------------ genie_index_create_device and genie_index_validate
@pytest.mark.parametrize("extra", [0, 4096])
@pytest.mark.parametrize("seed_table", [True, False])
def test_index_create_device(env, extra, seed_table):
    """The image written into a 256- but not 512-byte aligned d_image of exactly the bound (and of the bound + 4096), with
    d_tmp of exactly genie_index_device_build_tmp_bytes: the host builder's bytes under all three poisons, nothing written
    past image_cap or past d_tmp, the codes untouched; the device-built handle validates."""
    import torch
    g, lib = env.g, env.lib
    from genie_smem_amd import synth
    codes = synth.synth_ref(20_000, 20_001)
    want = g.GenieIndex.build(codes, K).serialize(seed_table).numpy()
    cap = int(lib.genie_index_device_image_bound(codes.size, K, 7, 0)) + extra
    tmp_bytes = int(lib.genie_index_device_build_tmp_bytes(codes.size, K, 7, 0))
    assert cap > 0 and tmp_bytes > 0
    for poison in POISONS:
        a = Arena("cuda", poison, capacity=cap + tmp_bytes + (1 << 20))
        a.freeze(a.put("codes", codes), "codes")
        image = a.alloc("image", cap, 256)
        a.alloc("tmp", tmp_bytes, 256)
        nbytes, h = C.c_int64(0), C.c_void_p(0)
        rc = lib.genie_index_create_device(C.c_void_p(a.addr("codes")), codes.size, K, 7, 0, 0 if seed_table else 1,
                                           C.c_void_p(a.addr("image")), cap, C.byref(nbytes), C.c_void_p(a.addr("tmp")), tmp_bytes,
                                           torch.cuda.current_device(), C.c_void_p(_stream()), C.byref(h))
        torch.cuda.synchronize()
        assert rc == 0 and nbytes.value == want.size <= cap
        try:
            got = as_numpy(image[:nbytes.value], np.uint8)
            if not np.array_equal(got, want):
                raise AssertionError(f"poison {poison:#04x}: first difference at byte {int(np.flatnonzero(got != want)[0])}")
            a.check()
            a.check_frozen()
            a.freeze(image, "image")
            what = C.c_uint32(0)
            assert lib.genie_index_validate(h, C.byref(what), C.c_void_p(_stream())) == 0 and what.value == 0
            a.check()
            a.check_frozen()
        finally:
            lib.genie_index_destroy(h)


def test_index_validate_leaves_the_image_alone(env):
    import torch
    for ref in (env.main, env.no_t):
        a = Arena("cuda", 0x5A, capacity=1 << 20)
        a.freeze(ref.ix.blob, "index image")
        what = C.c_uint32(7)
        assert env.lib.genie_index_validate(ref.ix._h, C.byref(what), C.c_void_p(_stream())) == 0 and what.value == 0
        torch.cuda.synchronize()
        a.check_frozen()


# ------------------------------------------------------------------ one workspace, many calls
def test_workspace_reuse_across_calls(env, low_complexity):
    """One workspace sized for the largest call and never refilled, used by long_ex (both strands + breaks), csr (LUT,
    short reads), split, packed6 and csr again: each result is what the same call gives on its own freshly poisoned
    workspace."""
    import torch
    ref, lib = env.main, env.lib
    from genie_smem_amd import synth
    long_reads = _long_batch(ref, True)
    short = synth.reads_from_ref_fast(ref.codes, 500, 151, 101)
    broken = _inject(synth.reads_from_ref_fast(ref.codes, 300, 200, 102), 0.02, 103)
    steps = [
        lambda a, s, ws: CC.find_long(lib, ref.ix, a, s, BOTH | SPLIT, "bwa", long_reads, 1, 40_000, first=5, slack=9, ws=ws),
        lambda a, s, ws: CC.find_csr(lib, ref.ix, a, s, "csr", "lut", short, None, 150, 1, 20_000, ws=ws),
        lambda a, s, ws: CC.find_csr(lib, ref.ix, a, s, "split", None, broken, None, 200, 1, 20_000, ws=ws),
        lambda a, s, ws: CC.find_packed(lib, ref.ix, a, s, 6, "rmi", short[:, :150], None, 1, 20_000, 4096, ws=ws),
        lambda a, s, ws: CC.find_csr(lib, ref.ix, a, s, "csr", "lut", short, None, 150, 1, 20_000, ws=ws),
    ]
    alone = []
    for step in steps:
        a = Arena("cuda", 0x5A)
        call = step(a, _stream(), None)
        torch.cuda.synchronize()
        alone.append(call.result())
        a.check()
        n_rows = int(alone[-1]["offsets"][-1] if "offsets" in alone[-1] else alone[-1]["totals"][0])
        assert 0 < n_rows == len(alone[-1]["rows"])          # the capacities above hold every row
    a = Arena("cuda", 0x5A, capacity=64 << 20)
    a.freeze(ref.ix.blob, "index image")
    total = sum(len(r) for r in long_reads) + 14
    big = max(lib.genie_find_smems_long_ex_workspace_bytes(len(long_reads), total, 12_000, BOTH | SPLIT),
              lib.genie_find_smems_workspace_bytes(500, 150), lib.genie_find_smems_split_workspace_bytes(300, 200))
    a.alloc("shared workspace", big, 256)
    ws = (a.addr("shared workspace"), big)
    for i, step in enumerate(steps):
        call = step(a, _stream(), ws)
        torch.cuda.synchronize()
        CC.same(call.result(), alone[i])
        a.check()
        a.check_frozen()
    CC.same(alone[1], alone[4])
