"""GPU tests of genie_find_smems_long (run with -m gpu on an MI355X): SMEMs of reads of any length, given as CSR, against
the CPU oracle (bit-exact), against genie_find_smems_csr on the reads that call accepts (byte for byte), and through the
drop-in per-query API on queries longer than GENIE_MAX_READ_LEN."""
import numpy as np
import pytest

import golden_util as G

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


def _ref(pkg, oracle_mod, name):
    """(codes, GenieIndex on the device with an RMI model, Oracle) of a synthetic reference or a golden one (K = 15)."""
    if name not in _REFS:
        from genie_smem_amd import synth
        if name == "big100k_K15":
            codes = G.load(name)[0]["ref_codes"].astype(np.uint8)
        else:
            codes = synth.synth_ref(name, name)
        ix = pkg.GenieIndex.build(codes, 15)
        ix.train_rmi([100])
        _REFS[name] = (codes, ix.to("cuda"), oracle_mod.Oracle(codes, 15))
    return _REFS[name]


def _csr(reads):
    offs = np.zeros(len(reads) + 1, np.int64)
    offs[1:] = np.cumsum([len(r) for r in reads])
    bases = np.concatenate(reads).astype(np.uint8) if reads else np.zeros(0, np.uint8)
    return bases, offs


def _long(ix, mode, reads, min_len=1, rows_hint=None):
    bases, offs = _csr(reads)
    off, sm, st = ix.find_smems_long(mode, bases, offs, min_len, rows_hint=rows_hint)
    return off.cpu().numpy(), sm.cpu().numpy(), st.cpu().numpy()


_ORC = {}


def _oracle_rows(o, read, min_len):
    """The oracle's BWA rows, remembered: its cost grows with the square of a verbatim match's length (about 40 s for one
    of 70 kb), so the verbatim cases below are sized by it and every answer is computed once."""
    key = (id(o), hash(read.tobytes()), read.size, min_len)
    if key not in _ORC:
        _ORC[key] = o.find_smems("bwa", read, min_len)
    return _ORC[key]


def _check_oracle(ix, o, mode, reads, min_len=1):
    off, sm, st = _long(ix, mode, reads, min_len)
    assert off[0] == 0 and off[-1] == sm.shape[0]
    for r, read in enumerate(reads):
        assert st[r] == 0, (r, st[r])
        # LUT / RMI give get_SMEMS's rows (min_len ignored); the oracle's BWA traversal is the specification
        rc, want = _oracle_rows(o, read, min_len if mode == "bwa" else 1)
        assert rc >= 0
        got = sm[off[r]:off[r + 1]]
        assert got.shape == want.shape and (got == want).all(), (r, len(read))
    return off, sm


def _mosaic(codes, length, seed, lo=3000, hi=70000, first=None):
    """A read made of verbatim pieces of the reference, lo .. hi bases each (the first `first` bases long if given)."""
    rng = np.random.default_rng(seed)
    parts, have = [], 0
    while have < length:
        s = first if (first and not parts) else int(rng.integers(lo, hi + 1))
        s = min(s, len(codes) - 1)
        p = int(rng.integers(0, len(codes) - s))
        parts.append(codes[p:p + s])
        have += s
    return np.concatenate(parts)[:length].astype(np.uint8)


def _from_ref(codes, length, seed):
    from genie_smem_amd import synth
    return synth.reads_from_ref_fast(codes, 1, length, seed)[0]


LENGTHS = [8193, 20000, 65535, 65536, 65537, 200000]


@pytest.mark.parametrize("name", [100_000, 1_000_000, "big100k_K15"])
def test_lengths_vs_oracle_all_modes(pkg, oracle_mod, name):
    codes, ix, o = _ref(pkg, oracle_mod, name)
    reads = [_from_ref(codes, L, 7 + i) for i, L in enumerate(LENGTHS)]
    reads.append(np.random.default_rng(5).integers(0, 4, 30000).astype(np.uint8))
    for mode in ("bwa", "lut", "rmi"):
        _check_oracle(ix, o, mode, reads)
    _check_oracle(ix, o, "bwa", reads, min_len=20)


@pytest.mark.parametrize("name", [100_000, 1_000_000])
def test_million_base_read(pkg, oracle_mod, name):
    codes, ix, o = _ref(pkg, oracle_mod, name)
    reads = [_from_ref(codes, 1_000_000, 99)]
    if name == 1_000_000:
        reads.append(_mosaic(codes, 1_000_000, 98, 3000, 4000))       # verbatim pieces across ~4000 windows
    _check_oracle(ix, o, "bwa", reads)
    _check_oracle(ix, o, "bwa", reads[:1], min_len=20)


@pytest.mark.parametrize("name", [100_000, 1_000_000, "big100k_K15"])
def test_verbatim_pieces(pkg, oracle_mod, name):
    codes, ix, o = _ref(pkg, oracle_mod, name)
    # 3 .. 70 kb pieces; on the 100 kb synthetic reference one of 66 000 bases: an SMEM and fwd values above 65 535
    big = name == 100_000
    reads = [_mosaic(codes, 100_000 if big else 120_000, 40, 3000, 12000 if big else 22000, first=66000 if big else 30000)]
    off, sm = _check_oracle(ix, o, "bwa", reads)
    if big:
        assert (sm[:, 1] - sm[:, 0]).max() > 65535
    _check_oracle(ix, o, "lut", reads)
    if not big:                                                  # (the oracle needs ~40 s per pass over the 66 kb piece)
        _check_oracle(ix, o, "bwa", reads, min_len=20)


def test_ragged_batch_matches_csr(pkg, oracle_mod):
    from genie_smem_amd import synth
    codes, ix, o = _ref(pkg, oracle_mod, 100_000)
    rng = np.random.default_rng(3)
    short_lens = [0, 1, 2, 14, 15, 16, 31, 32, 33, 150, 255, 256, 257, 1000, 4095, 8191, 8192] + \
        [int(x) for x in rng.integers(0, 8193, 40)]
    pool = synth.reads_from_ref_fast(codes, len(short_lens), 8192, 4)
    shorts = [pool[i, :L].copy() for i, L in enumerate(short_lens)]
    longs = [_from_ref(codes, 30000, 8), _mosaic(codes, 40000, 9, 3000, 8000)]
    reads = shorts[:20] + [longs[0]] + shorts[20:] + [longs[1]]
    where = [i for i, r in enumerate(reads) if len(r) <= 8192]
    strided = np.zeros((len(where), 8192), np.uint8)
    lens = np.zeros(len(where), np.int32)
    for j, i in enumerate(where):
        strided[j, :len(reads[i])] = reads[i]
        lens[j] = len(reads[i])
    for mode, ml in (("bwa", 1), ("bwa", 20), ("lut", 1), ("rmi", 1)):
        off, sm, st = _long(ix, mode, reads, ml)
        coff, csm, cst = (t.cpu().numpy() for t in ix.find_smems(mode, strided, lens, ml))
        for j, i in enumerate(where):
            assert st[i] == cst[j], (mode, i, len(reads[i]))
            assert sm[off[i]:off[i + 1]].tobytes() == csm[coff[j]:coff[j + 1]].tobytes(), (mode, i, len(reads[i]))
        for i in (20, len(reads) - 1):
            rc, want = _oracle_rows(o, reads[i], ml if mode == "bwa" else 1)
            assert (sm[off[i]:off[i + 1]] == want).all()


def test_bad_and_absent_bases(pkg, oracle_mod):
    codes, ix, o = _ref(pkg, oracle_mod, 100_000)
    good = _from_ref(codes, 20000, 11)
    bad = good.copy()
    bad[12345] = 4
    bad_end = good.copy()
    bad_end[-1] = 7
    off, sm, st = _long(ix, "bwa", [good, bad, bad_end, good[:10]])
    assert st.tolist() == [0, 1, 1, 0]
    assert off[2] == off[1] and off[3] == off[2]
    _, st_lut = _long(ix, "lut", [good[:10]])[1:]
    assert st_lut.tolist() == [2]                                  # shorter than K in LUT mode
    # a reference without T: every read holding a T is an absent-base read
    rng = np.random.default_rng(2)
    ref = rng.integers(0, 3, 50000).astype(np.uint8)
    ix2 = pkg.GenieIndex.build(ref, 15).to("cuda")
    o2 = oracle_mod.Oracle(ref, 15)
    r_ok = ref[1000:21000].copy()
    r_abs = r_ok.copy()
    r_abs[15000] = 3
    off, sm, st = _long(ix2, "bwa", [r_ok, r_abs, r_ok])
    assert st.tolist() == [0, 3, 0]
    assert off[2] == off[1]
    rc, want = o2.find_smems("bwa", r_ok)
    assert (sm[off[0]:off[1]] == want).all() and (sm[off[2]:off[3]] == want).all()


def test_row_capacity_overflow(pkg, oracle_mod):
    codes, ix, o = _ref(pkg, oracle_mod, 100_000)
    reads = [_from_ref(codes, 20000, 21), _from_ref(codes, 9000, 22)]
    full = _long(ix, "bwa", reads)
    small = _long(ix, "bwa", reads, rows_hint=5)                    # reruns with the exact size
    assert (full[0] == small[0]).all() and (full[1] == small[1]).all()
    import torch
    bases, offs = _csr(reads)
    total = int(full[0][-1])
    cap = total // 3
    b = torch.as_tensor(bases).cuda()
    of = torch.as_tensor(offs).cuda()
    lib = pkg._native.lib()
    ws_bytes = lib.genie_find_smems_long_workspace_bytes(2, len(bases), 20000)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    out_off = torch.empty(3, dtype=torch.int64, device="cuda")
    rows = torch.full((cap + 4, 4), -7, dtype=torch.int32, device="cuda")
    st = torch.empty(2, dtype=torch.int32, device="cuda")
    import ctypes as C
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = lib.genie_find_smems_long(ix._h, 0, p(b), p(of), 2, len(bases), 20000, 1, p(out_off), p(rows), cap, p(st), p(ws),
                                   ws_bytes, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    assert out_off.cpu().numpy().tolist() == full[0].tolist()
    r = rows.cpu().numpy()
    assert (r[:cap] == full[1][:cap]).all() and (r[cap:] == -7).all()


def test_invalid_offsets(pkg, oracle_mod):
    import ctypes as C
    import torch
    codes, ix, o = _ref(pkg, oracle_mod, 100_000)
    lib = pkg._native.lib()
    bases = torch.as_tensor(_from_ref(codes, 30000, 31)).cuda()
    ws_bytes = lib.genie_find_smems_long_workspace_bytes(3, 30000, 20000)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    out_off = torch.empty(4, dtype=torch.int64, device="cuda")
    rows = torch.empty((1000, 4), dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for offs in ([0, 100, 50, 30000],            # decreasing
                 [0, 100, 200, 30001],           # past total_bases
                 [-5, 100, 200, 300],            # negative
                 [0, 25000, 26000, 27000]):      # a read longer than max_len
        of = torch.as_tensor(np.asarray(offs, np.int64)).cuda()
        rc = lib.genie_find_smems_long(ix._h, 0, p(bases), p(of), 3, 30000, 20000, 1, p(out_off), p(rows), 1000, None, p(ws),
                                       ws_bytes, s)
        assert rc == -1, offs
    of = torch.as_tensor(np.asarray([0, 100, 20100, 30000], np.int64)).cuda()
    rc = lib.genie_find_smems_long(ix._h, 0, p(bases), p(of), 3, 30000, 20000, 1, p(out_off), p(rows), 1000, None, p(ws),
                                   ws_bytes, s)
    assert rc == 0


def test_locate_on_long_read_rows(pkg, oracle_mod):
    codes, ix, o = _ref(pkg, oracle_mod, 1_000_000)
    read = _mosaic(codes, 200000, 51, lo=3000, hi=20000)
    off, sm, st = ix.find_smems_long("bwa", read, np.asarray([0, len(read)], np.int64))
    pos_off, pos = ix.locate(sm[:, 2:4])
    pos_off, pos, sm = pos_off.cpu().numpy(), pos.cpu().numpy(), sm.cpu().numpy()
    sa = o.suffix_array
    for j in range(sm.shape[0]):
        s, e, lo, hi = sm[j].tolist()
        want = sorted(int(sa[r]) for r in range(lo, hi + 1))          # 1-based, as locate
        got = sorted(pos[pos_off[j]:pos_off[j + 1]].tolist())
        assert got == want, j
        assert (codes[want[0] - 1:want[0] - 1 + e - s] == read[s:e]).all()


def test_dropin_long_query(pkg, oracle_mod):
    from genie_smem_amd import synth
    codes = synth.synth_ref(100_000, 100_000)
    ref = G.codes_to_str(codes)
    qcodes = _from_ref(codes, 20000, 61)
    query = G.codes_to_str(qcodes)
    m = pkg.ExactMatch("long.fa")
    m.set_reference(ref)
    sm = pkg.SMEM(m, 15)
    o = oracle_mod.Oracle(codes, 15)
    for ml in (1, 20):
        rc, rows = o.find_smems("bwa", qcodes, ml)
        want = {query[s:e]: (int(lo), int(hi)) for s, e, lo, hi in rows.tolist()}
        assert sm.get_SMEMS(query, ml) == want
        if ml == 1:
            assert sm.get_smems_lut(query) == want
