"""GPU tests of the interval kernel of short reads in CSR form (interval_rows_kernel: one lane per row over tiles of at most
256 reads staged in LDS, the batch cut into equal tiles; run with -m gpu on an MI355X).  Expected rows, offsets and status come from the CPU oracle, compared
row by row, on references of a few kb.  The cases are the places where that kernel takes another path: batch sizes around
the tile, counts above the 15 pairs a slot's head holds (later pairs come from the kj row), rows of one read on both sides
of a wave's 64-row chunk, slot geometries of other read lengths, flagged reads (tiles and batches that end in reads without
rows), a row capacity below the total, a reference whose rows mostly take the general search, and the packed, 6-byte and
both-strand entry points, which run the same kernel with other row forms."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 11
TILE, CHUNK, HEAD_PAIRS = 256, 64, 15
READ_OK, READ_BAD_BASE, READ_TOO_SHORT = 0, 1, 2


@pytest.fixture(scope="module")
def env(oracle_mod):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import genie_smem_amd as g
    from genie_smem_amd import synth

    class E:
        pass
    e = E()
    e.g, e.synth, e.lib = g, synth, g._native.lib()
    e.ref = synth.synth_ref(6000, 6000)
    e.ix = g.GenieIndex.build(e.ref, K).to("cuda")
    e.o = oracle_mod.Oracle(e.ref, K)
    # a repeat-rich reference: 8 kb of one 6-mer in tandem, then random bases
    unit = np.asarray([0, 2, 1, 3, 3, 1], np.uint8)
    e.rep_ref = np.concatenate([np.tile(unit, 8000 // 6 + 1)[:8000], synth.synth_ref(4000, 4001)]).astype(np.uint8)
    e.rep_ix = g.GenieIndex.build(e.rep_ref, K).to("cuda")
    e.rep_o = oracle_mod.Oracle(e.rep_ref, K)

    @functools.lru_cache(maxsize=None)
    def thousand(kind):
        """1000 reads of 150 bases of one kind and what the oracle says of them (made once, shared, not changed)."""
        rd = synth.reads_from_ref(e.ref, 1000, 150, 7) if kind == "fromref" else synth.reads_random(1000, 150, 8)
        counts, want = e.o.find_smems_batch("lut", rd, nthreads=8)
        return rd, counts, want
    e.thousand = thousand
    return e


def _expected(o, mode, reads, lens=None, bad=()):
    """(offsets, rows, status) the CSR call has to return: the oracle's rows; reads in `bad` hold a code > 3."""
    n, L = reads.shape
    clean = reads.copy()
    clean[clean > 3] = 0
    counts, want = o.find_smems_batch(mode, clean, nthreads=8, lens=lens)
    ln = np.full(n, L, np.int64) if lens is None else np.asarray(lens, np.int64)
    status = np.zeros(n, np.int32)
    if mode != "bwa":
        status[ln < K] = READ_TOO_SHORT
    status[list(bad)] = READ_BAD_BASE
    assert (counts[(status == READ_OK)] >= 0).all()                   # every base occurs in these references
    counts = np.where(status == READ_OK, counts, 0)
    return _csr(counts, want), status


def _csr(counts, want):
    off = np.zeros(len(counts) + 1, np.int64)
    np.cumsum(counts, out=off[1:])
    rows = np.concatenate([np.zeros((0, 4), np.int32)] + [want[r, :counts[r]] for r in range(len(counts))])
    return off, rows


def _same(got, off, rows, status=None):
    g_off, g_rows = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert np.array_equal(g_off, off)
    assert g_rows.shape == rows.shape
    differ = np.flatnonzero((g_rows != rows).any(axis=1))
    assert differ.size == 0, (differ[:5], g_rows[differ[:5]], rows[differ[:5]])
    if status is not None:
        assert np.array_equal(got[2].cpu().numpy(), status)


def _crosses_chunk(off, tile):
    """Some read's rows lie on both sides of a 64-row chunk boundary of its tile's rows, the tiles being `tile` reads."""
    for t0 in range(0, len(off) - 1, tile):
        rel = off[t0:min(t0 + tile, len(off) - 1) + 1] - off[t0]
        first, last = rel[:-1], rel[1:] - 1
        if ((last >= first) & (first // CHUNK != last // CHUNK)).any():
            return True
    return False


@pytest.mark.parametrize("kind", ["fromref", "random"])
@pytest.mark.parametrize("n", [1, 63, 255, 256, 257, 1000])
def test_batch_sizes_around_the_tile(env, kind, n):
    rd, counts, want = env.thousand(kind)
    off, rows = _csr(counts[:n], want[:n])
    if kind == "random":
        assert counts[:n].max() > HEAD_PAIRS                         # pairs behind the slot's head: from the kj row
    if n >= 63:                                                      # whichever tile size of 63 .. 256 reads the launch picks
        assert all(_crosses_chunk(off, tile) for tile in range(63, TILE + 1))
    _same(env.ix.find_smems("lut", rd[:n]), off, rows, np.zeros(n, np.int32))


@pytest.mark.parametrize("L", [16, 255])
def test_other_fixed_lengths(env, L):
    rd = np.concatenate([env.synth.reads_from_ref(env.ref, 200, L, L), env.synth.reads_random(100, L, L + 1)])
    (off, rows), status = _expected(env.o, "lut", rd)
    assert off[-1] > 300
    _same(env.ix.find_smems("lut", rd), off, rows, status)


def test_mixed_lengths(env):
    rd = env.synth.reads_from_ref(env.ref, 300, 200, 21)
    lens = np.random.default_rng(22).integers(0, 201, 300).astype(np.int32)
    lens[[0, 17, 255, 256, 299]] = 0
    lens[[1, 257]] = 200
    for mode in ("bwa", "lut"):
        (off, rows), status = _expected(env.o, mode, rd, lens)
        _same(env.ix.find_smems(mode, rd, lens=lens), off, rows, status)


def test_flagged_reads(env):
    """A bad base, reads shorter than K (LUT mode), both among good reads; a whole tile of flagged reads (its rows: none);
    the last read of the batch flagged (the total is written all the same)."""
    n, L = 4 * TILE + 40, 100
    rd = env.synth.reads_from_ref(env.ref, n, L, 31)
    lens = np.full(n, L, np.int32)
    # reads 256 .. 767 are all flagged: 512 in a row hold a whole tile however the batch is cut into tiles of at most 256
    bad = list(range(3, TILE, 5)) + list(range(TILE, 3 * TILE, 2)) + [n - 1]
    short = [r for r in range(4, TILE, 7) if r not in bad] + list(range(TILE + 1, 3 * TILE, 2))
    for r in bad:
        rd[r, (r * 13) % L] = 4 + r % 3
    lens[short] = np.arange(len(short)) % K
    lens[n - 1] = L
    (off, rows), status = _expected(env.o, "lut", rd, lens, bad)
    assert (status[TILE:3 * TILE] != READ_OK).all() and off[TILE] == off[3 * TILE] and status[n - 1] == READ_BAD_BASE
    assert set(status.tolist()) == {READ_OK, READ_BAD_BASE, READ_TOO_SHORT} and off[-1] > off[3 * TILE] > 0
    _same(env.ix.find_smems("lut", rd, lens=lens), off, rows, status)
    # only flagged reads: an empty CSR
    got = env.ix.find_smems("lut", rd[TILE:2 * TILE], lens=lens[TILE:2 * TILE])
    _same(got, np.zeros(TILE + 1, np.int64), np.zeros((0, 4), np.int32), status[TILE:2 * TILE])


def test_row_capacity_below_the_total(env):
    """Guarded buffers: the rows up to the capacity are right, nothing behind it is written, the offsets are complete."""
    import torch
    import contract_calls as CC
    from guarded import Arena
    rd, counts, want = env.thousand("random")
    n = 600
    off, rows = _csr(counts[:n], want[:n])
    total = int(off[-1])
    for cap in (total // 2 + 3, 1, off[TILE] - 1):                   # inside a tile's rows; one row; one short of a tile's end
        cap = int(cap)
        a = Arena("cuda", 0x5A)
        call = CC.find_csr(env.lib, env.ix, a, torch.cuda.current_stream().cuda_stream, "csr", "lut", rd[:n], None, 150, 1, cap)
        torch.cuda.synchronize()
        res = call.result()                                          # (asserts the poison behind row `cap`)
        a.check()
        a.check_frozen()
        assert np.array_equal(res["offsets"], off) and np.array_equal(res["rows"], rows[:cap])
        assert not res["status"].any()


def _repeat_batch(env):
    rng = np.random.default_rng(41)
    n, L = 700, 150
    rd = np.stack([env.rep_ref[p:p + L] for p in rng.integers(0, 8000 - L, n)]).astype(np.uint8)
    at = rng.integers(0, L, (n, 3))                                  # three substitutions per read: several rows each
    for r in range(n):
        rd[r, at[r]] = (rd[r, at[r]] + 1 + rng.integers(0, 3, 3)) & 3
    return rd


def test_repeat_rich_reference(env):
    rd = _repeat_batch(env)
    (off, rows), status = _expected(env.rep_o, "lut", rd)
    wide = rows[:, 3] - rows[:, 2] >= 7                              # more rows than any table entry describes
    assert wide.sum() * 2 > len(rows)
    # a wave takes every eighth 64-row chunk of a tile and searches its list when 64 rows wait: that happens inside a tile
    tile_rows = wide[off[0]:off[TILE]]
    per_wave = [sum(int(tile_rows[c:c + CHUNK].sum()) for c in range(CHUNK * w, len(tile_rows), CHUNK * 8)) for w in range(8)]
    assert max(per_wave) >= 64
    _same(env.rep_ix.find_smems("lut", rd), off, rows, status)


@pytest.mark.parametrize("which", ["plain", "repeat"])
def test_other_entry_points_equal_the_csr_call(env, which):
    from genie_smem_amd import packing
    if which == "plain":
        ix, rd = env.ix, np.concatenate([env.thousand("fromref")[0][:300], env.thousand("random")[0][:300]])
    else:
        ix, rd = env.rep_ix, _repeat_batch(env)
    off, rows, st = (x.cpu().numpy() for x in ix.find_smems("lut", rd))
    span = rows[:, 3].astype(np.int64) - rows[:, 2]
    for rb, top in ((8, 0xFFFF), (6, 0xFF)):
        c8, s8, r8, esc = ix.find_smems_packed("lut", packing.pack_reads(rd), 150, row_bytes=rb)
        esc = esc.cpu().numpy()
        want_esc = {(int(i), int(rows[i, 3])) for i in np.flatnonzero(span >= top)}
        assert {tuple(x) for x in esc.tolist()} == want_esc and len(esc) == len(want_esc)
        if which == "repeat" and rb == 6:
            assert want_esc
        off2, rows2 = packing.unpack_rows(c8.cpu().numpy(), r8.cpu().numpy(), esc, row_bytes=rb)
        assert np.array_equal(off2, off) and np.array_equal(rows2, rows) and np.array_equal(s8.cpu().numpy(), st)
    both = np.empty((2 * len(rd), 150), np.uint8)
    both[0::2], both[1::2] = rd, packing.reverse_complement(rd)
    want = ix.find_smems("lut", both)
    got = ix.find_smems_both("lut", rd)
    _same(got, want[0].cpu().numpy(), want[1].cpu().numpy(), want[2].cpu().numpy())
