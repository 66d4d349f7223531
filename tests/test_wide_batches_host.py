"""Host tests of tests/wide_util.py (no GPU): the tiling rule that test_wide_batches_gpu.py relies on, proved against the brute
force -- for every call and flag set the brute force of c = 3 copies of a tiny block is the brute force of the block, tiled by
the very checkers the GPU tests apply to the device's output -- and, by arithmetic alone, that every shape of the GPU tests
crosses the threshold it is named for."""
import numpy as np
import pytest

import lookup_util as U
import text_util as TU
import fasta_util as FU
import wide_util as W

BOTH, SPLIT = W.BOTH, W.SPLIT
FAMILY = U.family()
C3 = 3


def _tiny(name, open_end=False):
    """A few reads of every kind the wide blocks hold, small enough for the brute force of three copies: tiny reads with
    their empties and flagged ones, and reads full of breaks (open_end: the last one ends without a break)."""
    reads = W.a1_block(name)[:24] + W.a2_block(name, segments=40, reads=3, open_end=open_end)
    if sum(len(r) for r in reads) % 2 == 0:
        reads.insert(0, FAMILY[name][:1].copy())
    if open_end:
        assert reads[-1][-1] < 4 and reads[-1][-1] in FAMILY[name]
    return reads


def _wide_reads(reads):
    bases, off = W.csr(reads)
    wb, wo = W.tile_csr(bases, off, C3)
    wb, wo = wb.numpy(), wo.numpy()
    assert wb.size == C3 * bases.size and np.array_equal(wo[len(reads):2 * len(reads) + 1], off + bases.size)
    return [wb[wo[i]:wo[i + 1]] for i in range(C3 * len(reads))]


@pytest.mark.parametrize("open_end", [False, True])
@pytest.mark.parametrize("name", ["rand4096", "noT"])
def test_tiling_rule_against_brute_force(name, open_end):
    ref = FAMILY[name]
    reads = _tiny(name, open_end)
    wide = _wide_reads(reads)
    for mode, flags in (("bwa", 0), ("lut", 0), ("bwa", BOTH), ("lut", BOTH), ("bwa", SPLIT), ("bwa", BOTH | SPLIT)):
        blk, wid = W.brute_smems(ref, reads, mode, flags), W.brute_smems(ref, wide, mode, flags)
        assert blk[1].shape[0] > 0
        W.assert_tiled_csr(W.to_torch(wid), W.to_torch(blk), C3, f"smems {mode} {flags}")
    for flags in (0, BOTH, SPLIT, BOTH | SPLIT):
        blk, wid = W.brute_match_stats(ref, reads, flags), W.brute_match_stats(ref, wide, flags)
        W.assert_tiled_all(W.to_torch(wid), W.to_torch(blk), C3, f"match_stats {flags}", ("ms", "lohi", "status"))
        if flags & BOTH:                                             # copy k owns the virtual positions [2 k Lb, 2 (k + 1) Lb)
            Lb = sum(len(r) for r in reads)
            assert blk[0].size == 2 * Lb and np.array_equal(wid[0][2 * Lb:4 * Lb], blk[0])
    for flags in (0, BOTH):
        blk, wid = W.brute_exact(ref, reads, flags), W.brute_exact(ref, wide, flags)
        W.assert_tiled_all(W.to_torch(wid), W.to_torch(blk), C3, f"exact_match {flags}", ("lohi", "counts", "status"))


def test_the_checkers_notice_a_wrong_copy():
    """One element of one copy changed, one offset off by one: each checker fails and names the copy."""
    import torch
    block = torch.arange(35, dtype=torch.int32).reshape(7, 5)
    wide = block.repeat(4, 1)
    assert W.first_bad_copy(wide, block, 4) is None and W.first_bad_copy(wide, block, 4, budget=40) is None
    wide[2 * 7 + 3, 4] += 1
    assert W.first_bad_copy(wide, block, 4) == 2 and W.first_bad_copy(wide, block, 4, budget=40) == 2
    off = torch.tensor([0, 2, 2, 9], dtype=torch.int64)
    good = torch.tensor([0, 2, 2, 9, 11, 11, 18, 20, 20, 27], dtype=torch.int64)
    W.assert_tiled_offsets(good, off, 3, "offsets")
    for at in (4, 9):
        bad = good.clone()
        bad[at] -= 1
        with pytest.raises(AssertionError):
            W.assert_tiled_offsets(bad, off, 3, "offsets")


@pytest.mark.parametrize("name", ["rand4096", "noT"])
def test_shape_a_crosses_the_launch_limit(name):
    """A1: more than 2^24 reads, so one block of 256 threads per window is 2^32 threads or more; with 16 400 copies more than
    2^26 reads, so one block per four windows is, too.  A2: more than 2^24 units from breaks alone."""
    ref = FAMILY[name]
    reads = W.a1_block(name)
    lens = [len(r) for r in reads]
    assert len(reads) == W.A1_READS and set(lens) == set(range(6)) and sum(lens) % 2 == 1
    assert any((r > 3).any() for r in reads)
    assert name != "noT" or any((r == 3).any() for r in reads)
    n, total = W.A1_READS * W.A1_COPIES, sum(lens) * W.A1_COPIES
    assert n == 16_805_900 > 1 << 24
    for strands in (1, 2):
        assert W.walk_threads(strands * total, strands * n) >= W.LAUNCH_LIMIT
    assert W.fwd_threads(total, n) < W.LAUNCH_LIMIT                 # the four-window launch still fits here ...
    n, total = W.A1_READS * W.A1_COPIES_FWD, sum(lens) * W.A1_COPIES_FWD
    assert n == 67_223_600 > 1 << 26
    assert W.fwd_threads(total, n) >= W.LAUNCH_LIMIT                # ... and no longer here
    # one block short of the limit fits: the limit is the product reaching 2^32, not the block count leaving 24 bits
    assert ((1 << 24) - 1) * W.WINDOW < W.LAUNCH_LIMIT <= (1 << 24) * W.WINDOW

    blk = W.a2_block(name)
    total = sum(len(r) for r in blk)
    assert total % 2 == 1 and 8000 < total < 16000
    assert all(r[0] > 3 or r[0] not in ref for r in blk) and all(r[-1] > 3 or r[-1] not in ref for r in blk)
    assert W.forward_segments(ref, blk) == W.A2_SEGMENTS
    units = W.A2_SEGMENTS * W.A2_COPIES
    assert units == 16_810_000 > 1 << 24
    assert W.walk_threads(total * W.A2_COPIES, units) >= W.LAUNCH_LIMIT
    # the minimum workspace holds the strand-reads and one unit per 32 positions: fewer than the units, so the GPU test sizes
    # its workspace for `units` reads to keep them in one pass
    assert len(blk) * W.A2_COPIES + total * W.A2_COPIES // 32 < units


def test_shape_b_crosses_31_and_32_bits():
    from genie_smem_amd import synth
    total = W.B_BASES * W.B_COPIES
    assert W.B_BASES % 2 == 1 and total == 2_149_656_650 > 1 << 31
    assert 2 * total == 4_299_313_300 > 1 << 32
    assert total - W.B_BASES > 1 << 31 and 2 * (total - W.B_BASES) > 1 << 32       # a whole copy lies beyond each boundary
    reads = W.b_block(synth.synth_ref(W.B_REF, W.B_REF))
    lens = np.asarray([len(r) for r in reads])
    assert lens.sum() == W.B_BASES and (lens == 150).sum() == 3000 and lens.max() == 300_000
    assert ((lens >= 1000) & (lens <= 20000)).sum() >= 12 and sum((r > 3).any() for r in reads) == 1
    # both strands: more than 2^24 windows, so the one-block-per-window launches are cut here as well
    assert W.walk_threads(2 * total, 2 * len(reads) * W.B_COPIES) >= W.LAUNCH_LIMIT
    # locate: more than 2^31 positions from 2100 intervals of all n + 1 rows
    assert (W.LOCATE_N + 1) * W.LOCATE_COPIES > 1 << 31
    assert (W.LOCATE_N + 1) * (W.LOCATE_COPIES - 1) > 1 << 31


def test_text_blocks_cross_31_bits():
    """Whole records, odd length, and 2100 copies put the text's bytes and the bases behind them past 2^31."""
    text = W.lines_block()
    status, out5, offs, bases = TU.parse(text, TU.LINES)
    assert status == TU.OK and out5[3] == len(text) and out5[2] == 100_000 and 0 in np.diff(offs)
    assert len(text) % 2 == 1 and len(text) * W.TEXT_COPIES > 1 << 31 and out5[1] * W.TEXT_COPIES > 1 << 31
    # the rule for text: the tiled text parses to the tiled bases, offsets shifted by the block's bases
    st3, out3, offs3, bases3 = TU.parse(text * C3, TU.LINES)
    assert out3 == [C3 * out5[0], C3 * out5[1], out5[2], C3 * out5[3], -1]
    W.assert_tiled(*W.to_torch((bases3, bases)), C3, "lines bases")
    W.assert_tiled_offsets(*W.to_torch((offs3, offs)), C3, "lines offsets")

    text = W.fasta_block()
    status, out5, offs, bases, starts = FU.parse(text)
    assert status == FU.OK and out5[3] == len(text) and out5[2] == 200_000 and 0 in np.diff(offs)
    assert len(text) % 2 == 1 and len(text) * W.TEXT_COPIES > 1 << 31 and out5[1] * W.TEXT_COPIES > 1 << 31
    st3, out3, offs3, bases3, starts3 = FU.parse(text * C3)
    assert out3 == [C3 * out5[0], C3 * out5[1], out5[2], C3 * out5[3], -1]
    W.assert_tiled(*W.to_torch((bases3, bases)), C3, "fasta bases")
    W.assert_tiled_offsets(*W.to_torch((offs3, offs)), C3, "fasta offsets")
    W.assert_tiled_offsets(*W.to_torch((np.append(starts3, C3 * len(text)), np.append(starts, len(text)))), C3, "fasta record starts")
