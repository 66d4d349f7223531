"""GPU: mate rescue through SMEM.map_pairs(rescue=True), on the 16 kb three-contig reference of tests/test_pair_gpu.py with
minimum_length 19.  A mate with a substitution every 13 bases has no exact run above 12 bases and so no record; seeded again
with min_len 12 in the window next to its partner it is found, the pair is proper, its CIGAR carries the X ops and NM counts the
substitutions -- with the partner on strand 0 (the RIGHT window) and on strand 1 (the LEFT window).  The same mate 5 kb away, a
random mate, and a mate whose only copy lies across the contig boundary from a clamped window stay unmapped.  Pairs that were
proper in the first pass keep their records and SAM rows, and a batch without a target returns what rescue=False returns.  What
each case must give -- windows, places, flags, CIGAR text -- is worked out on the CPU from the planted reads before the GPU is
asked; the windows also come from the planner's brute force of tests/window_util.py."""
import numpy as np
import pytest

import align_util as AU
import window_util as WU

pytestmark = pytest.mark.gpu

N_REF = 1 << 14
TABLE = np.asarray([0, 6000, 12000, N_REF], np.int64)
MIN_LEN = 19
EVERY = 13
END_BONUS = 5                                                        # align_chains' default: an extension that reaches its end gets it


def _text(q):
    return "".join("ACGT"[c] for c in q)


def _diverged(piece):
    """A substitution at every 13th base: the longest exact run has 12 bases -> (read, substitutions, CIGAR against the piece)."""
    q = np.asarray(piece, np.uint8).copy()
    at = np.arange(EVERY - 1, q.size, EVERY)
    q[at] = (q[at] + 1) % 4
    tail = q.size - (int(at[-1]) + 1)
    return q, at.size, f"{EVERY - 1}=1X" * at.size + (f"{tail}=" if tail else "")


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import genie_smem_amd as g

    class Env:
        pass
    e = Env()
    e.g = g
    T = np.random.default_rng(50).integers(0, 4, N_REF).astype(np.uint8)
    T[9000:9300] = T[2000:2300]                                     # two exact copies of a 300-base segment
    e.T = T
    m = g.ExactMatch("rescue_planted.fa")
    m.set_reference(_text(T))
    e.sm, e.rs = g.SMEM(m, 4), g.ReferenceSet(["a", "b", "c"], TABLE, T)
    near, e.subs, e.cigar = _diverged(T[750:900])
    far = _diverged(T[5200:5350])[0]
    over = _diverged(T[6050:6200])[0]
    left = _diverged(T[12500:12650])[0]
    rand = np.random.default_rng(94).integers(0, 4, 150).astype(np.uint8)
    e.reads = [T[3000:3150].copy(), AU.revcomp(T[3250:3400]),        # 0 proper in the first pass
               T[500:650].copy(), AU.revcomp(near),                  # 1 rescued in the RIGHT window of a strand-0 partner
               left, AU.revcomp(T[12750:12900]),                     # 2 rescued in the LEFT window of a strand-1 partner
               T[200:350].copy(), AU.revcomp(far),                   # 3 the diverged mate 5 kb away: outside the window
               T[13000:13150].copy(), rand,                          # 4 a random mate
               T[5700:5850].copy(), AU.revcomp(over),                # 5 the diverged mate's only copy lies in the next contig
               T[2050:2200].copy(), AU.revcomp(T[9400:9550])]        # 6 proper in the first pass through the duplication
    e.strs = [_text(q) for q in e.reads]
    return e


def _np(t):
    import torch
    return (t.view(torch.int32) if t.dtype == torch.uint32 else t).cpu().numpy()


def _same_but_chain(rec_a, sam_a, lo_a, rec_b, sam_b, lo_b, n):
    """n records from lo_a of one run equal those from lo_b of another in every column but the chain index, the mate's record
    index taken relative to the pair's first record."""
    keep = [c for c in range(12) if c != 1]
    assert np.array_equal(rec_a[lo_a:lo_a + n][:, keep], rec_b[lo_b:lo_b + n][:, keep])
    a, b = sam_a[lo_a:lo_a + n].copy(), sam_b[lo_b:lo_b + n].copy()
    a[:, 2] -= np.where(a[:, 2] >= 0, lo_a, 0)
    b[:, 2] -= np.where(b[:, 2] >= 0, lo_b, 0)
    assert np.array_equal(a, b)


def test_rescue_through_map_pairs(env):
    g, sm, rs = env.g, env.sm, env.rs
    # ---- worked out on the CPU: the first pass's gaps, the windows, and what rescue must find
    want_windows = np.zeros((28, 2), np.int32)
    want_windows[2 * 3 + 1] = (500, 1500)                            # pair 1: partner [500, 650) forward: RIGHT, strand 1 of read 3
    want_windows[2 * 4 + 0] = (12000, 12900)                         # pair 2: partner [750, 900) of contig c reverse: LEFT [-100, 900), cut at 0
    want_windows[2 * 7 + 1] = (200, 1200)
    want_windows[2 * 9 + 1] = (13000, 14000)
    want_windows[2 * 11 + 1] = (5700, 6000)                          # clamped to contig a
    plain = sm.map_pairs(env.strs, MIN_LEN, rs)
    assert len(plain) == 7
    rec0, so0, pairs0, sam0 = _np(plain[0]), _np(plain[1]), _np(plain[5]), _np(plain[6])
    assert np.diff(so0).tolist() == [1, 1, 1, 0, 0, 1, 1, 0, 1, 0, 1, 0, 2, 1]      # every diverged mate is without a record
    assert (pairs0[:, 2] & 1).tolist() == [1, 0, 0, 0, 0, 0, 1]
    csr = sm._csr_reads(env.strs, False)
    brute, brute_tt = WU.plan(N_REF, TABLE, np.asarray(csr[1]), so0, rec0, pairs0, 1, 1000, 40)
    assert np.array_equal(brute, want_windows) and brute_tt.tolist() == [5, 5, 5]
    # ---- the GPU
    out = sm.map_pairs(env.strs, MIN_LEN, rs, rescue=True)
    assert len(out) == 8
    rec, so, offs, cigar, info, pairs, sam = (_np(t) for t in out[:7])
    windows, status, totals = (_np(t) for t in out[7])
    assert np.array_equal(windows, want_windows)
    assert status.tolist() == [int(w[1] > w[0]) for w in want_windows] and totals[2] == 0 and totals[1] >= 2 * (150 // EVERY)
    assert np.diff(so).tolist() == [1, 1, 1, 1, 1, 1, 1, 0, 1, 0, 1, 0, 2, 1]
    assert (pairs[:, 2] & 1).tolist() == [1, 1, 1, 0, 0, 0, 1]
    text = g.cigar_strings(out[2], out[3])
    for pair, mate, strand, contig, offset, anchor_flag, mate_flag in ((1, 3, 1, 0, 751, 99, 147), (2, 4, 0, 2, 501, 147, 99)):
        j = int(so[mate])
        assert rec[j, [0, 2, 3, 4, 5, 6, 7, 8]].tolist() == [mate, 0, strand, contig, offset, 150, 0, 150]
        assert text[j] == env.cigar and "X" in text[j] and info[j, 3] == env.subs == info[j, 5] and info[j, 6] == info[j, 7] == 0
        other = int(so[mate ^ 1])
        assert sam[j, 0] == mate_flag and sam[other, 0] == anchor_flag and sam[j, 2] == other and sam[other, 2] == j
        assert abs(int(sam[j, 3])) == 400 and pairs[pair, 5] == 400 and pairs[pair, 7] == 0      # FR, 400 bases end to end
        assert rec[j, 9] == 150 - 5 * env.subs + 2 * END_BONUS       # match 1, mismatch 4, both ends reached: every alignment's program
    for pair in (3, 4, 5):                                           # outside the window, random, across the boundary
        assert pairs[pair, :3].tolist() == [int(so[2 * pair]), -1, 2] and sam[so[2 * pair], 0] == 73
    # ---- pairs that were proper in the first pass: the same records and SAM rows but for the chain index
    for pair in (0, 6):
        lo_a, lo_b = int(so[2 * pair]), int(so0[2 * pair])
        n = int(so[2 * pair + 2]) - lo_a
        assert n == int(so0[2 * pair + 2]) - lo_b
        _same_but_chain(rec, sam, lo_a, rec0, sam0, lo_b, n)
    lines = g.sam_lines(out[0], out[6], out[4], out[2], out[3], [f"p{i // 2}" for i in range(14)], rs.names, env.strs)
    mate = [ln.split("\t") for ln in lines if ln.startswith("p1\t")][1]
    assert mate[1:6] == ["147", "a", "751", mate[4], env.cigar] and f"NM:i:{env.subs}" in mate


def test_options_reach_the_calls(env):
    sm, rs = env.sm, env.rs
    strs = env.strs[2:4] + env.strs[6:8]                             # the rescued pair and the pair 5 kb apart
    out = sm.map_pairs(strs, MIN_LEN, rs, rescue=True, rescue_options=dict(min_len=13))      # one base above the longest run
    assert (_np(out[5])[:, 2] & 1).tolist() == [0, 0] and _np(out[7][1]).tolist() == [0, 0, 0, 1, 0, 0, 0, 1]
    wide = dict(isize_max=5500, pen_max=0)
    out = sm.map_pairs(strs, MIN_LEN, rs, rescue=True, pair_options=wide)      # the window follows pair_options: 5 kb is inside now
    assert (_np(out[5])[:, 2] & 1).tolist() == [1, 1] and _np(out[7][0])[7].tolist() == [200, 5700]
    out = sm.map_pairs(strs, MIN_LEN, rs, rescue=True, pair_options=wide, rescue_options=dict(isize_max=1000))
    assert (_np(out[5])[:, 2] & 1).tolist() == [1, 0] and _np(out[7][0])[7].tolist() == [200, 1200]
    out = sm.map_pairs(strs, MIN_LEN, rs, rescue=True, rescue_options=dict(min_anchor_score=150 + 2 * END_BONUS + 1))      # above an exact mate's score
    assert not _np(out[7][0]).any() and (_np(out[5])[:, 2] & 1).tolist() == [0, 0]
    with pytest.raises(TypeError):
        sm.map_pairs(strs, MIN_LEN, rs, rescue=True, rescue_options=dict(minimum=3))
    with pytest.raises(ValueError):
        sm.map_pairs(strs, MIN_LEN, rs, both_strands=False, rescue=True)


def test_a_batch_without_a_target_is_unchanged(env):
    sm, rs = env.sm, env.rs
    strs = env.strs[0:2] + env.strs[12:14]                           # the two pairs that are proper without rescue
    plain = sm.map_pairs(strs, MIN_LEN, rs)
    out = sm.map_pairs(strs, MIN_LEN, rs, rescue=True)
    assert len(plain) == 7 and len(out) == 8
    for x, y in zip(plain, out[:7]):
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(_np(x), _np(y))
    windows, status, totals = (_np(t) for t in out[7])
    assert windows.shape == (8, 2) and not windows.any() and status.tolist() == [0] * 8 and totals.tolist() == [0, 0, 0]
