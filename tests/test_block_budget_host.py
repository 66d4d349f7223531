"""CPU-only: the compact match table past its 65535 overflow blocks (tests/budget_util.py).  The host builder is the
specification of the image, so the branch that writes an eligible entry without a block -- "the rows decide" -- is pinned
here from the serialized bytes alone: that the budget is exhausted and in which order, what the blocks hold, that the read
batches of test_block_budget_gpu.py land on such entries, that automatic knobs reach the branch on a 4.1 Mb reference, the
kFlagDir16 header bit in both states, and the device builder's image bound.

Measured with REF (1 500 000 random bases, table_bits 9): 90 821 entries with 7 .. 13 suffixes, 65 535 served, 25 286
starved (5 of these because a suffix is cut short); 11.5 % of the positions of 2000 x 150 from-reference reads fall on
starved entries and 29.9 % on block entries."""
import numpy as np
import pytest

import budget_util as B
from test_host_index import _parse


@pytest.fixture(scope="module")
def pkg():
    import genie_smem_amd as g
    g._native.build()
    g._native.lib()
    return g


@pytest.fixture(scope="module")
def cls(pkg):
    return B.classes(pkg)


def _eligible(cls):
    return (cls.count >= B.M16_MIN_ROWS) & (cls.count <= B.M16_MAX_ROWS) & ~cls.cut


def test_budget_is_exhausted_in_code_order(pkg, cls):
    h, _, mtab, _, _ = B.sections(B.image(pkg))
    assert (h["P"], h["P2"], h["K"], h["n"]) == (7, B.P2, B.K, B.N_REF) and h["flags"] & 2
    assert h["ov_entries"] == B.MAX_BLOCKS + 1
    served = np.flatnonzero(cls.block)
    assert len(served) == B.MAX_BLOCKS
    # block indices 1 .. 65535, each used once, ascending with the P2-mer code
    assert mtab["key"][served, B.M16_KEYS - 1].astype(np.int64).tolist() == list(range(1, B.MAX_BLOCKS + 1))
    assert (cls.nib[served] == cls.count[served] - 7).all()
    # the first 65535 eligible entries, in code order, have the blocks; none after them does
    eligible = np.flatnonzero(_eligible(cls))
    assert len(eligible) > B.MAX_BLOCKS
    assert cls.block[eligible[:B.MAX_BLOCKS]].all() and not cls.block[eligible[B.MAX_BLOCKS:]].any()
    assert np.array_equal(served, eligible[:B.MAX_BLOCKS])
    # a starved entry: six keys and "the rows decide"
    starved = np.flatnonzero(cls.starved)
    assert (cls.cnt4[starved] == B.M16_KEYS).all() and ((cls.nib[starved] & B.M16_GENERAL) != 0).all()
    not_cut = starved[~cls.cut[starved]]
    assert np.array_equal(not_cut, eligible[B.MAX_BLOCKS:])
    print(f"eligible {len(eligible)}, served {len(served)}, starved {len(starved)} ({len(not_cut)} not cut short)")
    assert len(not_cut) >= 20_000                             # measured 25 286


def test_block_contents(pkg, cls):
    """Keys 0 .. 4 of a block entry and the keys of its block are the 8 bases after the P2-mer of rows lb .. lb + count - 1;
    unused block slots repeat the block's first key.  A starved entry holds the keys of its first six rows."""
    _, _, mtab, ov, sa0 = B.sections(B.image(pkg))
    served = np.flatnonzero(cls.block)
    lb, count = cls.lb[served], cls.count[served]
    slot = np.arange(B.M16_MAX_ROWS)[None, :]
    row = lb[:, None] + np.minimum(slot, count[:, None] - 1)
    keys = B.keys_after(B.REF, sa0[row], cls.P2)              # [entries, 13]; slots past the count hold the last row's key
    assert (np.diff(keys, axis=1) >= 0).all()                 # suffix-array order
    assert np.array_equal(mtab["key"][served, :5].astype(np.int64), keys[:, :5])
    blocks = ov[mtab["key"][served, 5]].astype(np.int64)
    want = np.where(slot[:, 5:] < count[:, None], keys[:, 5:], keys[:, 5:6])
    bad = np.flatnonzero((blocks != want).any(1))
    assert not len(bad), (len(bad), "first: P2-mer", int(served[bad[0]]), blocks[bad[0]].tolist(), want[bad[0]].tolist())
    assert not ov[0].any()                                    # block 0 is never referenced
    starved = np.flatnonzero(cls.starved & ~cls.cut)
    keys6 = B.keys_after(B.REF, sa0[cls.lb[starved][:, None] + np.arange(B.M16_KEYS)[None, :]], cls.P2)
    assert np.array_equal(mtab["key"][starved].astype(np.int64), keys6)


def test_the_workload_reaches_it(pkg, cls):
    b = B.batches(pkg)
    reads = b["fromref150"]
    assert len(reads) == 2000 and all(len(r) == 150 for r in reads)
    total = B.positions(reads)
    on_starved, on_block = B.positions_on(cls.starved, reads, cls.P2), B.positions_on(cls.block, reads, cls.P2)
    print(f"positions on starved entries {on_starved / total:.3f}, on block entries {on_block / total:.3f}")
    assert on_starved >= 0.05 * total                          # measured 11.5 %
    assert on_block >= 0.10 * total                            # measured 29.9 %
    for label, kind in B.TARGETED.items():
        mask = cls.starved if kind == "starved" else cls.block
        assert len(b[label]) >= 72 and B.starts_on(mask, b[label], cls.P2), label
    for label in ("fromref255", "random150", "ragged", "mid705", "mid1409", "long9000"):
        assert B.positions_on(cls.starved, b[label], cls.P2) >= 0.05 * B.positions(b[label]), label
    assert sorted(len(r) for r in b["ragged"]) == list(range(1, 256))
    assert {len(r) for r in b["mid705"]} == {705} and {len(r) for r in b["mid1409"]} == {1409}
    assert min(len(r) for r in b["long9000"]) > 8192


def test_default_knobs_reach_it_too(pkg):
    ref = np.random.default_rng(1).integers(0, 4, 4_100_000).astype(np.uint8)
    h = _parse(pkg.GenieIndex.build(ref, 0).serialize().numpy())
    assert h["P2"] == 10 and h["flags"] & 2 and h["ov_entries"] == B.MAX_BLOCKS + 1


def test_dir16_flag_both_ways(pkg):
    """kFlagDir16 (header flags bit 0) is cleared when 16 neighbouring directory entries span more than 65535 rows."""
    flags = _parse(pkg.GenieIndex.build(np.zeros(70_000, np.uint8), 8).serialize().numpy())["flags"]
    assert flags & 1 == 0 and flags & 2
    assert _parse(pkg.GenieIndex.build(np.zeros(5000, np.uint8), 8).serialize().numpy())["flags"] & 1
    assert _parse(B.image(pkg))["flags"] & 1


def test_device_image_bound_holds(pkg):
    """What a caller of genie_index_create_device allocates from holds the image the host builder writes."""
    N = pkg._native
    lib = N.lib()
    cases = [(B.index(pkg), B.N_REF, B.K, 7, B.P2 | N.TABLE_COMPACT),
             (pkg.GenieIndex.build(np.zeros(70_000, np.uint8), 8), 70_000, 8, 7, 0)]
    for ix, n, k, dir_bits, table_bits in cases:
        bound = int(lib.genie_index_device_image_bound(n, k, dir_bits, table_bits))
        tmp = int(lib.genie_index_device_build_tmp_bytes(n, k, dir_bits, table_bits))
        for image_flags in (0, N.IMAGE_NO_SEED_TABLE):
            nbytes = int(lib.genie_index_image_bytes(ix._h, image_flags))
            assert nbytes > 0 and bound >= nbytes and tmp >= nbytes, (n, image_flags, nbytes, bound, tmp)
