"""GPU: the capped slow list of the match-statistics kernel (match_table_body.inc) against the brute force of
tests/smem_util.py.  A group of more than kMtSlowCap = 512 positions keeps a slow list of 512 entries and runs its slow
passes whenever the next lookup pass could overflow it; that must change no result.

The reads that fill the list are cuts of the tandem references of tests/lookup_util.py: every position of such a read
matches up to the end of the read, which no table entry can decide (its 8-mers have hundreds of suffixes each), so
all but the last lookups of every round are slow items.  With GENIE_OPT_GROUP_POSITIONS = 1 000 000 a group is 16 reads (12 at 255 bases): 608 quads
at 150 bases, so the list reaches its capacity in round 1, in the middles and in the neighbours of one group; with the
default options (10 reads at 150 bases, 6 at 255) in round 2 only.  Batches of 33 and 4 x 16 + 1 reads: whole groups and a
last group of one read.  Between cuts of rand4096 -- random to the index, next to no slow items -- the list crosses its
threshold at other iterations, and a flush is followed by iterations that add nothing.  Offsets, rows and statuses are
compared exactly, for every read."""
import functools

import numpy as np
import pytest

import smem_util as S
import test_tuning_knobs_gpu as T

pytestmark = pytest.mark.gpu

SETTING = (7, 0, "compact")
HARD = ["tandem7", "tandem1"]
MODES = [("bwa", 1), ("lut", 1), ("rmi", 1)]
SIZES = (33, 4 * 16 + 1)
ALL_IN_ONE_GROUP = 1_000_000


@pytest.fixture(scope="module")
def pkg():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import genie_smem_amd as g
    g._native.lib()
    return g


_INDEX = {}


def _index(pkg, name):
    if name not in _INDEX:
        K = T.key_size(name, T.AUTO_P2, HARD.index(name))
        _INDEX[name] = (T._build(pkg, name, *SETTING, K), K)
    return _INDEX[name]


def _cut(ref, rng, L):
    s = int(rng.integers(0, len(ref) - L + 1))
    return ref[s:s + L].copy()


@functools.lru_cache(maxsize=None)
def _batch(name, kind, n):
    """A list of reads.  "fixed": n cuts of 150 bases of the tandem reference; "ragged": n cuts of lengths 1 .. 255, 1, 150
    and 255 among them; "mixed": runs of 1, 3, 9 and 16 hard reads between cuts of rand4096; "skipped": hard reads with a
    code 7 and an empty read among them."""
    ref, easy = T.FAMILY[name], T.FAMILY["rand4096"]
    rng = np.random.default_rng(1000 * HARD.index(name) + n)
    if kind == "fixed":
        return tuple(_cut(ref, rng, 150) for _ in range(n))
    if kind == "ragged":
        lens = [255, 1, 150, 254, 2] + [int(x) for x in rng.integers(1, 256, n - 5)]
        return tuple(_cut(ref, rng, L) for L in lens)
    if kind == "mixed":
        out = []
        for run, gap in ((1, 7), (3, 2), (9, 13), (16, 5), (16, 1), (3, 21)):
            out += [_cut(easy, rng, 150) for _ in range(gap)] + [_cut(ref, rng, 150) for _ in range(run)]
        return tuple(out)
    assert kind == "skipped"
    out = [_cut(ref, rng, int(rng.integers(100, 256))) for _ in range(n)]
    for i in range(1, n, 5):
        out[i] = np.zeros(0, np.uint8) if i % 2 else out[i].copy()
        if len(out[i]):
            out[i][len(out[i]) // 2] = S.BAD_CODE
    return tuple(out)


_DEVICE = {}


def _on_device(name, kind, n):
    import torch
    if (name, kind, n) not in _DEVICE:
        reads = _batch(name, kind, n)
        if kind in ("fixed", "mixed"):
            _DEVICE[name, kind, n] = (torch.as_tensor(np.stack(reads)).cuda(), None)
        else:
            mat, lens = S.matrix(list(reads), 255 + 3)
            _DEVICE[name, kind, n] = (torch.as_tensor(mat).cuda(), torch.as_tensor(lens).cuda())
    return _DEVICE[name, kind, n]


@functools.lru_cache(maxsize=None)
def _want(name, kind, n, mode, min_len, K):
    return S.expected_batch(T.FAMILY[name], list(_batch(name, kind, n)), mode, min_len, K)


def _options(pkg, which):
    N = pkg._native
    return {"one-group": {N.OPT_GROUP_POSITIONS: ALL_IN_ONE_GROUP},
            "one-group-all": {N.OPT_GROUP_POSITIONS: ALL_IN_ONE_GROUP, N.OPT_SEARCH_ALL: 1},
            "default": {}}[which]


def _with_options(pkg, ix, which, body):
    setting = _options(pkg, which)
    try:
        for opt, value in setting.items():
            ix.set_option(opt, value)
        body()
    finally:
        for opt in setting:
            ix.set_option(opt, 0)


def _check(ix, K, name, kind, n, tag, modes=MODES):
    reads = _batch(name, kind, n)
    mat, lens = _on_device(name, kind, n)
    for mode, min_len in modes:
        got = ix.find_smems(mode, mat, lens, min_len)
        T._compare(got, _want(name, kind, n, mode, min_len, K if mode != "bwa" else 0), reads, tag + (kind, n, mode))


def test_hard_reads_have_slow_items_everywhere():
    """What the batches rest on, from the brute force alone: a hard read is a piece of the reference, so every position
    matches up to the end of the read -- beyond table_bits + 16 bases, past every shortcut of a table entry, for all but the
    last positions -- and its 8-mers have many suffixes each."""
    for name in HARD:
        ref = T.FAMILY[name]
        for read in _batch(name, "fixed", 33) + _batch(name, "ragged", 33):
            assert (S.matching_stats(ref, read) == len(read)).all(), name


OPTIONS = ["one-group", "one-group-all", "default"]


@pytest.mark.parametrize("which", OPTIONS)
@pytest.mark.parametrize("name", HARD)
def test_every_position_slow(pkg, name, which):
    ix, K = _index(pkg, name)
    N = pkg._native
    if which != "default":
        ix.set_option(N.OPT_GROUP_POSITIONS, ALL_IN_ONE_GROUP)
    try:
        big, small = ix.launch_info("bwa", 150)["lds_bytes"], None
        ix.set_option(N.OPT_GROUP_POSITIONS, 512)
        small = ix.launch_info("bwa", 150)["lds_bytes"]
    finally:
        ix.set_option(N.OPT_GROUP_POSITIONS, 0)
    assert big > small                                       # the groups under test are larger than the list's capacity

    def body():
        for n in SIZES:
            _check(ix, K, name, "fixed", n, (name, which))
            _check(ix, K, name, "ragged", n, (name, which))
    _with_options(pkg, ix, which, body)


@pytest.mark.parametrize("which", OPTIONS)
@pytest.mark.parametrize("name", HARD)
def test_mixed_groups_and_skipped_reads(pkg, name, which):
    ix, K = _index(pkg, name)
    want = _want(name, "skipped", 33, "bwa", 1, 0)
    assert S.READ_BAD_BASE in want[2].tolist() and 0 in [len(r) for r in _batch(name, "skipped", 33)]

    def body():
        _check(ix, K, name, "mixed", 0, (name, which))
        for n in SIZES:
            _check(ix, K, name, "skipped", n, (name, which))
    _with_options(pkg, ix, which, body)


@pytest.mark.parametrize("which", OPTIONS)
def test_both_strands_and_packed_reads(pkg, which):
    from genie_smem_amd import packing
    name = "tandem7"
    ix, K = _index(pkg, name)
    ref = T.FAMILY[name]
    reads = list(_batch(name, "fixed", SIZES[1]))
    ragged = list(_batch(name, "ragged", 33))
    both = [x for r in ragged for x in (r, packing.reverse_complement(r))]
    mat, lens = _on_device(name, "ragged", 33)
    packed = packing.pack_reads(np.stack(reads))

    def body():
        for mode, min_len in MODES:
            k = K if mode != "bwa" else 0
            T._compare(ix.find_smems_both(mode, mat, lens, min_len), S.expected_batch(ref, both, mode, min_len, k), both,
                       (which, "both", mode))
            c8, s8, r8, esc = ix.find_smems_packed(mode, packed, 150, None, min_len, row_bytes=8)
            off, rows = packing.unpack_rows(c8.cpu().numpy(), r8.cpu().numpy(), esc.cpu().numpy(), row_bytes=8)
            T._compare((off, rows, s8.cpu().numpy().astype(np.int32)), _want(name, "fixed", SIZES[1], mode, min_len, k), reads,
                       (which, "packed", mode))
    _with_options(pkg, ix, which, body)
