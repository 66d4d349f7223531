"""GPU: the persistent kernels -- the match-statistics kernel (match_table_kernel, match_table_both_kernel,
match_table_long*_kernel), interval_rows_kernel and interval_kernel -- over MANY groups per wave on HARD reads, against the
brute force of tests/smem_util.py.  A wave of these kernels carries state from one group of reads to the next, and the launch
plans cap the grid at the batch, so a wave takes a second group only in batches of several thousand reads; the batches of
the other brute-force tests end within a wave's first group.  Here a batch is an order over the few hundred distinct reads of
one edge reference (tests/handout_util.py, pinned on the host by test_group_handout_host.py): the brute force runs once per
distinct read, the batch is built on the device by index_select, and offsets, rows (or counts and slots) and statuses of the
WHOLE batch are compared exactly, on the device.  The batch size follows from genie_launch_info and the device's CU count
and is asserted: every wave of the match-statistics kernel takes at least four groups (N >= 4 x grid x waves x 16, 16 =
kMtMaxG, the most reads a group holds; one read per group above 255 bases), interval_rows_kernel more than two rounds of
tiles (N > 2 x CUs x 4 x 256), interval_kernel at least four passes per wave (N >= 4 x CUs x 4 x 32).

What every order aims at (names as in csrc/match_table_body.inc, match_table_long_body.inc and short_read_kernel.inc):
  "shuffled"         a slot of a wave holds a read of any length and kind after any other: the zero padding of `Dp` behind a
                     read (only the first DWp dwords of a row are rewritten per group), its length in `Ls`, the round-2
                     lists `qa` / `qb` and the slow list `sl` refilled from zero by every group; ragged `lens`, and `vlens`
                     of the strand-reads in the both-strands kernel, whose pairs an odd group splits over two groups.
  "runs"             whole groups, several in a row on every wave, of ONE kind of read: the longest slow path (one base
                     repeated, the tandem unit tile: the longest `sl` and `qa` / `qb` there are, and the most rows per tile
                     of interval_rows_kernel, up to 255 per read), then only flagged reads (`any_read` false: the group is
                     skipped, nothing of the previous group's `Ls`, `fwL` or lists may reach the output), then only empty
                     reads, then 1-base reads behind 255-base ones.  Runs of 1, 7, 64 and 300 reads put the change of kind
                     inside a group, at a group's edge and at a tile's edge.
  "long_then_short"  a long read directly followed by a short one, in the end every read behind every other one: what a
                     longer predecessor leaves in `Dp`, `fwL` and the staged tile of interval_rows_kernel behind a shorter
                     read; a read without rows between reads with many (the bisection over the tile's starts).
  "tail"             the partial last group (N is odd) and the last tile, the last claims of the hand-out counter
                     `next_group` (the group after the current one is claimed, and its input rows touched, a group early):
                     a flagged read, an empty read and 35 reads of 255 bases end the batch.
The launch options (GENIE_OPT_SCHEDULING, _GROUP_POSITIONS, _SEARCH_BLOCKS_PER_CU, _SEARCH_ALL) change who takes which
group, how many reads a group holds and which positions are looked up; each setting is compared with the brute force too.

A batch with min_len 12 keeps few rows (0.04 to 0.4 per read: most pool reads are shorter than 12 bases), so "more rows than
reads" is asserted there for the rows of the same batch with min_len 1, which the kernels traverse all the same."""
import functools

import numpy as np
import pytest

import handout_util as H
import smem_util as S
import test_tuning_knobs_gpu as T

pytestmark = pytest.mark.gpu

REFS = ["rand4096", "tandem7", "noT", "tail_AAAAAAAA"]
SETTINGS = [(7, 0, "compact"), (7, 0, "wide"), (7, 11, "compact")]      # the 6-, 8- and 4-waves-per-SIMD builds
WPS = {SETTINGS[0]: 6, SETTINGS[1]: 8, SETTINGS[2]: 4}
MODES = T.MODES
MAX_G = 16                          # kMtMaxG
SEED = 11


@pytest.fixture(scope="module")
def pkg():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import genie_smem_amd as g
    g._native.lib()
    return g


def _mode_id(m):
    return f"{m[0]}{m[1]}"


# ------------------------------------------------------------------ indexes, pools, sizes
_INDEX, _POOL = {}, {}


def _index(pkg, name, setting):
    """(index on the device, K): host-built, natively trained RMI [10]; K below, at or above P2 by reference and setting."""
    if (name, setting) not in _INDEX:
        P, bits, form = setting
        refs = REFS + ["tandem1"]
        K = T.key_size(name, bits or T.AUTO_P2, refs.index(name) + SETTINGS.index(setting))
        ix = T._build(pkg, name, P, bits, form, K)
        kernel = ix.search_kernel_name("bwa", 255)
        assert kernel.startswith(f"match_table_kernel<{WPS[setting]}, "), kernel
        _INDEX[name, setting] = (ix, K)
    return _INDEX[name, setting]


def test_key_sizes_lie_on_either_side_of_table_bits():
    signs = set()
    for s, (P, bits, form) in enumerate(SETTINGS):
        for r, name in enumerate(REFS):
            signs.add(int(np.sign(T.key_size(name, bits or T.AUTO_P2, r + s) - (bits or T.AUTO_P2))))
    assert signs == {-1, 0, 1}


def _pool(name, variant):
    """(reads, matrix on the device, lens on the device or None) of a pool, uploaded once.  "short" / "mid": handout_util.pool;
    "cut-short": the short pool with breaks; "fixed150+0" / "fixed150+3": the 150-base reads, `lens` NULL, stride 150 / 153;
    "packed150" / "packed255": the reads of that length without a code > 3, 2-bit packed."""
    import torch
    from genie_smem_amd import packing
    if (name, variant) not in _POOL:
        reads = H.pool(name, "mid" if variant == "mid" else "short")[0]
        lens = None
        if variant in ("short", "mid"):
            _, mat, lens = H.pool(name, variant)
        elif variant == "cut-short":
            reads = T._with_breaks(reads, T.AUTO_P2)
            mat, lens = S.matrix(reads, 255 + 3, H.JUNK)
        elif variant.startswith("fixed"):
            L, slack = (int(x) for x in variant[5:].split("+"))
            reads = [r for r in reads if len(r) == L]
            mat, _ = S.matrix(reads, L + slack, H.JUNK)
        else:
            L = int(variant[6:])
            reads = [r for r in reads if len(r) == L and not H.flagged(r)]
            mat = packing.pack_reads(np.stack(reads))
        _POOL[name, variant] = (reads, torch.as_tensor(mat).cuda(), None if lens is None else torch.as_tensor(lens).cuda())
    return _POOL[name, variant]


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _odd(n):
    return n | 1


def _size(ix, max_len, rows_kernel=False, slots=False):
    """The batch size for reads of up to max_len bases under the index's current options, asserted against the launch the
    library reports: at least four groups for every wave of the match-statistics kernel; with rows_kernel more than two
    rounds of tiles of interval_rows_kernel; with slots four passes of every wave of interval_kernel.  Odd."""
    info = ix.launch_info("bwa", max_len)
    grid, block = info["grid"], info["block"]
    assert grid >= 1 and block % 64 == 0 and block >= 64, info
    assert all(ix.launch_info(m, max_len) == info for m in ("lut", "rmi"))
    G = MAX_G if max_len <= 255 else 1
    need = 4 * grid * (block // 64) * G
    if rows_kernel:
        need = max(need, 2 * _cus() * 4 * 256 + 1)
    if slots:
        need = max(need, 4 * _cus() * 4 * 32)
    N = _odd(need)
    assert N >= 4 * grid * (block // 64) * G and N % 2 == 1, (N, info)
    assert not rows_kernel or N > 2 * _cus() * 4 * 256
    assert not slots or N >= 4 * _cus() * 4 * 32
    return N


@functools.lru_cache(maxsize=8)
def _orders(name, variant, N):
    """The orders of a pool; those of the pool with breaks are the plain pool's (the same reads, index for index: with a
    break in every read none of them would be of the kinds that "runs" and "tail" are made of)."""
    return H.orders(_pool(name, "short" if variant == "cut-short" else variant)[0], N, SEED)


def _batch(name, variant, order, N):
    """(pick on the host, reads [N, stride] on the device, lens [N] or None)."""
    import torch
    _, mat, lens = _pool(name, variant)
    pick = _orders(name, variant, N)[order]
    at = torch.as_tensor(pick).cuda()
    return pick, mat.index_select(0, at), None if lens is None else lens.index_select(0, at)


# ------------------------------------------------------------------ expectations and the comparison
_WANT = {}          # the last expectation, on the device: consecutive cases that differ in the index alone share it


def _want(name, variant, order, N, mode, min_len, K, both=False):
    """((offsets, rows, status) on the device, the same on the host, the number of rows with min_len 1) of a batch."""
    import torch
    K = 0 if mode == "bwa" else K
    key = (name, variant, order, N, mode, min_len, K, both)
    if key not in _WANT:
        _WANT.clear()
        reads = _pool(name, variant)[0]
        pick = _orders(name, variant, N)[order]
        if both:
            reads, pick = H.both_strands(reads), H.both_pick(pick)
        per = H.per_read(name, reads, mode, min_len, K, split=variant.startswith("cut"))
        host = H.gather_expected(per, pick)
        ones = H.count_rows(H.per_read(name, reads, mode, 1, K, split=variant.startswith("cut")), pick)
        _WANT[key] = (tuple(torch.as_tensor(x).cuda() for x in host), host, ones)
    return _WANT[key]


def _check_statuses(name, status, mode, short=True, flagged=True, split=False):
    """The batch holds a read of every status it can: OK; BAD_BASE (a code 7) unless the pool has none; ABSENT_BASE where the
    reference lacks a base; TOO_SHORT outside bwa where the pool has `short` reads (a pool read of 150 bases and more is
    longer than any K).  With breaks every status is OK."""
    have = set(np.unique(status).tolist())
    want = {S.READ_OK}
    if not split:
        if flagged:
            want.add(S.READ_BAD_BASE)
        if len(np.unique(T.FAMILY[name])) < 4:
            want.add(S.READ_ABSENT_BASE)
        if mode != "bwa" and short:
            want.add(S.READ_TOO_SHORT)
    assert have == want, (have, want)


def _explain(got, want, reads, pick, tag):
    """Offsets, rows and statuses differ somewhere: names the first batch element that does, its pool read and both row lists."""
    off, rows, st = (x.cpu().numpy() for x in got)
    woff, wrows, wst = want
    n = min(len(st), len(wst))
    bad = np.flatnonzero((st[:n] != wst[:n]) | (np.diff(off)[:n] != np.diff(woff)[:n]))
    if not len(bad) and rows.shape == wrows.shape:
        r = int(np.flatnonzero((rows != wrows).any(axis=1))[0])
        bad = [int(np.searchsorted(woff, r, side="right")) - 1]
    assert len(bad), (tag, "shapes", off.shape, woff.shape, rows.shape, wrows.shape)
    b = int(bad[0])
    a = (int(st[b]), rows[off[b]:off[b + 1]].tolist())
    w = (int(wst[b]), wrows[woff[b]:woff[b + 1]].tolist())
    raise AssertionError((tag, "batch element", b, "of", len(wst), "pool read", int(pick[b]), np.asarray(reads[int(pick[b])]).tolist()[:100],
                          "the elements before it", np.asarray(pick[max(b - 48, 0):b]).tolist(), "got", a, "want", w))


def _compare(got, want, reads, pick, tag):
    """A CSR result against the expectation, exactly and on the device."""
    import torch
    dev, host, _ = want
    off, rows, st = got
    if off.shape == dev[0].shape and rows.shape == dev[1].shape and st.shape == dev[2].shape \
            and torch.equal(off, dev[0]) and torch.equal(st, dev[2]) and torch.equal(rows, dev[1]):
        return
    _explain(got, host, reads, pick, tag)


def _find_fixed(ix, mode, mat, fixed_len, min_len, rows_hint):
    """genie_find_smems_csr without lengths on rows that are longer than the reads (GenieIndex.find_smems takes the stride for
    the length): every read is the first fixed_len bytes of its row."""
    from genie_smem_amd import _native as N
    from genie_smem_amd.index import _ptr
    n, stride = mat.shape
    assert mat.is_contiguous() and fixed_len <= stride
    ws, ws_bytes = ix._workspace("genie_find_smems_workspace_bytes", n, fixed_len)
    return ix._run_csr("genie_find_smems_csr", (N.MODES[mode], _ptr(mat), _ptr(None), n, stride, fixed_len, int(min_len)), n, rows_hint,
                       (_ptr(ws), ws_bytes))


def _check_csr(ix, K, name, variant, order, N, mode, min_len, tag, flagged=True, fixed_len=None):
    """genie_find_smems_csr on one batch, against the brute force."""
    pick, mat, lens = _batch(name, variant, order, N)
    want = _want(name, variant, order, N, mode, min_len, K)
    if fixed_len is None:
        got = ix.find_smems(mode, mat, lens, min_len, rows_hint=len(want[1][1]) + 1)
    else:
        assert lens is None
        got = _find_fixed(ix, mode, mat, fixed_len, min_len, len(want[1][1]) + 1)
    _compare(got, want, _pool(name, variant)[0], pick, tag)
    _check_statuses(name, want[1][2], mode, variant == "short", flagged)
    assert want[2] > N and (min_len > 1 or len(want[1][1]) > N)
    return want


# ------------------------------------------------------------------ genie_find_smems_csr, reads of up to 255 bases
CSR_CASES = [(name, order, mode, setting) for name in REFS for order in H.ORDERS for mode in MODES for setting in SETTINGS]


def _csr_id(c):
    return f"{c[0]}-{c[1]}-{_mode_id(c[2])}-{T._id(c[3])}"


@pytest.mark.parametrize("case", CSR_CASES, ids=_csr_id)
def test_csr_ragged(pkg, case):
    """match_table_kernel (the group holds 3 reads at 255 bases), traverse_kernel, interval_rows_kernel."""
    name, order, (mode, min_len), setting = case
    ix, K = _index(pkg, name, setting)
    N = _size(ix, 255, rows_kernel=True)
    _check_csr(ix, K, name, "short", order, N, mode, min_len, _csr_id(case))


FIXED_CASES = [(name, slack, mode, SETTINGS[(i + j + k) % 3]) for i, name in enumerate(REFS) for j, slack in enumerate((0, 3))
               for k, mode in enumerate((MODES[1], MODES[2]))]


@pytest.mark.parametrize("case", FIXED_CASES, ids=lambda c: f"{c[0]}-stride{150 + c[1]}-{_mode_id(c[2])}-{T._id(c[3])}")
def test_csr_fixed_length(pkg, case):
    """`lens` NULL, 150 bases, stride 150 (a read's last 16-byte piece is loaded from the next read's row) and 153: the group
    holds 5 reads."""
    name, slack, (mode, min_len), setting = case
    ix, K = _index(pkg, name, setting)
    N = _size(ix, 150, rows_kernel=True)
    variant = f"fixed150+{slack}"
    assert _pool(name, variant)[1].shape[1] == 150 + slack and _pool(name, variant)[2] is None
    _check_csr(ix, K, name, variant, "runs", N, mode, min_len, (name, variant, mode, min_len, setting), fixed_len=150)


# ------------------------------------------------------------------ genie_find_smems_both
BOTH_CASES = [(name, order, mode) for name in REFS for order in ("shuffled", "long_then_short") for mode in (MODES[1], MODES[2])]


@pytest.mark.parametrize("case", BOTH_CASES, ids=lambda c: f"{c[0]}-{c[1]}-{_mode_id(c[2])}")
def test_both_strands_ragged(pkg, case):
    """match_table_both_kernel: with 255-base reads the group holds 3 strand-reads, so every other pair lies in two groups."""
    name, order, (mode, min_len) = case
    setting = SETTINGS[(REFS.index(name) + BOTH_CASES.index(case)) % 3]
    ix, K = _index(pkg, name, setting)
    N2 = _size(ix, 255, rows_kernel=True)                 # strand-reads
    N = _odd((N2 + 1) // 2)
    pick, mat, lens = _batch(name, "short", order, N)
    want = _want(name, "short", order, N, mode, min_len, K, both=True)
    assert len(want[1][2]) == 2 * N >= N2
    got = ix.find_smems_both(mode, mat, lens, min_len, rows_hint=len(want[1][1]) + 1)
    _compare(got, want, H.both_strands(_pool(name, "short")[0]), H.both_pick(pick), (case, setting))
    _check_statuses(name, want[1][2], mode)
    assert want[2] > 2 * N


# ------------------------------------------------------------------ genie_find_smems_packed / _packed6
def _packed_rows(rows, row_bytes):
    """int32 (start, end, lo, hi) rows -> (the 8- or 6-byte rows as uint8 [S, row_bytes], escapes int64 [E, 2] in row order) as
    include/genie_smem.h lays them out: start, end, then span = hi - lo in 16 bits and lo in 32 (8 bytes), or lo in 24 bits
    and span in 8 (6 bytes), little-endian; a span of the field's largest value or more holds that value and has an escape
    (row index, hi)."""
    rows = rows.astype(np.int64)
    top = 0xFFFF if row_bytes == 8 else 0xFF
    span = np.minimum(rows[:, 3] - rows[:, 2], top)
    lo = rows[:, 2]
    if row_bytes == 8:
        cols = [rows[:, 0], rows[:, 1], span & 255, span >> 8, lo & 255, (lo >> 8) & 255, (lo >> 16) & 255, lo >> 24]
    else:
        assert int(lo.max()) < 1 << 24
        cols = [rows[:, 0], rows[:, 1], lo & 255, (lo >> 8) & 255, lo >> 16, span]
    wide = np.flatnonzero(span == top)
    return np.stack(cols, axis=1).astype(np.uint8), np.stack([wide, rows[wide, 3]], axis=1).astype(np.int64)


PACKED_CASES = [(name, rb, L, mode) for name, rb in [(n, 8) for n in REFS] + [("tandem1", 6), ("rand4096", 6)] for L in (150, 255)
                for mode in (MODES[1], MODES[2])]


@pytest.mark.parametrize("case", PACKED_CASES, ids=lambda c: f"{c[0]}-{c[1]}bytes-L{c[2]}-{_mode_id(c[3])}")
def test_packed_fixed_length(pkg, case):
    """match_table_kernel<.., PK = true> and interval_rows_kernel with 8- and 6-byte rows: the pool without the reads that
    hold a code 7, one length per batch, order "runs"."""
    import torch
    from genie_smem_amd import packing
    name, rb, L, (mode, min_len) = case
    setting = SETTINGS[PACKED_CASES.index(case) % 3]
    ix, K = _index(pkg, name, setting)
    N = _size(ix, L, rows_kernel=True)
    variant = f"packed{L}"
    reads = _pool(name, variant)[0]
    pick, packed, _ = _batch(name, variant, "runs", N)
    assert packed.shape == (N, packing.packed_stride(L))
    per = H.per_read(name, reads, mode, min_len, K)
    pool8, pool_esc = _packed_rows(H._table(per)[1], rb)     # the pool's rows in the compact form; its rows with an escape
    woff, src, wst = H.gather_index(per, pick)
    counts = np.diff(woff)
    assert int(counts.max()) <= 255 and H.count_rows(H.per_read(name, reads, mode, 1, K), pick) > N
    want8 = pool8[src]
    wide = np.zeros(len(pool8), bool)
    wide[pool_esc[:, 0]] = True
    hi = np.zeros(len(pool8), np.int64)
    hi[pool_esc[:, 0]] = pool_esc[:, 1]
    at = np.flatnonzero(wide[src])
    want_esc = np.stack([at, hi[src[at]]], axis=1).astype(np.int64)
    c8, s8, rows8, esc = ix.find_smems_packed(mode, packed, L, None, min_len, rows_hint=len(src) + 1, row_bytes=rb)
    esc = esc[torch.argsort(esc[:, 0])] if len(esc) else esc
    same = (rows8.shape == want8.shape and esc.shape == want_esc.shape
            and torch.equal(c8, torch.as_tensor(counts.astype(np.uint8)).cuda()) and torch.equal(s8, torch.as_tensor(wst.astype(np.uint8)).cuda())
            and torch.equal(rows8, torch.as_tensor(want8).cuda()) and torch.equal(esc, torch.as_tensor(want_esc).cuda()))
    if not same:
        off, rows = packing.unpack_rows(c8.cpu().numpy(), rows8.cpu().numpy(), esc.cpu().numpy(), row_bytes=rb)
        got = tuple(torch.as_tensor(x) for x in (off, rows, s8.cpu().numpy().astype(np.int32)))
        _explain(got, H.gather_expected(per, pick), reads, pick, (case, setting))
    _check_statuses(name, wst, mode, short=False, flagged=False)
    if name == "tandem1":
        assert len(want_esc) > 0                              # intervals of 255 rows and more: the escape list of the 6-byte rows


# ------------------------------------------------------------------ genie_find_smems_split
SPLIT_CASES = [(name, min_len) for name in REFS for min_len in (1, 12)]


@pytest.mark.parametrize("case", SPLIT_CASES, ids=lambda c: f"{c[0]}-min{c[1]}")
def test_split_ragged(pkg, case):
    """The pool reads with breaks (code 4 at position 0, L - 1, P2 - 1, P2 and a run of three, in turn; the code 7 of the
    flagged reads and the bases the reference lacks are breaks too)."""
    name, min_len = case
    setting = SETTINGS[SPLIT_CASES.index(case) % 2]       # the automatic table_bits, which the breaks are placed by
    ix, K = _index(pkg, name, setting)
    N = _size(ix, 255, rows_kernel=True)
    pick, mat, lens = _batch(name, "cut-short", "shuffled", N)
    want = _want(name, "cut-short", "shuffled", N, "bwa", min_len, K)
    got = ix.find_smems_split(mat, lens, min_len, rows_hint=len(want[1][1]) + 1)
    _compare(got, want, _pool(name, "cut-short")[0], pick, (case, setting))
    _check_statuses(name, want[1][2], "bwa", split=True)
    assert want[2] > N


# ------------------------------------------------------------------ genie_find_smems: slots, interval_kernel
CAP = 32
SLOT_CASES = [(name, kind, mode) for name in REFS for kind in ("short", "mid") for mode in (MODES[0], MODES[2])]


@pytest.mark.parametrize("case", SLOT_CASES, ids=lambda c: f"{c[0]}-{c[1]}-{_mode_id(c[2])}")
def test_slots(pkg, case):
    """Counts, the first min(count, cap) slots of every read and statuses, GENIE_READ_OVERFLOW among them, cap 32."""
    import torch
    name, kind, (mode, min_len) = case
    setting = SETTINGS[SLOT_CASES.index(case) % 3]
    ix, K = _index(pkg, name, setting)
    reads, _, lens_pool = _pool(name, kind)
    N = _size(ix, int(lens_pool.max().item()), slots=True)
    pick, mat, lens = _batch(name, kind, "runs", N)
    per = H.per_read(name, reads, mode, min_len, K)
    counts, slots, filled, status = H.gather_slots(per, pick, CAP)
    got_counts, got_slots, got_status = ix.find_smems_slots(mode, mat, lens, min_len, cap=CAP)
    filled_dev = torch.as_tensor(filled).cuda()[:, :, None]
    if not (torch.equal(got_counts, torch.as_tensor(counts).cuda()) and torch.equal(got_status, torch.as_tensor(status).cuda())
            and torch.equal(got_slots * filled_dev, torch.as_tensor(slots).cuda())):
        c, s, st = got_counts.cpu().numpy(), got_slots.cpu().numpy(), got_status.cpu().numpy()
        for b in range(N):
            k = min(int(counts[b]), CAP)
            a = (int(c[b]), int(st[b]), s[b, :k].tolist())
            w = (int(counts[b]), int(status[b]), slots[b, :k].tolist())
            assert a == w, (case, setting, "batch element", b, "pool read", int(pick[b]), reads[int(pick[b])].tolist()[:100], "got", a, "want", w)
        raise AssertionError((case, "slots beyond the count differ"))
    have = set(np.unique(status).tolist())
    want = {S.READ_OK, S.READ_BAD_BASE, H.READ_OVERFLOW} | ({S.READ_ABSENT_BASE} if name == "noT" else set())
    assert have == want | ({S.READ_TOO_SHORT} if mode != "bwa" and kind == "short" else set()), have
    assert int(counts.astype(np.int64).sum()) > N


# ------------------------------------------------------------------ reads of 256 .. 1409 bases through genie_find_smems_csr
LONG_CASES = [(name, order, mode, few) for name in REFS for order in ("shuffled", "runs") for mode in (MODES[1], MODES[2]) for few in (False, True)]


@pytest.mark.parametrize("case", LONG_CASES, ids=lambda c: f"{c[0]}-{c[1]}-{_mode_id(c[2])}-{'16lanes' if c[3] else '2lanes'}")
def test_csr_mid_lengths(pkg, case):
    """match_table_long_kernel (one read per group), traverse_long_kernel with two lanes per read (N >= 32768) and, under one
    block per CU, with sixteen (N < 32768), interval_kernel with CSR rows."""
    name, order, (mode, min_len), few = case
    setting = SETTINGS[LONG_CASES.index(case) % 2]
    ix, K = _index(pkg, name, setting)
    opt = pkg._native.OPT_SEARCH_BLOCKS_PER_CU
    try:
        if few:
            ix.set_option(opt, 1)
        N = _size(ix, 1409)
        if few:
            assert N < 32768, N
        else:
            N = max(N, 32769)
        _check_csr(ix, K, name, "mid", order, N, mode, min_len, (case, setting))
    finally:
        ix.set_option(opt, 0)


# ------------------------------------------------------------------ launch options
def _options(N):
    return ([{N.OPT_SCHEDULING: v} for v in (1, 2, 8, 15)] + [{N.OPT_GROUP_POSITIONS: v} for v in (1, 64)]
            + [{N.OPT_SEARCH_BLOCKS_PER_CU: 1}, {N.OPT_SEARCH_ALL: 1}])


OPTION_CASES = [(name, i, ("runs", "tail")[(i + j) % 2]) for j, name in enumerate(("tandem7", "noT")) for i in range(8)]
OPTION_NAMES = ["scheduling1", "scheduling2", "scheduling8", "scheduling15", "group1", "group64", "blocks1", "all"]


@pytest.mark.parametrize("case", OPTION_CASES, ids=lambda c: f"{c[0]}-{OPTION_NAMES[c[1]]}-{c[2]}")
def test_launch_options_against_brute_force(pkg, case):
    """Every setting against the brute force, not against the default run: GENIE_OPT_SCHEDULING 1 (no hand-out: groups by
    grid stride), 2 (no priority rotation), 8 (no touch ahead), 15 (all of them, and the interval kernels' rotation off);
    GENIE_OPT_GROUP_POSITIONS 1 (one read per group) and 64; one block per CU; every position looked up."""
    name, i, order = case
    native = pkg._native
    setting = _options(native)[i]
    assert len(_options(native)) == len(OPTION_NAMES)
    ix, K = _index(pkg, name, SETTINGS[i % 3])
    mode, min_len = MODES[1 + i % 3]
    try:
        for opt, value in setting.items():
            ix.set_option(opt, value)
        N = _size(ix, 255, rows_kernel=True)
        _check_csr(ix, K, name, "short", order, N, mode, min_len, (case, mode, min_len))
    finally:
        for opt in (native.OPT_SCHEDULING, native.OPT_GROUP_POSITIONS, native.OPT_SEARCH_BLOCKS_PER_CU, native.OPT_SEARCH_ALL):
            ix.set_option(opt, 0)
