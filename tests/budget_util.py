"""The reference, the entry classes and the read batches of the block-budget tests (test_block_budget_host.py,
test_block_budget_gpu.py).  No GPU here.

The compact match table gives a P2-mer with 7 .. 13 suffixes, none cut short, five keys in its entry plus one overflow block
of eight; a block is reached through a 16-bit index, so an image holds at most kM16MaxOv - 1 = 65535 of them, handed out in
the order of the P2-mer codes.  Every eligible entry after the 65535th is written as "the rows decide" (cnt4 = 6, nib =
kM16General) although none of its suffixes is cut short: a "starved" entry.  REF is the smallest random reference found
that exhausts the budget (at table_bits 9: 90 821 entries with 7 .. 13 suffixes, 65 535 served, 25 286 starved, 5 of these
because a suffix is cut short); with automatic knobs the same happens from about 3 Mb to 16 Mb (4.1 Mb: P2 = 10, see test_block_budget_host.py).

Everything about the image is read from its serialized bytes (the host builder is the specification); the reads are
windows of REF that start at a suffix of a starved entry -- or of an entry that got a block, as the control -- left exact or
with one substitution that ends the match inside the entry's 8-base key, at its edge, or past anything an entry holds."""
import collections

import numpy as np

import smem_util as S
from test_host_index import _parse

N_REF = 1_500_000
REF = np.random.default_rng(1).integers(0, 4, N_REF).astype(np.uint8)
K = 12
KNOBS = dict(dir_bits=7, table_bits=9, table_format="compact")
P2 = 9
MAX_BLOCKS = 65535                          # kM16MaxOv - 1: block 0 is never referenced
M16_KEYS, M16_MORE, M16_GENERAL, M16_MIN_ROWS, M16_MAX_ROWS = 6, 7, 8, 7, 13
KEY_BASES = 8
SUB_OFFSETS = (0, 7, 8, 9, 15, 16, 17, 40)  # a substitution at P2 + j: inside the key, at its edge, past a wide key, far
READ_OK, READ_BAD_BASE, READ_TOO_SHORT = 0, 1, 2

_CACHE = {}


def index(pkg):
    """The host-built index of REF (one per process)."""
    if "index" not in _CACHE:
        _CACHE["index"] = pkg.GenieIndex.build(REF, K, **KNOBS)
    return _CACHE["index"]


def image(pkg, seed_table=True):
    """Its serialized image as a numpy uint8 array."""
    if ("image", seed_table) not in _CACHE:
        _CACHE["image", seed_table] = index(pkg).serialize(seed_table).numpy()
    return _CACHE["image", seed_table]


def oracle(oracle_mod):
    """The CPU oracle of REF (one per process)."""
    if "oracle" not in _CACHE:
        _CACHE["oracle"] = oracle_mod.Oracle(REF, K)
    return _CACHE["oracle"]


# ------------------------------------------------------------------ the image
SECTION_NAMES = ["sa", "ref", "dir", "lut", "rmi", "dir2", "rmi_err", "mtab", "ov"]


def section_of(img, at):
    """Name of the image section that holds byte `at` (for a readable failure)."""
    h = _parse(img)
    best, start = "header", 0
    for name in SECTION_NAMES:
        o = h["off_" + name]
        if start <= o <= at:
            best, start = name, o
    return best


def sections(img):
    """-> (header dict, dir2 records, match-table records, overflow blocks uint16 [ov_entries, 8], suffix starts (0-based)
    in row order)."""
    h = _parse(img)
    n = h["n"]
    head = np.frombuffer(bytes(img[h["off_dir2"]:h["off_dir2"] + 16 * h["dir2_entries"]]),
                         np.dtype([("lb", "<u4"), ("meta", "<u4"), ("key", "<u8")]))
    mtab = np.frombuffer(bytes(img[h["off_mtab"]:h["off_mtab"] + 16 * h["mtab_entries"]]), np.dtype([("w0", "<u4"), ("key", "<u2", (6,))]))
    ov = np.frombuffer(bytes(img[h["off_ov"]:h["off_ov"] + 16 * h["ov_entries"]]), "<u2").reshape(-1, 8)
    sa0 = np.frombuffer(bytes(img[h["off_sa"]:h["off_sa"] + 16 * (n + 1)]), "<i4").reshape(-1, 4)[:, 0].astype(np.int64)
    return h, head, mtab, ov, sa0


Classes = collections.namedtuple("Classes", "P2 n count lb cnt4 nib block starved cut sa0")


def entry_classes(img):
    """From the serialized image alone, per P2-mer: the row count (dir2 word 1 & 0x7fffffff), the first row, cnt4 (bits
    24 .. 27 of match-table word 0) and nib (bits 28 .. 31), and three masks: `block` (cnt4 == kM16More), `starved` (7 ..
    13 rows and no block) and `cut` (a suffix of the entry has fewer than P2 + 8 bases left, from the suffix-array
    section)."""
    h, head, mtab, _, sa0 = sections(img)
    assert h["flags"] & 2, "the compact table is what has a block budget"
    n, p2 = h["n"], h["P2"]
    count = (head["meta"] & 0x7FFFFFFF).astype(np.int64)
    lb = head["lb"].astype(np.int64)
    cnt4 = ((mtab["w0"] >> 24) & 15).astype(np.int64)
    nib = (mtab["w0"] >> 28).astype(np.int64)
    block = cnt4 == M16_MORE
    starved = (count >= M16_MIN_ROWS) & (count <= M16_MAX_ROWS) & ~block
    # rows whose suffix holds a P2-mer but fewer than P2 + 8 bases; the entry of a row: first rows ascend with the code
    rows = np.flatnonzero((n - sa0 >= p2) & (n - sa0 < p2 + KEY_BASES))
    present = np.flatnonzero(count > 0)
    assert (np.diff(lb[present]) > 0).all()
    owner = present[np.searchsorted(lb[present], rows, side="right") - 1]
    assert ((lb[owner] <= rows) & (rows < lb[owner] + count[owner])).all()
    cut = np.zeros(len(count), bool)
    cut[owner] = True
    return Classes(p2, n, count, lb, cnt4, nib, block, starved, cut, sa0)


def classes(pkg):
    if "classes" not in _CACHE:
        _CACHE["classes"] = entry_classes(image(pkg))
    return _CACHE["classes"]


def keys_after(ref, starts, p2, bases=KEY_BASES):
    """The `bases` bases after the P2-mer of every suffix start, 2 bits each, zero past the end of the reference."""
    starts = np.asarray(starts, np.int64)
    key = np.zeros(starts.shape, np.int64)
    for j in range(bases):
        p = starts + p2 + j
        key = (key << 2) | np.where(p < len(ref), ref[np.minimum(p, len(ref) - 1)], 0)
    return key


# ------------------------------------------------------------------ reads and the entries they touch
def window_codes(read, p2):
    """The P2-mer code at every position of a read that holds one (-1: fewer than P2 bases left, or a code > 3 in it)."""
    read = np.asarray(read, np.int64)
    out = np.full(len(read), -1, np.int64)
    if len(read) < p2:
        return out
    w = np.lib.stride_tricks.sliding_window_view(read, p2)
    code = (w << (2 * (p2 - 1 - np.arange(p2)))).sum(1)
    out[:len(code)] = np.where((w > 3).any(1), -1, code)
    return out


def positions_on(mask, reads, p2):
    """The number of read positions whose P2-mer falls in `mask` (a bool per P2-mer code)."""
    total = 0
    for r in reads:
        c = window_codes(r, p2)
        total += int(mask[c[c >= 0]].sum())
    return total


def positions(reads):
    return int(sum(len(r) for r in reads))


def starts_on(mask, reads, p2):
    """Does every read start with a P2-mer of `mask`?"""
    return all(len(r) >= p2 and window_codes(r[:p2], p2)[0] >= 0 and bool(mask[window_codes(r[:p2], p2)[0]]) for r in reads)


def from_ref(n_reads, length, seed):
    from genie_smem_amd import synth
    return list(synth.reads_from_ref(REF, n_reads, length, seed))


def random_reads(n_reads, length, seed):
    from genie_smem_amd import synth
    return list(synth.reads_random(n_reads, length, seed))


def _substitute(read, at, rng):
    read = read.copy()
    read[at] = (int(read[at]) + 1 + int(rng.integers(0, 3))) & 3
    return read


def class_starts(cls, mask, n_entries, length, rng):
    """Suffix starts of `n_entries` entries of `mask`, one row each (any of the entry's rows), with `length` bases left."""
    codes = rng.permutation(np.flatnonzero(mask))
    out = []
    for c in codes:
        s = int(cls.sa0[cls.lb[c] + int(rng.integers(0, cls.count[c]))])
        if s + length <= cls.n:
            out.append(s)
            if len(out) == n_entries:
                break
    assert len(out) == n_entries
    return out


def targeted(cls, mask, n_entries, length, seed, ref=REF):
    """Windows of the reference that start at a suffix of an entry of `mask`: one left exact, and one with a substitution
    at P2 + j for every j of SUB_OFFSETS that the length allows."""
    rng = np.random.default_rng(seed)
    out = []
    for s in class_starts(cls, mask, n_entries, length, rng):
        w = ref[s:s + length].copy()
        out.append(w)
        out += [_substitute(w, cls.P2 + j, rng) for j in SUB_OFFSETS if cls.P2 + j < length]
    return out


def ragged(cls, seed, ref=REF):
    """One read of every length 1 .. 255: a window at a suffix of a starved entry, every other one with a substitution."""
    rng = np.random.default_rng(seed)
    starts = class_starts(cls, cls.starved, 255, 255, rng)
    out = []
    for length, s in zip(range(1, 256), starts):
        w = ref[s:s + length].copy()
        if length % 2 == 0:
            w = _substitute(w, min(length - 1, cls.P2 + SUB_OFFSETS[(length // 2) % len(SUB_OFFSETS)]), rng)
        out.append(w)
    return out


def long_windows(cls, mask, lengths, seed, every, ref=REF):
    """Reads of the given lengths: windows at a suffix of an entry of `mask` with one substitution at P2 + j (j in turn
    from SUB_OFFSETS) and one in every `every` bases after it, so that matches of a few hundred bases follow each other."""
    rng = np.random.default_rng(seed)
    out = []
    for i, length in enumerate(lengths):
        s = class_starts(cls, mask, 1, length, rng)[0]
        w = _substitute(ref[s:s + length], cls.P2 + SUB_OFFSETS[i % len(SUB_OFFSETS)], rng)
        for at in range(every, length, every):
            w = _substitute(w, at + int(rng.integers(0, every // 2)) - every // 4, rng)
        out.append(w)
    return out


def batches(pkg):
    """{label: list of uint8 reads}: from-reference reads of 150 and 255 bases, random reads of 150, targeted reads of 150 and 255 on starved
    entries and on block entries (the control), the ragged batch, 705 and 1409 bases (match_table_long_kernel) and four
    reads of about 9000 (find_smems_long)."""
    if "batches" not in _CACHE:
        cls = classes(pkg)
        b = {"fromref150": from_ref(2000, 150, 7001),
             "fromref255": from_ref(300, 255, 7016),
             "random150": random_reads(500, 150, 7002),
             "starved150": targeted(cls, cls.starved, 24, 150, 7003),
             "block150": targeted(cls, cls.block, 24, 150, 7004),
             "starved255": targeted(cls, cls.starved, 8, 255, 7005),
             "block255": targeted(cls, cls.block, 8, 255, 7006),
             "ragged": ragged(cls, 7007),
             "mid705": long_windows(cls, cls.starved, [705] * 8, 7008, 180) + long_windows(cls, cls.block, [705] * 2, 7009, 180)
             + from_ref(6, 705, 7010),
             "mid1409": long_windows(cls, cls.starved, [1409] * 8, 7011, 250) + long_windows(cls, cls.block, [1409] * 2, 7012, 250)
             + from_ref(6, 1409, 7013),
             "long9000": long_windows(cls, cls.starved, [9000, 8999, 9001], 7014, 300) + from_ref(1, 9100, 7015)}
        _CACHE["batches"] = b
    return _CACHE["batches"]


TARGETED = {"starved150": "starved", "starved255": "starved", "block150": "block", "block255": "block"}


def with_breaks(reads, p2):
    """Copies of the reads with a break (code 4) planted at offset P2 - 1, P2 and mid-read, in turn."""
    out = []
    for i, r in enumerate(reads):
        r = r.copy()
        r[(p2 - 1, p2, len(r) // 2)[i % 3]] = 4
        out.append(r)
    return out


# ------------------------------------------------------------------ what the CPU oracle answers
NO_ROWS = np.zeros((0, 4), np.int32)


def expected_batch(orc, reads, mode, min_len=1):
    """The oracle's rows of a list of reads as a CSR entry point returns them: (offsets int64 [N + 1], rows int32 [S, 4],
    status int32 [N]).  A read the oracle refuses as shorter than K is READ_TOO_SHORT, one with a code > 3 READ_BAD_BASE;
    both have no rows."""
    status = {-3: READ_TOO_SHORT, -2: READ_BAD_BASE}
    parts, st = [NO_ROWS], []
    if max(len(r) for r in reads) <= 2048:
        mat, lens = S.matrix(reads, fill=0)
        counts, out = orc.find_smems_batch(mode, mat, min_len=min_len, nthreads=8, lens=lens)
        for i, c in enumerate(counts):
            st.append(READ_OK if c >= 0 else status[int(c)])
            parts.append(out[i, :max(int(c), 0)])
    else:
        for r in reads:
            c, rows = orc.find_smems(mode, r, min_len)
            st.append(READ_OK if c >= 0 else status[int(c)])
            parts.append(rows if c > 0 else NO_ROWS)
    off = np.zeros(len(reads) + 1, np.int64)
    off[1:] = np.cumsum([len(p) for p in parts[1:]])
    return off, np.concatenate(parts).astype(np.int32), np.asarray(st, np.int32)


def expected_split(orc, reads, min_len=1):
    """find_smems_split: the oracle's rows of every run between breaks (tests/split_util.py); the status is always 0."""
    import split_util
    parts = [split_util.split_rows(orc, r, min_len) for r in reads]
    off = np.zeros(len(reads) + 1, np.int64)
    off[1:] = np.cumsum([len(p) for p in parts])
    return off, np.concatenate([NO_ROWS] + parts).astype(np.int32), np.zeros(len(reads), np.int32)


def compare(got, want, reads, tag):
    """Offsets, rows and statuses of a CSR result against the expectation, exactly; names the first read that differs."""
    off, rows, st = (x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x) for x in got)
    woff, wrows, wst = want
    if off.tolist() == woff.tolist() and st.tolist() == wst.tolist() and rows.tolist() == wrows.tolist():
        return
    for r in range(len(wst)):
        a = (int(st[r]), rows[off[r]:off[r + 1]].tolist()) if r + 1 < len(off) else None
        b = (int(wst[r]), wrows[woff[r]:woff[r + 1]].tolist())
        assert a == b, (tag, "read", r, np.asarray(reads[r]).tolist()[:100], "got", a, "want", b)
    raise AssertionError((tag, "shapes", off.shape, woff.shape, rows.shape, wrows.shape))
