"""The K-mer hash table (the `lut` section of the index image) as the header and index_host.cpp define it, modelled in
plain NumPy, and references crafted so that the table holds what random references never give it: stretches of
thousands of occupied slots over several 1024-slot segment borders and across slot 0, carries in the hundreds, hundreds
of keys on one home slot.  Nothing here comes from the library under test; test_seed_table_host.py pins the model
against the host builder byte for byte.

The rule: the m distinct K-mer codes (first base in the top bits) are inserted in ascending order into S = 2 m + 8 slots
by linear probing from home = ((code * 0x9E3779B1 mod 2^32) * S) >> 32.  The multiplier is odd, so the hash is
invertible and a K-mer with a wanted home slot can be written down: with GINV its inverse mod 2^32, the hashed value y
belongs to the code y * GINV mod 2^32, and the y of home slot s are [ceil(s 2^32 / S), ceil((s + 1) 2^32 / S)).  For
K = 16 every 32-bit code is a K-mer; for a smaller K only the codes below 4^K are."""
import functools

import numpy as np

MULT = 0x9E3779B1
GINV = pow(MULT, -1, 2 ** 32)
MASK = 0xFFFFFFFF
SEG = 1024                      # slots per carry segment of the device builder
SLOT = np.dtype([("key", "<u4"), ("lo", "<i4"), ("hi", "<i4"), ("pad", "<u4")])


# ------------------------------------------------------------------ the model
def kmer_codes(ref, K):
    """Code of the K-mer at every position 0 .. n - K (int64; first base in the top bits)."""
    ref = np.asarray(ref, np.int64)
    n = len(ref)
    if n < K:
        return np.zeros(0, np.int64)
    c = np.zeros(n - K + 1, np.int64)
    for j in range(K):
        c = (c << 2) | ref[j:n - K + 1 + j]
    return c


def bases_of(codes, K):
    """uint8 [N, K] bases of the codes."""
    codes = np.asarray(codes, np.int64).reshape(-1)
    return ((codes[:, None] >> (2 * (K - 1 - np.arange(K)))) & 3).astype(np.uint8)


def homes(codes, S):
    y = (np.asarray(codes).astype(np.uint64) * np.uint64(MULT)) & np.uint64(MASK)
    return ((y * np.uint64(S)) >> np.uint64(32)).astype(np.int64)


def _suffix_keys(ref, K):
    """Per suffix start 0 .. n its first K symbols as a base-5 number: base + 1, 0 past the end ('$' sorts first)."""
    n = len(ref)
    d = np.zeros(n + K, np.int64)
    d[:n] = np.asarray(ref, np.int64) + 1
    key = np.zeros(n + 1, np.int64)
    for j in range(K):
        key = key * 5 + d[j:n + 1 + j]
    return key


def _kmer_keys(kmers):
    key = np.zeros(len(kmers), np.int64)
    for j in range(kmers.shape[1]):
        key = key * 5 + kmers[:, j].astype(np.int64) + 1
    return key


def kmer_intervals(ref, kmers):
    """int64 [N, 2]: per K-mer (first, last) of the suffix-array rows that start with it, row 0 = the empty suffix; an
    absent K-mer gives (first, first - 1), first = the row it would be inserted at.  The definition of
    lookup_util.kmer_interval, from the K leading symbols of every suffix instead of whole suffix strings, so that it
    works past 4096 bases."""
    kmers = np.asarray(kmers, np.uint8)
    keys = np.sort(_suffix_keys(ref, kmers.shape[1]))
    q = _kmer_keys(kmers)
    return np.stack([np.searchsorted(keys, q, "left"), np.searchsorted(keys, q, "right") - 1], 1)


def carry_into(hcount):
    """The carry into every slot (keys that probe into it from the slot before): x -> max(0, x + h - 1) slot by slot,
    cyclic; a second pass from the first's end value closes it."""
    h = np.asarray(hcount).tolist()
    cin, x, ends = [0] * len(h), 0, []
    for _ in range(2):
        for j, v in enumerate(h):
            cin[j] = x
            x = x + v - 1
            if x < 0:
                x = 0
        ends.append(x)
    assert ends[0] == ends[1] == cin[0]
    return np.asarray(cin, np.int64)


class Table:
    """The seed table of (ref, K): codes (sorted distinct), S, home, hcount (homes per slot), carry (the carry INTO each
    slot: keys that probe into it from the slot before), flag (no carry in: a stretch starts here), starts / lengths of
    the stretches (slots from one flagged slot to the next, cyclic)."""

    def __init__(self, ref, K):
        self.ref, self.K = np.ascontiguousarray(ref, np.uint8), K
        self.codes = np.unique(kmer_codes(ref, K))
        self.m = len(self.codes)
        self.S = S = 2 * self.m + 8
        self.home = homes(self.codes, S)
        self.hcount = np.bincount(self.home, minlength=S)
        self.carry = carry_into(self.hcount)
        self.flag = self.carry == 0
        self.starts = np.flatnonzero(self.flag)
        self.lengths = np.diff(np.append(self.starts, self.starts[0] + S))
        self._slots = None

    def stretch_of(self, slot):
        """Index into starts / lengths of the stretch that holds `slot`."""
        return int(np.searchsorted(self.starts, slot % self.S, "right") - 1) % len(self.starts)

    def slots(self):
        """The slot array: the keys re-inserted one by one in ascending order, as the host does."""
        if self._slots is None:
            iv = kmer_intervals(self.ref, bases_of(self.codes, self.K))
            S, used, at = self.S, [False] * self.S, []
            for p in self.home.tolist():
                while used[p]:
                    p = p + 1 if p + 1 < S else 0
                used[p] = True
                at.append(p)
            out = np.zeros(S, SLOT)
            out["lo"] = out["hi"] = -1
            out["key"][at], out["lo"][at], out["hi"][at] = self.codes, iv[:, 0], iv[:, 1]
            self._slots = out
        return self._slots

    def probes(self, codes):
        """Slots a lookup of each code reads: from its home up to the slot that holds it or the first empty one."""
        sl = self.slots()
        key, used, S = sl["key"].tolist(), (sl["lo"] >= 0).tolist(), self.S
        out = []
        for c, p in zip(np.asarray(codes).tolist(), homes(codes, S).tolist()):
            t = 1
            while used[p] and key[p] != c:
                p = p + 1 if p + 1 < S else 0
                t += 1
            out.append(t)
        return np.asarray(out, np.int64)

    def summary(self):
        S = self.S
        i = int(np.argmax(self.lengths))
        first, length = int(self.starts[i]), int(self.lengths[i])
        last = first + length - 1
        borders = last // SEG - first // SEG if last < S else (S - 1) // SEG - first // SEG + (last - S) // SEG
        return {"S": S, "S_mod_seg": S % SEG, "segments": -(-S // SEG), "stretch_first": first, "stretch_slots": length,
                "stretch_borders": int(borders), "stretch_wraps": last >= S, "max_carry": int(self.carry.max()),
                "carry_into_0": int(self.carry[0]), "max_homes": int(self.hcount.max())}


# ------------------------------------------------------------------ crafting
_HOME_OF_ALL = {}


def codes_homed_on(K, S, slots, rng):
    """One K-mer code per entry of `slots`, homed on that slot of a table of S slots, drawn with rng."""
    slots = np.asarray(slots, np.int64).reshape(-1)
    if K == 16:
        out = []
        for s in slots.tolist():
            lo, hi = -((-s << 32) // S), -((-(s + 1) << 32) // S)
            out.append(int(rng.integers(lo, hi)) * GINV & MASK)
        out = np.asarray(out, np.int64)
    else:                                   # scan: which of the 4^K codes land on the wanted slots (about one y in 4^(16-K))
        if (K, S) not in _HOME_OF_ALL:
            _HOME_OF_ALL.clear()
            _HOME_OF_ALL[K, S] = homes(np.arange(4 ** K, dtype=np.int64), S).astype(np.int32)
        home = _HOME_OF_ALL[K, S]
        need = np.zeros(S, bool)
        need[slots] = True
        pool = np.flatnonzero(need[home])
        pool = pool[np.argsort(home[pool], kind="stable")]
        ph = home[pool]
        a, b = np.searchsorted(ph, slots, "left"), np.searchsorted(ph, slots, "right")
        assert (b > a).all(), "no %d-mer is homed on some wanted slot" % K
        out = pool[a + (rng.random(len(slots)) * (b - a)).astype(np.int64)].astype(np.int64)
    assert (homes(out, S) == slots).all()
    return out


def craft(K, c, place, seed):
    """A reference of c crafted K-mers back to back (n = K c).  place(S, rng) gives the c wanted home slots in a table
    of S = 2 (n - K + 1) + 8 slots; the other K-mers of the reference, K - 1 per junction, are background.  A crafted
    K-mer that makes two K-mers of the reference equal is redrawn, so that the table has exactly S slots.
    -> (uint8 codes, the wanted homes)."""
    rng = np.random.default_rng(seed)
    n = K * c
    S = 2 * (n - K + 1) + 8
    want = np.asarray(place(S, rng), np.int64) % S
    assert want.shape == (c,)
    blocks = codes_homed_on(K, S, want, rng)
    while True:
        ref = bases_of(blocks, K).reshape(-1)
        allc = kmer_codes(ref, K)
        order = np.argsort(allc, kind="stable")
        again = order[1:][allc[order[1:]] == allc[order[:-1]]]          # a position whose K-mer stood further left too
        if not len(again):
            return ref, want
        redo = np.unique(again // K)
        blocks[redo] = codes_homed_on(K, S, want[redo], rng)


def absent_codes_homed_on(table, slots, rng):
    """codes_homed_on for K-mers that the table does not hold."""
    out = codes_homed_on(table.K, table.S, slots, rng)
    while True:
        held = np.isin(out, table.codes)
        if not held.any():
            return out
        out[held] = codes_homed_on(table.K, table.S, np.asarray(slots)[held], rng)


def random_ref_with_slots(S, seed):
    """A random reference whose K = 16 table has exactly S slots (the prefix of one random stream with S / 2 - 4
    distinct 16-mers)."""
    m = S // 2 - 4
    stream = np.random.default_rng(seed).integers(0, 4, m + 15 + 64).astype(np.uint8)
    first = np.unique(kmer_codes(stream, 16), return_index=True)[1]     # where each distinct 16-mer stands first
    n = int(np.sort(first)[m - 1]) + 16                                 # the prefix that ends with the m-th of them
    return stream[:n]


# ------------------------------------------------------------------ the cases
C_KEYS = 1400                   # crafted keys of mid, wrap, back_to_back and k12
C_PILE = 700
MID_START = 5000
PILE_SLOT = 5000
B2B_START = 3000
B2B_NEAR = 8                    # "within a few slots"


def _window(start_of, c):
    return lambda S, rng: start_of(S) + rng.integers(0, c, c)


B2B_HEAD = 20                   # keys homed on the second window's first slot: its stretch starts exactly there


def _b2b_place(second):
    h = C_KEYS // 2

    def place(S, rng):
        a, b = B2B_START + rng.integers(0, h, h), second + rng.integers(0, h, h)
        b[:B2B_HEAD] = second
        return np.concatenate([a, b])
    return place


def b2b_stretches(table, second):
    """(first slot, slots) of the stretches holding the last slot of the window at B2B_START and of the window at
    `second` (where the carry of a window is largest), and whether they are two."""
    i, j = table.stretch_of(B2B_START + C_KEYS // 2 - 1), table.stretch_of(second + C_KEYS // 2 - 1)
    return (int(table.starts[i]), int(table.lengths[i])), (int(table.starts[j]), int(table.lengths[j])), i != j


def b2b_ok(table, second):
    a, b, two = b2b_stretches(table, second)
    return two and 0 <= b[0] - (a[0] + a[1]) <= B2B_NEAR and min(a[1], b[1]) >= C_KEYS // 2


def _back_to_back(seed):
    """Where the first window's stretch ends depends on the background K-mers, half of which move with the second
    window, so the second window's start is searched: candidates around the end found with the second window far away,
    in a fixed order, each checked on the table that results."""
    ref, _ = craft(16, C_KEYS, _b2b_place(B2B_START + 4 * C_KEYS), seed)
    t = Table(ref, 16)
    i = t.stretch_of(B2B_START + C_KEYS // 2 - 1)
    end = int(t.starts[i] + t.lengths[i])
    for k in range(96):
        second = end - 16 + k % 48
        ref, want = craft(16, C_KEYS, _b2b_place(second), seed + 1000 * (k // 48))
        if b2b_ok(Table(ref, 16), second):
            return ref, want, second
    raise AssertionError("no back-to-back placement found")


CRAFTED = ["mid", "wrap", "pile", "back_to_back", "k12"]
SEGMENT_EDGE = {"rem0": 22 * SEG, "rem2": 22 * SEG + 2, "rem1022": 22 * SEG + 1022, "seg256": 256 * SEG, "seg257": 256 * SEG + 2}
CASES = CRAFTED + list(SEGMENT_EDGE)


class Case:
    def __init__(self, name, ref, K, want=None, second=None):
        self.name, self.ref, self.K, self.want, self.second = name, ref, K, want, second
        self.table = Table(ref, K)
        self.summary = self.table.summary()


@functools.lru_cache(maxsize=None)
def case(name, seed=1):
    if name == "mid":
        return Case(name, *craft(16, C_KEYS, _window(lambda S: MID_START, C_KEYS), seed)[:1], 16)
    if name == "wrap":
        return Case(name, *craft(16, C_KEYS, _window(lambda S: S - C_KEYS // 2, C_KEYS), seed)[:1], 16)
    if name == "pile":
        ref, want = craft(16, C_PILE, lambda S, rng: np.full(C_PILE, PILE_SLOT), seed)
        return Case(name, ref, 16, want)
    if name == "back_to_back":
        ref, want, second = _back_to_back(seed)
        return Case(name, ref, 16, want, second)
    if name == "k12":
        return Case(name, *craft(12, C_KEYS, _window(lambda S: MID_START, C_KEYS), seed)[:1], 12)
    return Case(name, random_ref_with_slots(SEGMENT_EDGE[name], 40 + seed), 16)


def lookups(cs, seed=7):
    """The K-mers a case is asked for -> (uint8 [N, K] K-mers, int32 [N, 2] what LUT mode answers, probes int64 [N]):
    every key of the table; absent keys homed on the first slot of the longest stretch (they read all of it and the
    empty slot behind), on its last slots, and on the last slots of the table; K-mers with a code above 3.  probes is
    the model's count of slots each lookup reads (0 for the K-mers that are refused)."""
    t, rng = cs.table, np.random.default_rng(seed)
    s = cs.summary
    first, length = s["stretch_first"], s["stretch_slots"]
    at = np.concatenate([np.full(8, first), first + length - 1 - np.arange(8), t.S - 1 - np.arange(8)]) % t.S
    absent = absent_codes_homed_on(t, at, rng)
    codes = np.concatenate([t.codes, absent])
    kmers = bases_of(codes, t.K)
    iv = kmer_intervals(t.ref, kmers)
    present = iv[:, 1] >= iv[:, 0]
    assert present[:t.m].all() and not present[t.m:].any()
    want = np.where(present[:, None], iv, -1)
    bad = kmers[rng.integers(0, t.m, 6)].copy()
    bad[np.arange(6), [0, t.K - 1, 3, 5, 7, 0]] = [4, 4, 5, 255, 128, 7]
    return (np.ascontiguousarray(np.concatenate([kmers, bad])), np.concatenate([want, np.full((6, 2), -2)]).astype(np.int32),
            np.concatenate([t.probes(codes), np.zeros(6, np.int64)]))


# ------------------------------------------------------------------ images
def sections(img):
    """name -> (offset, end) of the sections of an index image, from its header (int64 words: off_sa, off_ref, off_dir,
    off_lut, off_rmi = 5 .. 9, lut_slots 12, off_dir2 26, off_rmi_err 29, off_mtab 31, off_ov 33, total_bytes 2)."""
    hdr = np.ascontiguousarray(img[:512]).view(np.int64)
    offs = {"sa": hdr[5], "ref": hdr[6], "dir": hdr[7], "lut": hdr[8], "rmi": hdr[9], "dir2": hdr[26], "rmi_err": hdr[29],
            "mtab": hdr[31], "ov": hdr[33]}
    names = sorted(offs, key=lambda k: int(offs[k]))
    ends = [int(offs[k]) for k in names[1:]] + [int(hdr[2])]
    return {k: (int(offs[k]), e) for k, e in zip(names, ends)}


def lut_section(img):
    """The slot array of an image as bytes: lut_slots 16-byte slots from off_lut."""
    hdr = np.ascontiguousarray(img[:512]).view(np.int64)
    return img[int(hdr[8]):int(hdr[8]) + 16 * int(hdr[12])], int(hdr[12])


def where(img, off):
    """Name of the image section holding byte `off` (for a readable failure)."""
    for name, (a, b) in sections(img).items():
        if a <= off < b:
            return name
    return "header"


def same_image(pkg, codes, K, table_bits=0, table_format="auto", seed_table=True):
    """test_device_index_build._same: the device-built image equals the host-built one byte for byte."""
    host = pkg.GenieIndex.build(codes, K, table_bits=table_bits, table_format=table_format)
    want = host.serialize(seed_table).numpy()
    dev = pkg.GenieIndex.build_on_device(codes, K, table_bits=table_bits, table_format=table_format, seed_table=seed_table)
    got = dev.blob.cpu().numpy()
    tag = (codes.size, K, table_bits, table_format, seed_table)
    assert got.size == want.size, tag
    if not np.array_equal(got, want):
        off = int(np.flatnonzero(got != want)[0])
        raise AssertionError(f"{tag}: first difference at byte {off} ({where(want, off)} section)")
    return host, dev
