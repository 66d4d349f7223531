"""CPU-only: the NumPy model of the K-mer hash table (tests/seed_table_util.py) and the crafted references, before the
device builder is judged on them (test_seed_table_gpu.py).  Every case's table really holds what the case is for --
long stretches over segment borders and across slot 0, large carries, a pile of homes on one slot -- by the model
alone; and the model's slot array equals the `lut` section of the host builder's image byte for byte."""
import numpy as np
import pytest

import lookup_util as L
import seed_table_util as U


@pytest.fixture(scope="module")
def pkg():
    import genie_smem_amd as g
    g._native.build()
    g._native.lib()
    return g


def test_hash_inverse_and_orientation(pkg):
    assert U.MULT * U.GINV % 2 ** 32 == 1
    rng = np.random.default_rng(5)
    for K in (12, 16):
        ref = rng.integers(0, 4, 3000).astype(np.uint8)
        t = U.Table(ref, K)
        ix = pkg.GenieIndex.build(ref, K)
        codes, lo, hi = ix.lut_arrays()                                   # views into ix
        assert np.array_equal(codes.astype(np.int64), t.codes)            # first base in the top bits
        assert U.kmer_codes(ref, K)[0] == L.kmer_code(ref[:K])
        iv = U.kmer_intervals(ref, U.bases_of(t.codes, K))
        assert np.array_equal(iv[:, 0], lo) and np.array_equal(iv[:, 1], hi)
        for s in (0, 1, t.S // 2, t.S - 1):
            assert (U.homes(U.codes_homed_on(K, t.S, np.full(5, s), rng), t.S) == s).all()


@pytest.mark.parametrize("name,K", [("rand37", 3), ("tail_TTTTTTTT", 8), ("tandem7", 12), ("rand4096", 16), ("rand5", 16)])
def test_kmer_intervals_equal_the_sorted_suffix_strings(name, K):
    """kmer_intervals (the K leading symbols of each suffix) against lookup_util.kmer_interval (whole suffix strings,
    at most 4096 bases): K-mers that occur, that do not, and the reference's tail padded to K."""
    ref = L.family()[name]
    rows = L.suffix_rows(ref)
    kmers = L.kmers_for(ref, K, 9)
    if len(kmers) > 1500:
        kmers = np.concatenate([kmers[::len(kmers) // 1000], kmers[-4 * K:]])
    got = U.kmer_intervals(ref, kmers)
    want = np.asarray([L.kmer_interval(ref, rows, k) for k in kmers])
    assert np.array_equal(got, want)
    assert len(ref) < K or ((want[:, 1] >= want[:, 0]).any() and (want[:, 1] < want[:, 0]).any())


def test_carry_model_on_a_hand_table():
    """homes per slot 0 0 3 0 0 1 1 0 | 2: the carry into each slot and the stretches, by hand (cyclic: the two keys on
    the last slot carry one into slot 0)."""
    assert U.carry_into([0, 0, 3, 0, 0, 1, 1, 0, 2]).tolist() == [1, 0, 0, 2, 1, 0, 0, 0, 0]
    assert U.carry_into([1, 1, 1, 0]).tolist() == [0, 0, 0, 0]
    assert U.carry_into([0, 0, 0, 3]).tolist() == [2, 1, 0, 0]


@pytest.mark.parametrize("name", U.CASES)
def test_case_conditions(name):
    cs = U.case(name)
    s, t = cs.summary, cs.table
    print(name, "n", len(cs.ref), "K", cs.K, s)
    assert t.m == len(cs.ref) - cs.K + 1 or name in U.SEGMENT_EDGE
    assert (10_000 <= len(cs.ref) <= 25_000) or name in ("seg256", "seg257")
    assert t.flag.any() and (t.slots()["lo"] < 0).sum() == t.S - t.m
    if name in ("mid", "wrap"):
        assert s["stretch_slots"] >= 2049 and s["stretch_borders"] >= 2 and s["max_carry"] >= 500
    if name == "wrap":
        first, length = s["stretch_first"], s["stretch_slots"]
        assert first <= t.S - 1 < first + length and first + length > t.S      # holds slot S - 1 and slot 0
        assert s["stretch_wraps"] and s["S_mod_seg"] != 0 and s["carry_into_0"] >= 100
        assert not t.flag[0] and not t.flag[t.S - 1]
    if name == "pile":
        assert s["max_homes"] >= 500 and t.hcount[U.PILE_SLOT] == s["max_homes"]
        i = t.stretch_of(U.PILE_SLOT)
        first, last = int(t.starts[i]), int(t.starts[i] + t.lengths[i] - 1)
        assert last < t.S and last // U.SEG - first // U.SEG >= 1
    if name == "back_to_back":
        a, b, two = U.b2b_stretches(t, cs.second)
        assert two and 0 <= b[0] - (a[0] + a[1]) <= U.B2B_NEAR and min(a[1], b[1]) >= U.C_KEYS // 2
        assert b[0] == cs.second and t.flag[a[0] + a[1]] and t.flag[b[0]]       # the no-carry flags between the two
    if name == "k12":
        assert cs.K == 12 and (t.codes < 4 ** 12).all() and s["stretch_borders"] >= 1
    if name in U.SEGMENT_EDGE:
        assert t.S == U.SEGMENT_EDGE[name]
        assert (s["S_mod_seg"], s["segments"]) == {"rem0": (0, 22), "rem2": (2, 23), "rem1022": (1022, 23),
                                                   "seg256": (0, 256), "seg257": (2, 257)}[name]


@pytest.mark.parametrize("name", U.CASES)
def test_model_equals_host_table(pkg, name):
    cs = U.case(name)
    img = pkg.GenieIndex.build(cs.ref, cs.K).serialize().numpy()
    sec, slots = U.lut_section(img)
    a, b = U.sections(img)["lut"]
    assert slots == cs.table.S and a % 16 == 0 and a + 16 * slots <= b
    want = cs.table.slots().tobytes()
    got = sec.tobytes()
    if got != want:
        g, w = np.frombuffer(got, U.SLOT), np.frombuffer(want, U.SLOT)
        bad = int(np.flatnonzero(g != w)[0])
        raise AssertionError(f"{name}: slot {bad}: host {g[bad]}, model {w[bad]}")
    assert not img[a + 16 * slots:b].any()


@pytest.mark.parametrize("name", U.CRAFTED)
def test_lookup_plan(name):
    """The lookups the device is asked: absent keys read the whole longest stretch and the empty slot behind it."""
    cs = U.case(name)
    kmers, want, probes = U.lookups(cs)
    s = cs.summary
    print(name, "longest probe sequence", int(probes.max()))
    assert probes.max() >= s["stretch_slots"] + 1                         # up to the first empty slot behind the stretch
    assert (want[:cs.table.m, 0] >= 0).all() and (want[cs.table.m:-6] == -1).all() and (want[-6:] == -2).all()
    assert (kmers[-6:] > 3).any(1).all() and (kmers[:-6] <= 3).all()
    if name in ("mid", "wrap", "k12"):
        assert probes.max() >= 2000
    if name == "wrap":                      # from the last slots of the table across slot 0
        h = U.homes([L.kmer_code(k) for k in kmers[cs.table.m:-6]], cs.table.S)
        assert ((h >= cs.table.S - 8) & (probes[cs.table.m:-6] > 8)).sum() >= 8
