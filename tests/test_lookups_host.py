"""CPU-only: the brute-force reference of tests/lookup_util.py is checked before the device is judged by it
(test_lookups_gpu.py) -- against the goldens of the unmodified reference, the known answers, the native suffix-array
builder and the CPU oracle."""
import numpy as np
import pytest

import golden_util as G
import lookup_util as U


@pytest.fixture(scope="module")
def pkg():
    import genie_smem_amd as g
    g._native.build()
    g._native.lib()
    return g


FAMILY = U.family()


def test_family_shape():
    assert len(FAMILY) == 18 and max(len(r) for r in FAMILY.values()) == U.MAX_N
    assert sorted(len(FAMILY[f"rand{n}"]) for n in (1, 2, 5, 37)) == [1, 2, 5, 37]
    for tail in U.TAILS:
        ref = FAMILY["tail_" + (tail or "none")]
        assert len(ref) == 300 + len(tail) and G.codes_to_str(ref[300:]) == tail
    for u, unit in U.TANDEM_UNITS.items():
        ref = FAMILY[f"tandem{u}"]
        want = np.tile(G.str_to_codes(unit), 3000)[:3000]
        assert len(ref) == 3000 and np.nonzero(ref != want)[0].tolist() == [U.TANDEM_BREAK]
    assert 3 not in FAMILY["noT"] and set(FAMILY["noT"].tolist()) == {0, 1, 2}


@pytest.mark.parametrize("ds", ["medium_K6", "syn10k_K8"])
def test_interval_reproduces_golden_back_prop(oracle_mod, ds):
    """Every g5 pattern of the golden; a reference of more than 4096 bases is cut to its first 4096 and the CPU oracle's
    back_prop on the cut reference is the expectation instead."""
    d, _ = G.load(ds)
    ref = d["ref_codes"]
    off, pat, want = d["g5.pat_off"], d["g5.pat"], d["g5.lohi"]
    cut = len(ref) > U.MAX_N
    if cut:
        ref = ref[:U.MAX_N]
        o = oracle_mod.Oracle(ref, 0)
    rows = U.suffix_rows(ref)
    present = 0
    for i in range(len(off) - 1):
        p = pat[off[i]:off[i + 1]]
        exp = o.back_prop(p) if cut else (int(want[i, 0]), int(want[i, 1]))
        assert U.interval(ref, rows, p) == tuple(exp), (ds, i)
        present += exp[0] >= 0
    assert 0 < present < len(off) - 1


def test_known_answers_mississippi():
    k = G.known()["mississippi"]
    ref = G.str_to_codes(k["ref"], "imps")
    rows = U.suffix_rows(ref)
    assert (rows + 1).tolist() == k["fm"]["sa_head"]
    for q, want in k["back_prop"].items():
        got = U.interval(ref, rows, G.str_to_codes(q, "imps"))
        assert got == ((-1, -1) if want == -1 else tuple(want)), q
    for q, pos in k["exact_match"].items():
        assert sorted(U.positions(rows, *U.interval(ref, rows, G.str_to_codes(q, "imps")))) == pos, q
    assert U.positions(rows, *U.interval(ref, rows, G.str_to_codes("ssi", "imps"))) == [6, 3]     # row order
    assert U.positions(rows, -1, -1) == U.positions(rows, -2, -2) == U.positions(rows, 5, 4) == []


@pytest.mark.parametrize("name", list(FAMILY))
def test_suffix_rows_equal_the_native_suffix_array(pkg, name):
    ref = FAMILY[name]
    rows = U.suffix_rows(ref)
    assert rows[0] == len(ref) and sorted(rows.tolist()) == list(range(len(ref) + 1))
    assert (rows + 1).tolist() == pkg.GenieIndex.build(ref, 0, dir_bits=3).suffix_array().tolist()
    assert U.interval(ref, rows, np.zeros(0, np.uint8)) == (0, len(ref))


def _plain_model(n, K, experts):
    """A model that spreads the K-mer codes evenly over the rows: good enough to start a search anywhere."""
    span = float(4 ** K)
    sizes = [1] + list(experts)
    coefs, icpts = [], []
    for l, size in enumerate(sizes):
        target = experts[l] if l < len(experts) else n + 1
        coefs.append(np.full(size, target / span))
        icpts.append(np.full(size, 0.25 * l))
    return coefs, icpts


@pytest.mark.parametrize("name,K", [("rand37", 3), ("tail_TTTTTTTT", 8), ("tail_CAAAAAA", 8), ("tandem7", 12),
                                    ("tandem1", 3), ("noT", 8), ("rand4096", 16)])
def test_kmer_interval_equals_oracle_rmi_suffix(oracle_mod, name, K):
    ref = FAMILY[name]
    rows = U.suffix_rows(ref)
    o = oracle_mod.Oracle(ref, K)
    o.set_rmi([10], *_plain_model(len(ref), K, [10]))
    own = np.lib.stride_tricks.sliding_window_view(ref, K)[::max(1, len(ref) // 100)]           # some that occur
    kmers = np.concatenate([own, U.kmers_for(ref, K, 7)])
    sel = np.arange(len(own))
    sel = np.union1d(sel,np.random.default_rng(K).choice(len(kmers), min(300, len(kmers)), replace=False))
    sel = np.union1d(sel, np.arange(len(kmers) - 4 * min(K, len(ref) + 1), len(kmers)))        # the padded tails
    hits = 0
    for i in sel:
        rc, lo, hi = o.rmi_suffix(kmers[i])
        assert rc == 0 and (lo, hi) == U.kmer_interval(ref, rows, kmers[i]), (name, K, kmers[i].tolist())
        if hi >= lo:
            hits += 1
            assert (lo, hi) == U.interval(ref, rows, kmers[i])
        else:
            assert U.interval(ref, rows, kmers[i]) == (-1, -1)
    assert 0 < hits < len(sel)


def test_rmi_predict_equals_oracle_bit_for_bit(pkg, oracle_mod):
    ref = FAMILY["rand4096"]
    K = 8
    models = []
    for experts in ([10], [10, 100], [4, 16, 64]):
        coefs, icpts, _, _, _ = pkg.GenieIndex.build(ref, K, dir_bits=3).train_rmi(experts)
        models.append((experts, coefs, icpts))
    rng = np.random.default_rng(11)
    models.append(([7, 5], [rng.normal(0, 1e-3, s) for s in (1, 7, 5)], [rng.normal(0, 3, s) for s in (1, 7, 5)]))
    codes = np.concatenate([np.arange(0, 4 ** K, 97), [4 ** K - 1]])
    for experts, coefs, icpts in models:
        o = oracle_mod.Oracle(ref, K)
        o.set_rmi(experts, coefs, icpts)
        sizes, scales = [len(c) for c in coefs], list(experts) + [1]
        coef, icpt = np.concatenate(coefs), np.concatenate(icpts)
        got = np.asarray([U.rmi_predict(sizes, scales, coef, icpt, int(c)) for c in codes], np.float64)
        want = np.asarray([o.rmi_predict(int(c)) for c in codes], np.float64)
        assert (got.view(np.uint64) == want.view(np.uint64)).all(), experts


def test_pattern_family_is_deterministic_and_covers_its_lengths():
    ref = FAMILY["tandem7"]
    a = U.patterns("tandem7", ref, 3, 5, 4097, 1)
    b = U.patterns("tandem7", ref, 3, 5, 4097, 1)
    assert len(a) == 4097 and all(x.tolist() == y.tolist() for x, y in zip(a, b))
    assert {len(p) for p in a} >= set(U.pattern_lengths(3, 5)) >= {3, 4, 5, 6, 35, 36, 39, 63, 64, 65, 95, 96, 97, 150, 1000}
    assert max(int(p.max()) for p in a if len(p)) <= 3
    short = U.patterns("rand5", FAMILY["rand5"], 7, 8, 4097, 2)
    assert sum(len(p) > 5 for p in short) > 1000 and any(U.runs_off_end(FAMILY["rand5"], p) for p in short)
