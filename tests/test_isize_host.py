"""CPU-only tests of genie_insert_size_stats (the insert-size distribution of a paired batch, estimated from the batch): the
brute force of tests/isize_util.py pinned on hand-written cases with literal expected rows, the exported symbols, every argument
check in the documented order on a handle without a device, the workspace formula, and index.insert_size_options."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import isize_util as IU
from isize_util import CAPACITY, INVALID, NO_DEVICE, TOO_LONG
from pair_util import FR, NO_TYPE, RF, SAME

P = IU.Params
ONE = P(20, 10000, 1)


@pytest.fixture(scope="module")
def pkg():
    import genie_smem_amd as g
    g._native.build()
    return g


def _rows(samples, p=ONE):
    return IU.stats_of(samples, p).tolist()


# ------------------------------------------------------------------ the definition, by hand
def test_ranks_for_one_to_nine_samples():
    ranks = {1: (0, 0, 0), 2: (0, 1, 1), 3: (1, 1, 2), 4: (1, 2, 3), 5: (1, 2, 4), 6: (1, 3, 4), 7: (2, 3, 5), 8: (2, 4, 6), 9: (2, 4, 7)}
    for n, (a, b, c) in ranks.items():
        assert (a, b, c) == tuple(min(n - 1, int(p * n + .499)) for p in (.25, .5, .75))        # BWA's, kept inside the samples
        v = [10 * (i + 1) for i in range(n)]
        rows = _rows([(RF, s) for s in reversed(v)])
        assert rows[1][:5] == [n, 1, 10 * (a + 1), 10 * (b + 1), 10 * (c + 1)], n
        assert rows[0] == [0] * 12 and rows[2] == [0] * 12


def test_all_spans_equal():
    assert _rows([(FR, 350)] * 30) == [[30, 1, 350, 350, 350, 350, 350, 30, 350, 0, 350, 350], [0] * 12, [0] * 12]
    assert _rows([(SAME, 1)] * 3)[2] == [3, 1, 1, 1, 1, 1, 1, 3, 1, 0, 1, 1]


def test_a_far_outlier_is_left_out():
    v = [100, 101, 102, 103, 104, 105, 106, 107, 5000]
    # IQR 5: bounds 92 and 117; the mean of the eight is 103.5 -> 104; SS 44 over 8: 2^2 8 < 44 <= 3^2 8
    assert _rows([(FR, s) for s in v])[0] == [9, 1, 102, 104, 107, 92, 117, 8, 104, 3, 87, 122]


def test_min_samples():
    p = P(20, 10000, 25)
    assert _rows([(FR, 300)] * 24, p)[0] == [24, 0, 300, 300, 300, 0, 0, 0, 0, 0, 0, 0]
    assert _rows([(FR, 300)] * 25, p)[0] == [25, 1, 300, 300, 300, 300, 300, 25, 300, 0, 300, 300]


def test_five_percent_rule():
    rf_ok = [5, 1, 500, 500, 500, 500, 500, 5, 500, 0, 500, 500]
    assert _rows([(FR, 300)] * 100 + [(RF, 500)] * 5)[1] == rf_ok                   # 20 * 5 == 100
    assert _rows([(FR, 300)] * 101 + [(RF, 500)] * 5)[1] == [5, 0, 500, 500, 500, 0, 0, 0, 0, 0, 0, 0]
    assert _rows([(SAME, 300)] * 101 + [(RF, 500)] * 5)[2][:2] == [101, 1]          # the largest type is any of the three


def test_window_is_clamped_at_both_ends():
    # q25 10, q75 200, IQR 190: 10 - 570 < 0 and 200 + 570 > 600; mean 105, SS 4 * 95^2, std 95
    assert _rows([(FR, s) for s in (200, 10, 10, 200)], P(20, 600, 1))[0] == [4, 1, 10, 200, 200, 1, 580, 4, 105, 95, 0, 600]
    assert _rows([(FR, s) for s in (200, 10, 10, 200)], P(20, 10000, 1))[0][10:] == [0, 770]


def test_std_is_a_ceiling():
    # SS = 4 = 1^2 * 4 exactly: std 1; SS = 5: std 2
    assert _rows([(FR, s) for s in (99, 99, 101, 101)])[0] == [4, 1, 99, 101, 101, 95, 105, 4, 100, 1, 93, 107]
    assert _rows([(FR, s) for s in (98, 100, 100, 101)])[0] == [4, 1, 100, 100, 101, 98, 103, 4, 100, 2, 92, 108]
    assert _rows([(FR, 98), (FR, 102)])[0] == [2, 1, 98, 102, 102, 90, 110, 2, 100, 2, 86, 114]      # SS 8 = 2^2 * 2


def test_expected_reads_heads_only():
    plan = [(FR, 300), (RF, 250, 19), (SAME, 400, 20), (NO_TYPE, 90), ("contigs", 300), "none", "left", "right", (FR, 10001), (FR, 10000),
            (FR, 300, 60, 19)]
    b = IU.batch_of(plan, extra=2)
    want = IU.expected(b, P(20, 10000, 1))
    assert want["samples"].tolist() == [[0, 300], [-1, 0], [2, 400], [-1, 0], [-1, 0], [-1, 0], [-1, 0], [-1, 0], [-1, 0], [0, 10000], [-1, 0]]
    assert want["totals"].tolist() == [8, 3, 2, 3]
    assert want["stats"][:, 0].tolist() == [2, 0, 1]
    cut = IU.expected(b, P(20, 10000, 1), n_records=1)               # mate 1 of pair 0 lost its records
    assert cut["samples"][0].tolist() == [-1, 0] and cut["totals"].tolist() == [0, 0, 0, 0]


# ------------------------------------------------------------------ the C layer
def test_insert_size_symbols_exported(pkg):
    lib = pkg._native.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "genie_smem.h")).read()
    for name, nargs, res in (("genie_insert_size_stats", 14, C.c_int), ("genie_insert_size_stats_workspace_bytes", 2, C.c_int64)):
        assert name in pkg._native.SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is res and len(fn.argtypes) == nargs
        assert name + "(" in header
    assert lib.genie_abi_version() == 2 and pkg._native.ABI_VERSION == 2      # an addition: the version stays
    for words in ("(n, ok, q25, q50, q75, lo_b, hi_b, n_in, mean, std, isize_min, isize_max)", "mean = floor((2 S + n_in) / (2 n_in))",
                  "the smallest d >= 0 with d d n_in >= SS", "20 n_t >= the largest n", "No atomic decides a value",
                  "every such sum is an integer add", "12 bytes per bin", "choices, not measurements"):
        assert words in header, words
    consts = dict(re.findall(r"#define (GENIE_[A-Z_]+) (\d+)", header))
    assert int(consts["GENIE_ISIZE_LDS_BINS"]) == pkg._native.ISIZE_LDS_BINS == IU.LDS_BINS
    assert (int(consts["GENIE_ISIZE_OUTLIER_IQR"]), int(consts["GENIE_ISIZE_WINDOW_IQR"]), int(consts["GENIE_ISIZE_WINDOW_STD"])) == \
        (IU.OUTLIER_IQR, IU.WINDOW_IQR, IU.WINDOW_STD) == (2, 3, 4)
    assert int(consts["GENIE_WINDOW_MAX"]) == IU.WINDOW_MAX and 0 < IU.LDS_BINS <= IU.WINDOW_MAX // 2


def test_insert_size_workspace_bytes(pkg):
    ws = pkg._native.lib().genie_insert_size_stats_workspace_bytes
    most = IU.WINDOW_MAX // 2
    assert ws(-2, 100) == INVALID and ws(2, 0) == INVALID and ws(2, -1) == INVALID and ws(2, most + 1) == INVALID
    up = lambda v: (v + 255) & ~255      # noqa: E731
    seen = []
    for span in (1, 20, 21, 63, 64, 1000, 4095, 4096, 10000, most):
        seen.append(ws(6, span))
        assert seen[-1] == 256 + 256 + up(12 * (span + 1)) and seen[-1] % 256 == 0, span
    assert all(a <= b for a, b in zip(seen, seen[1:]))
    assert ws(0, 500) == ws(2, 500) == ws(2**31 - 1, 500) == ws(2**40, 500)          # nothing per pair


def test_insert_size_argument_checks_before_device(pkg):
    lib = pkg._native.lib()
    ref = np.random.default_rng(1).integers(0, 4, 2000).astype(np.uint8)
    h = C.c_void_p(0)
    assert lib.genie_index_create(ref.ctypes.data_as(C.POINTER(C.c_uint8)), ref.size, 8, 0, C.byref(h)) == 0
    try:
        buf = np.zeros(1 << 20, np.uint8)
        al = (buf.ctypes.data + 255) & ~255
        p = C.c_void_p(al)
        at = lambda k: C.c_void_p(al + k)      # noqa: E731
        bytes_ok = lib.genie_insert_size_stats_workspace_bytes(4, 1000)
        assert 0 < bytes_ok <= (1 << 20) - 256

        def call(ix=h, N=4, so=p, rec=p, nrec=10, mapq=20, span=1000, least=25, stats=p, smp=p, tt=p, wsp=p, wsb=bytes_ok):
            return lib.genie_insert_size_stats(ix, N, so, rec, nrec, mapq, span, least, stats, smp, tt, wsp, wsb, None)

        assert call(ix=None) == INVALID and call(so=None) == INVALID and call(stats=None) == INVALID
        assert call(N=3) == INVALID and call(N=-2) == INVALID and call(N=1) == INVALID
        assert call(nrec=-1) == INVALID and call(wsb=-1) == INVALID
        assert call(rec=None) == INVALID
        for bad in (dict(mapq=-1), dict(mapq=61), dict(span=0), dict(span=-1), dict(span=IU.WINDOW_MAX // 2 + 1), dict(least=0),
                    dict(least=-1), dict(least=(1 << 30) + 1)):
            assert call(**bad) == INVALID, bad
        assert call(rec=at(8)) == INVALID                                # 16-byte aligned
        for name in ("so", "stats", "smp", "tt"):                        # 8-byte aligned
            assert call(**{name: at(4)}) == INVALID, name
        assert call(N=2**31) == TOO_LONG and call(nrec=2**31) == TOO_LONG
        assert call(N=2**31, wsp=None) == TOO_LONG and call(N=2**31, span=0) == INVALID and call(N=2**31 + 1) == INVALID
        assert call(wsp=None) == CAPACITY and call(wsp=at(16)) == CAPACITY
        assert call(wsb=bytes_ok - 1) == CAPACITY and call(wsb=0) == CAPACITY and call(span=1021) == CAPACITY
        assert call(mapq=61, wsp=None) == INVALID
        assert call() == NO_DEVICE
        assert call(mapq=0, span=1, least=1) == NO_DEVICE
        assert call(mapq=60, span=IU.WINDOW_MAX // 2, least=1 << 30, wsb=1 << 19) == NO_DEVICE
        assert call(smp=None) == NO_DEVICE and call(tt=None) == NO_DEVICE and call(nrec=0, rec=None) == NO_DEVICE
        assert call(N=0, wsp=None, wsb=0) == NO_DEVICE
    finally:
        lib.genie_index_destroy(h)


# ------------------------------------------------------------------ Python
def _stats(fr=None, rf=None, same=None):
    rows = np.zeros((3, 12), np.int64)
    for t, row in enumerate((fr, rf, same)):
        if row is not None:
            n, ok, lo, hi, mean = row
            rows[t] = [n, ok, mean, mean, mean, lo, hi, n, mean, 7, lo, hi]
    return rows


def test_insert_size_options(pkg):
    import torch
    opt, kind = pkg.index.insert_size_options, pkg.index.InsertSize
    assert pkg.insert_size_options is opt and pkg.InsertSize is kind
    got = opt(_stats(fr=(50, 1, 100, 900, 480), rf=(900, 1, 1500, 2500, 2000), same=(60, 1, 5, 6, 5)))
    assert isinstance(got, kind) and got[:5] == (2, 1500, 2500, 2000, True) and got.orient == pkg._native.PAIR_ORIENT["rf"]
    assert got.stats[1] == (900, 1, 2000, 2000, 2000, 1500, 2500, 900, 2000, 7, 1500, 2500) and len(got.stats) == 3
    assert opt(_stats(fr=(900, 0, 0, 0, 0), same=(60, 1, 5, 6, 5)))[:5] == (4, 5, 6, 5, True)      # the largest type is not ok
    assert opt(_stats(fr=(70, 1, 1, 2, 1), rf=(70, 1, 3, 4, 3), same=(70, 1, 5, 6, 5)))[:5] == (1, 1, 2, 1, True)      # a tie
    assert opt(_stats(rf=(70, 1, 3, 4, 3), same=(70, 1, 5, 6, 5)))[:5] == (2, 3, 4, 3, True)
    assert opt(torch.from_numpy(_stats(fr=(70, 1, 1, 2, 1))))[:5] == (1, 1, 2, 1, True)             # a CPU tensor
    none = _stats(fr=(24, 0, 0, 0, 0))
    assert opt(none)[:5] == (1, 0, 1000, 300, False) and opt(none).stats[0][0] == 24               # pair_alignments' defaults
    assert opt(none, dict(orient="rf", isize_max=4000, pen_slope=3))[:5] == (2, 0, 4000, 300, False)
    assert opt(none, dict(orient=5, isize_min=10, isize_mean=77))[:5] == (5, 10, 1000, 77, False)
    assert opt(np.zeros((3, 12), np.int64), {})[:5] == (1, 0, 1000, 300, False)


def test_python_layer(pkg):
    ref = np.random.default_rng(2).integers(0, 4, 3000).astype(np.uint8)
    ix = pkg.GenieIndex.build(ref, 8)                               # host-only: no device was touched
    assert callable(ix.insert_size_stats) and callable(pkg.SMEM.insert_size_stats)
    import inspect
    sig = inspect.signature(pkg.GenieIndex.insert_size_stats)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[3:]] == [("min_mapq", 20), ("max_span", 10000), ("min_samples", 25),
                                                                             ("samples", False)]
    assert inspect.signature(pkg.SMEM.map_pairs).parameters["insert_size"].default is None
    assert IU.DEFAULTS == (20, 10000, 25)
    with pytest.raises(Exception):
        ix.insert_size_stats(np.asarray([0, 0, 0], np.int64), np.zeros((0, 12), np.int32))
