"""GPU: every find_smems* entry point against the brute force of tests/smem_util.py (pinned on the host by
test_tuning_knobs_host.py) over the knobs that "do not change results": dir_bits (P) 1 .. 7, table_bits (P2) 2 .. 12, both
forms of the match table, K on both sides of P2, the launch options, and images built on the device.  The references are
the edge family of tests/lookup_util.py (at most 4096 bases, so a large P2 makes almost every table entry an absent
P2-mer); the reads are smem_util.batches(): every length from 1 to 17, 31, 32, 33, 64, 150 and 255 (match_table_kernel),
256, 705 and 1409 (match_table_long_kernel), 9000 (find_smems_long, in every mode too) and a ragged batch with empty reads -- random reads,
stitched reference pieces, exact substrings (the first and last bases of the reference among them), substitutions, the
reference's tail followed by random bases, one base repeated, reads that end where a run of A goes on, tandem units across
and up to the substituted base, a base the reference lacks, a code 7.  Offsets, rows and statuses are compared exactly,
for every read."""
import ctypes as C
import functools

import numpy as np
import pytest

import lookup_util as U
import smem_util as S
from test_host_index import _parse

pytestmark = pytest.mark.gpu

FAMILY = U.family()
REFS = ["rand1", "rand2", "rand5", "rand37", "tail_none", "tail_A", "tail_AAAAAAAA", "tail_TTTTTTTT", "tail_CAAAAAA",
        "tandem1", "tandem3", "tandem7", "noT", "rand4096"]
AUTO_P2 = 8                                                   # automatic table_bits at dir_bits 7 below 262144 bases
PAIRS = [(1, 2), (1, 5), (2, 3), (3, 4), (3, 6), (3, 9), (5, 6), (5, 8), (7, 8), (7, 10), (7, 11), (7, 0)]
FORMS = ["compact", "wide"]
GRID = [(P, bits, form) for P, bits in PAIRS for form in FORMS]
REDUCED = [(P, bits, form) for P, bits in [(1, 2), (3, 4), (5, 8), (7, 11)] for form in FORMS]


@pytest.fixture(scope="module")
def pkg():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import genie_smem_amd as g
    g._native.lib()
    return g


def _id(case):
    return f"P{case[0]}-bits{case[1] or 'auto'}-{case[2]}"


def key_size(name, P2, turn):
    """K from {P2 - 1, P2, P2 + 1} (by `turn`), clipped to [1, min(16, n)]: the RMI branch K >= P2 is taken both ways."""
    return max(1, min(P2 + turn % 3 - 1, 16, len(FAMILY[name])))


def _build(pkg, name, P, bits, form, K, rmi=True):
    """Host-built index on the device with a natively trained model; the header holds the knobs that were asked for."""
    ix = pkg.GenieIndex.build(FAMILY[name], K, dir_bits=P, table_bits=bits, table_format=form)
    h = _parse(ix.serialize().numpy())
    assert h["P"] == P == ix.info()["dir_bits"] and h["n"] == len(FAMILY[name]) and h["K"] == K
    assert h["P2"] == (bits or AUTO_P2) and h["P2"] > P
    assert bool(h["flags"] & 2) == (form != "wide")                                 # kFlagCompactTable
    if rmi:
        ix.train_rmi([10])
    return ix.to("cuda")


# ------------------------------------------------------------------ batches on the device, expectations on the host
_DEVICE = {}


def _groups(name, kinds=("short", "mid", "ragged")):
    """(label, reads) of the fixed-length groups and the ragged batch of one reference."""
    b = S.batches(name)
    out = []
    for kind in kinds:
        out += [(kind, b[kind])] if kind == "ragged" else [(f"{kind}{L}", r) for L, r in b[kind].items()]
    return out


def _on_device(name, label, reads):
    """(reads [N, stride] uint8 on the device, lens or None): a fixed-length group as it is, the ragged batch with junk
    behind every read and three bytes of slack."""
    import torch
    if (name, label) not in _DEVICE:
        if label == "ragged":
            mat, lens = S.matrix(reads, max(len(r) for r in reads) + 3)
            _DEVICE[name, label] = (torch.as_tensor(mat).cuda(), torch.as_tensor(lens).cuda())
        else:
            _DEVICE[name, label] = (torch.as_tensor(np.stack(reads)).cuda(), None)
    return _DEVICE[name, label]


@functools.lru_cache(maxsize=None)
def _want(name, label, mode, min_len, K):
    reads = dict(_groups(name) + [("long", _long_reads(name))])[label]
    return S.expected_batch(FAMILY[name], reads, mode, min_len, K)


def _compare(got, want, reads, tag):
    """Offsets, rows and statuses of a CSR result against the brute force, exactly; names the first read that differs."""
    off, rows, st = (x.cpu().numpy() if hasattr(x, "cpu") else x for x in got)
    woff, wrows, wst = want
    if off.tolist() == woff.tolist() and st.tolist() == wst.tolist() and rows.tolist() == wrows.tolist():
        return
    for r in range(len(wst)):
        a = (int(st[r]), rows[off[r]:off[r + 1]].tolist()) if r + 1 < len(off) else None
        b = (int(wst[r]), wrows[woff[r]:woff[r + 1]].tolist())
        assert a == b, (tag, r, np.asarray(reads[r]).tolist()[:100], "got", a, "want", b)
    raise AssertionError((tag, "shapes", off.shape, woff.shape, rows.shape, wrows.shape))


MODES = [("bwa", 1), ("bwa", 12), ("lut", 1), ("rmi", 1)]


def _check_find_smems(ix, name, K, tag, modes=MODES, kinds=("short", "mid", "ragged")):
    n_reads = 0
    for label, reads in _groups(name, kinds):
        mat, lens = _on_device(name, label, reads)
        for mode, min_len in modes:
            got = ix.find_smems(mode, mat, lens, min_len)
            _compare(got, _want(name, label, mode, min_len, K if mode != "bwa" else 0), reads, tag + (label, mode, min_len, K))
        n_reads += len(reads)
    return n_reads


def _long_reads(name):
    return S.batches(name)["long"] + S.batches(name)["long_extra"]


def _check_find_smems_long(ix, name, K, tag, modes=MODES):
    import torch
    reads = _long_reads(name)
    if (name, "long") not in _DEVICE:
        _DEVICE[name, "long"] = tuple(torch.as_tensor(a).cuda() for a in S.csr(reads))
    for mode, min_len in modes:
        got = ix.find_smems_long(mode, *_DEVICE[name, "long"], min_len)
        _compare(got, _want(name, "long", mode, min_len, K if mode != "bwa" else 0), reads, tag + ("long", mode, K))


# ------------------------------------------------------------------ the knob grid
@pytest.mark.parametrize("case", GRID, ids=_id)
def test_find_smems_over_dir_bits_and_table_bits(pkg, case):
    P, bits, form = case
    P2 = bits or AUTO_P2
    ks = set()
    for i, name in enumerate(REFS):
        K = key_size(name, P2, i + GRID.index(case))
        ks.add(np.sign(K - P2) if len(FAMILY[name]) > P2 else None)
        ix = _build(pkg, name, P, bits, form, K)
        assert _check_find_smems(ix, name, K, (_id(case), name)) > 300
        _check_find_smems_long(ix, name, K, (_id(case), name))
    assert ks >= {-1, 0, 1}                                   # K below, at and above P2


@pytest.mark.parametrize("form", FORMS)
def test_find_smems_with_the_largest_tables(pkg, form):
    """table_bits 12: 16.7 M entries, all but a few thousand of them absent P2-mers."""
    for i, name in enumerate(["tandem7", "rand37"]):
        K = key_size(name, 12, i)
        ix = _build(pkg, name, 7, 12, form, K)
        _check_find_smems(ix, name, K, ("P7-bits12", form, name))
        _check_find_smems_long(ix, name, K, ("P7-bits12", form, name))


# ------------------------------------------------------------------ the other entry points
OTHER_REFS = ["tandem3", "tail_AAAAAAAA", "rand4096"]


def _with_breaks(reads, P2):
    """Copies of the reads with breaks (code 4) at position 0, L - 1, P2 - 1, P2 and a run of three, in turn."""
    out = []
    for j, r in enumerate(reads):
        r, L = r.copy(), len(r)
        at = [[0], [L - 1], [P2 - 1], [P2], [L // 2, L // 2 + 1, L // 2 + 2]][j % 5]
        r[[a for a in at if 0 <= a < L]] = 4
        out.append(r)
    return out


@pytest.mark.parametrize("case", REDUCED, ids=_id)
def test_both_split_long_ex_and_packed_over_the_knobs(pkg, case):
    from genie_smem_amd import packing
    P, bits, form = case
    for i, name in enumerate(OTHER_REFS + ["tandem1"]):
        ref = FAMILY[name]
        K = key_size(name, bits, i)
        ix = _build(pkg, name, P, bits, form, K)
        escapes = 0
        for label, reads in _groups(name, ("short",)):
            tag = (_id(case), name, label, K)
            mat = np.stack(reads)
            ok = [r for r in reads if int(r.max()) <= 3]                         # a code 7 cannot be packed in 2 bits
            packed = packing.pack_reads(np.stack(ok))
            for mode, min_len in MODES:
                for rb in (8, 6):
                    c8, s8, r8, esc = ix.find_smems_packed(mode, packed, mat.shape[1], None, min_len, row_bytes=rb)
                    off, rows = packing.unpack_rows(c8.cpu().numpy(), r8.cpu().numpy(), esc.cpu().numpy(), row_bytes=rb)
                    _compare((off, rows, s8.cpu().numpy().astype(np.int32)), S.expected_batch(ref, ok, mode, min_len, K), ok,
                             tag + ("packed", rb, mode, min_len))
                    escapes += len(esc)
            if name == "tandem1":
                continue
            both = [x for r in reads for x in (r, packing.reverse_complement(r))]
            for mode, min_len in MODES:
                _compare(ix.find_smems_both(mode, mat, None, min_len), S.expected_batch(ref, both, mode, min_len, K), both,
                         tag + ("both", mode, min_len))
            cut = _with_breaks(reads, bits)
            for min_len in (1, 12):
                _compare(ix.find_smems_split(np.stack(cut), None, min_len), S.expected_batch(ref, cut, "bwa", min_len, split=True),
                         cut, tag + ("split", min_len))
        if name == "tandem1":
            assert escapes > 0                                # intervals of 255 rows and more: the 6-byte rows' escape list
            continue
        for label, reads in _groups(name, ("mid",)):
            cut = _with_breaks(reads, bits)
            both = [x for r in cut for x in (r, packing.reverse_complement(r))]
            for min_len in (1, 12):
                got = ix.find_smems_long("bwa", *S.csr(cut), min_len, both_strands=True, split_breaks=True)
                _compare(got, S.expected_batch(ref, both, "bwa", min_len, split=True), both, (_id(case), name, label, "long_ex", min_len))


# ------------------------------------------------------------------ launch options
def _lds(ix):
    return ix.launch_info("bwa", 150)["lds_bytes"]


@pytest.mark.parametrize("case", [(7, 0, "compact"), (3, 4, "compact")], ids=_id)
def test_launch_options_do_not_change_results(pkg, case):
    N = pkg._native
    P, bits, form = case
    settings = [{N.OPT_GROUP_POSITIONS: 1}, {N.OPT_GROUP_POSITIONS: 64}, {N.OPT_GROUP_POSITIONS: 1_000_000},
                {N.OPT_SEARCH_BLOCKS_PER_CU: 1}, {N.OPT_SEARCH_ALL: 1}, {N.OPT_GROUP_POSITIONS: 1, N.OPT_SEARCH_ALL: 1}]
    for i, name in enumerate(["tandem7", "rand4096"]):
        K = key_size(name, bits or AUTO_P2, i)
        ix = _build(pkg, name, P, bits, form, K)
        lds = {0: _lds(ix)}
        try:
            for setting in settings:
                for opt, value in setting.items():
                    ix.set_option(opt, value)
                if list(setting) == [N.OPT_GROUP_POSITIONS]:
                    lds[setting[N.OPT_GROUP_POSITIONS]] = _lds(ix)
                _check_find_smems(ix, name, K, (_id(case), name, tuple(setting.items())), kinds=("short", "mid"))
                for opt in setting:
                    ix.set_option(opt, 0)
        finally:
            for opt in (N.OPT_GROUP_POSITIONS, N.OPT_SEARCH_BLOCKS_PER_CU, N.OPT_SEARCH_ALL):
                ix.set_option(opt, 0)
        assert lds[1] != lds[1_000_000] and _lds(ix) == lds[0], lds          # the knob reached the plan, and was reset


# ------------------------------------------------------------------ images built on the device
@pytest.mark.parametrize("case", GRID, ids=_id)
def test_device_built_image_over_dir_bits_and_table_bits(pkg, case):
    import torch
    P, bits, form = case
    for i, name in enumerate(["rand37", "tail_AAAAAAAA", "tandem7", "rand4096"]):
        K = key_size(name, bits or AUTO_P2, i)
        want = pkg.GenieIndex.build(FAMILY[name], K, dir_bits=P, table_bits=bits, table_format=form).serialize().numpy()
        dev = pkg.GenieIndex.build_on_device(FAMILY[name], K, dir_bits=P, table_bits=bits, table_format=form)
        got = dev.blob.cpu().numpy()
        assert got.size == want.size, (_id(case), name)
        diff = np.flatnonzero(got != want)
        assert not len(diff), (_id(case), name, K, "first difference at byte", int(diff[0]))
        what = C.c_uint32(77)
        with torch.cuda.device(dev.device):
            rc = pkg._native.lib().genie_index_validate(dev._h, C.byref(what), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert (rc, what.value) == (0, 0), (_id(case), name)
        _check_find_smems(dev, name, K, (_id(case), name, "device-built"), modes=MODES[:3], kinds=("ragged",))
