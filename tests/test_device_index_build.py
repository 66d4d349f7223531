"""Index image built on the device (GenieIndex.build_on_device / genie_index_create_device) against the host builder,
which stays the specification: the two images must agree byte for byte, and the device-built handle must answer
queries like the host-built one."""
import numpy as np
import pytest

import golden_util as G

pytestmark = pytest.mark.gpu

SECTIONS = ["sa", "ref", "dir", "lut", "rmi", "dir2", "rmi_err", "mtab", "ov"]


@pytest.fixture(scope="module")
def pkg():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import genie_smem_amd as g
    g._native.lib()
    return g


def _where(img, off):
    """Name of the image section holding byte `off` (for a readable failure)."""
    hdr = img[:512].view(np.int64)
    # BlobHeader: off_sa .. off_rmi are int64 words 6..10, off_dir2 18, off_rmi_err 22, off_mtab 24, off_ov 26
    offs = {"sa": hdr[6], "ref": hdr[7], "dir": hdr[8], "lut": hdr[9], "rmi": hdr[10]}
    best = "header"
    for name, o in offs.items():
        if off >= o:
            best = name
    return best


def _same(pkg, codes, K, table_bits=0, table_format="auto", seed_table=True):
    host = pkg.GenieIndex.build(codes, K, table_bits=table_bits, table_format=table_format)
    want = host.serialize(seed_table).numpy()
    dev = pkg.GenieIndex.build_on_device(codes, K, table_bits=table_bits, table_format=table_format, seed_table=seed_table)
    got = dev.blob.cpu().numpy()
    tag = (codes.size, K, table_bits, table_format, seed_table)
    assert got.size == want.size, tag
    if not np.array_equal(got, want):
        off = int(np.flatnonzero(got != want)[0])
        raise AssertionError(f"{tag}: first difference at byte {off} ({_where(want, off)} section)")
    return host, dev


FORMATS = ["auto", "wide", "compact"]


@pytest.mark.parametrize("ds", [d for d in G.DATASETS if G.have(d)])
def test_golden_datasets_byte_identical(pkg, ds):
    d, _ = G.load(ds)
    codes = np.ascontiguousarray(d["ref_codes"], np.uint8)
    for K in sorted({0, 2, 8, 15, 16, int(d["K"])}):
        for fmt in FORMATS:
            for seed in (True, False):
                _same(pkg, codes, K, table_format=fmt, seed_table=seed)
    _same(pkg, codes, int(d["K"]), table_bits=10)
    _same(pkg, codes, int(d["K"]), table_bits=12, table_format="wide")


def test_tiny_references_byte_identical(pkg):
    """n = 1 .. 40: shorter than P, P2 and K, every tail case of the directory and the tables."""
    rng = np.random.default_rng(11)
    for n in range(1, 41):
        for codes in (rng.integers(0, 4, n).astype(np.uint8), np.zeros(n, np.uint8), np.full(n, 3, np.uint8)):
            for K in (0, 2, 8, 16):
                for fmt in FORMATS:
                    _same(pkg, codes, K, table_format=fmt, seed_table=(n % 2 == 0))
            _same(pkg, codes, 8, table_bits=9)


def test_repeats_byte_identical(pkg):
    """Tandem repeats and low complexity: chains, overflow blocks, 'rows decide' entries, long prefix doubling."""
    rng = np.random.default_rng(12)
    refs = [np.tile(np.asarray([0, 1, 1, 2, 3, 0, 2], np.uint8), 3000),
            np.zeros(5000, np.uint8),
            np.tile(rng.integers(0, 4, 37).astype(np.uint8), 400),
            np.concatenate([rng.integers(0, 4, 2000), np.tile([0, 1], 900), rng.integers(0, 4, 9000)]).astype(np.uint8)]
    # a reference where P2-mers occur 7 .. 29 times without being cut short: some copies of a few segments
    seg = [rng.integers(0, 4, 40).astype(np.uint8) for _ in range(30)]
    parts = []
    for i, s in enumerate(seg):
        for _ in range(1 + i):
            parts += [s, rng.integers(0, 4, 25).astype(np.uint8)]
    refs.append(np.concatenate(parts))
    for codes in refs:
        for K in (0, 8, 15):
            for fmt in FORMATS:
                for seed in (True, False):
                    _same(pkg, codes, K, table_format=fmt, seed_table=seed)
        _same(pkg, codes, 8, table_bits=9, table_format="compact")


@pytest.mark.parametrize("n", [100_000, 1_000_000])
def test_synthetic_byte_identical(pkg, n):
    from genie_smem_amd import synth as B
    ref = B.synth_ref(n, n)
    for K in (0, 2, 8, 15, 16):
        _same(pkg, ref, K)
    for fmt in ("wide", "compact"):
        _same(pkg, ref, 15, table_format=fmt, seed_table=False)
    _same(pkg, ref, 15, table_bits=12)


def _check_queries(pkg, host_ix, dev_ix, ref, n_reads=2000):
    import torch
    from genie_smem_amd import synth as B
    host_ix.to("cuda")
    rd = B.reads_from_ref(ref, n_reads, 150, 2501)
    for algo in ("bwa", "lut"):
        a = host_ix.find_smems(algo, rd)
        b = dev_ix.find_smems(algo, rd)
        for x, y in zip(a, b):
            assert torch.equal(x, y), algo
    rng = np.random.default_rng(25)
    pats = np.zeros((1000, 60), np.uint8)
    lens = rng.integers(1, 61, 1000).astype(np.int32)
    for i in range(1000):
        p0 = int(rng.integers(0, ref.size - 60))
        pats[i, :lens[i]] = ref[p0:p0 + lens[i]]
        if i % 3 == 0:
            pats[i, lens[i] - 1] = (pats[i, lens[i] - 1] + 1) % 4
    assert torch.equal(host_ix.sa_interval(pats, lens), dev_ix.sa_interval(pats, lens))


@pytest.mark.parametrize("n", [2_500_000, 17_000_000])
def test_megabase_references_answer_like_the_host_index(pkg, n):
    """2.5 Mb (compact table) and 17 Mb (past 2^24 bases: the wide table): byte identity, then find_smems in BWA and
    LUT modes and sa_interval on the device-built handle against the host-built one."""
    from genie_smem_amd import synth as B
    ref = B.synth_ref(n, n)
    host, dev = _same(pkg, ref, 15)
    assert dev.info()["has_host"] == 0 and dev.info()["has_device"] == 1
    _check_queries(pkg, host, dev, ref)


def test_errors_and_device_only_handle(pkg):
    import torch
    rng = np.random.default_rng(3)
    codes = rng.integers(0, 4, 5000).astype(np.uint8)
    bad = codes.copy()
    bad[1234] = 4
    with pytest.raises(pkg._native.GenieError) as e:
        pkg.GenieIndex.build_on_device(bad, 8)
    assert e.value.status == -2                                            # GENIE_E_ALPHABET
    ix = pkg.GenieIndex.build_on_device(codes, 8)
    with pytest.raises(pkg._native.GenieError) as e:
        ix.find_smems("rmi", np.zeros((4, 50), np.uint8))
    assert e.value.status == -7                                            # GENIE_E_NO_MODEL
    with pytest.raises(pkg._native.GenieError) as e:
        ix.seed_lookup("rmi", np.zeros((4, 8), np.uint8))
    assert e.value.status == -7
    with pytest.raises(RuntimeError):
        ix.suffix_array()
    with pytest.raises(pkg._native.GenieError):
        ix.train_rmi([100])
    # a device tensor goes in without a host round trip and gives the same image
    again = pkg.GenieIndex.build_on_device(torch.as_tensor(codes).cuda(), 8)
    assert torch.equal(again.blob, ix.blob)


def test_broadcast_hand_off(pkg):
    """broadcast_image at world size 1 (RCCL), then from_image on the device-built blob answers like the host index."""
    import socket
    import torch
    import torch.distributed as dist
    from genie_smem_amd import parallel, synth as B
    if dist.is_initialized():
        pytest.skip("process group already initialised")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    try:
        ref = B.synth_ref(100_000, 100_000)
        dev = pkg.GenieIndex.build_on_device(ref, 15, device="cuda:0")
        buf = parallel.broadcast_image(dev.blob, src=0, device="cuda:0")
        got = pkg.GenieIndex.from_image(buf)
        host = pkg.GenieIndex.build(ref, 15).to("cuda:0")
        rd = B.reads_from_ref(ref, 500, 100, 9)
        for algo in ("bwa", "lut"):
            for x, y in zip(host.find_smems(algo, rd), got.find_smems(algo, rd)):
                assert torch.equal(x, y), algo
    finally:
        dist.destroy_process_group()
