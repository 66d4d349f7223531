"""GPU: the K-mer hash table built on the device (index_build.hip, pass 6) and read back by genie_seed_lookup in LUT
mode, on the crafted references of tests/seed_table_util.py: stretches of thousands of slots over segment borders and
across slot 0, carries in the hundreds, hundreds of homes on one slot, two stretches back to back, and table sizes at
the edges of the 1024-slot carry segments.  The host builder is the specification: the device image equals the host
image byte for byte (test_seed_table_host.py pins the host table against the NumPy model), and both handles answer
every lookup like the brute force."""
import time

import numpy as np
import pytest

import seed_table_util as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import genie_smem_amd as g
    g._native.lib()
    return g


@pytest.mark.parametrize("name", U.CASES)
def test_image_and_lookups(pkg, name):
    """Image identity, then every lookup of seed_table_util.lookups on the host-built image (uploaded) and on the
    device-built one.  Binding either image runs genie_index_validate: neither may raise."""
    import torch
    cs = U.case(name)
    kmers, want, probes = U.lookups(cs)
    assert probes.max() >= cs.summary["stretch_slots"] + 1
    if name in ("mid", "wrap", "k12"):
        assert probes.max() >= 2000
    took, blobs = [], []
    for _ in range(2):                                                        # the first build of a process also loads the kernels
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        blobs.append(pkg.GenieIndex.build_on_device(cs.ref, cs.K).blob)
        torch.cuda.synchronize()
        took.append(time.perf_counter() - t0)
    print(f"{name}: n {len(cs.ref)} K {cs.K} device build {took[0]:.4f} s, again {took[1]:.4f} s, "
          f"longest probe sequence {int(probes.max())}, {cs.summary}")
    host, dev = U.same_image(pkg, cs.ref, cs.K)
    assert torch.equal(blobs[0], dev.blob) and torch.equal(blobs[1], dev.blob)       # the same bytes on every build
    host.to("cuda")
    for who, ix in (("host image", host), ("device image", dev)):
        assert ix.info()["lut_slots"] == cs.table.S and ix.info()["lut_keys"] == cs.table.m
        got = ix.seed_lookup("lut", kmers).cpu().numpy()
        bad = np.flatnonzero((got != want).any(1))
        assert not len(bad), (name, who, len(bad), [(int(i), kmers[i].tolist(), got[i].tolist(), want[i].tolist(),
                                                      int(probes[i])) for i in bad[:3]])


@pytest.mark.parametrize("name", ["mid", "wrap"])
@pytest.mark.parametrize("fmt", ["wide", "compact"])
def test_both_table_formats(pkg, name, fmt):
    cs = U.case(name)
    U.same_image(pkg, cs.ref, cs.K, table_format=fmt)


def test_without_seed_table(pkg):
    """seed_table=False: the section is the 8 empty slots, everything else equals the host image."""
    cs = U.case("wrap")
    _, dev = U.same_image(pkg, cs.ref, cs.K, seed_table=False)
    sec, slots = U.lut_section(dev.blob.cpu().numpy())
    empty = np.zeros(8, U.SLOT)
    empty["lo"] = empty["hi"] = -1
    assert slots == 8 and sec.tobytes() == empty.tobytes()
