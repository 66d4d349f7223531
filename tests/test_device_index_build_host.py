"""Device index build (genie_index_create_device), the parts that need no GPU: the new symbols, the image bound against
host-built images, and the argument checks that come before any device work."""
import ctypes as C

import numpy as np
import pytest

import golden_util as G


@pytest.fixture(scope="module")
def pkg():
    import genie_smem_amd as g
    g._native.build()
    return g


NEW = ["genie_index_device_image_bound", "genie_index_device_build_tmp_bytes", "genie_index_create_device"]


def test_new_symbols_declared_and_exported(pkg):
    import os
    hdr = open(os.path.join(G.GOLDEN, "..", "..", "include", "genie_smem.h")).read()
    lib = pkg._native.lib()
    for name in NEW:
        assert name + "(" in hdr
        assert name in pkg._native.SYMBOLS
        getattr(lib, name)


def _refs():
    rng = np.random.default_rng(7)
    out = [("n%d" % n, rng.integers(0, 4, n).astype(np.uint8)) for n in (1, 2, 5, 9, 17, 40)]
    out.append(("tandem", np.tile(np.asarray([0, 1, 1, 2, 3, 0, 2], np.uint8), 700)))
    out.append(("polyA", np.zeros(3000, np.uint8)))
    out.append(("rand100k", rng.integers(0, 4, 100_000).astype(np.uint8)))
    for ds in G.DATASETS:
        if G.have(ds):
            d, _ = G.load(ds)
            out.append((ds, np.ascontiguousarray(d["ref_codes"], np.uint8)))
    return out


@pytest.mark.parametrize("K", [0, 2, 8, 15, 16])
@pytest.mark.parametrize("table", [("auto", 0), ("wide", 0), ("compact", 0), ("auto", 9)])
def test_image_bound_covers_host_images(pkg, K, table):
    L = pkg._native.lib()
    fmt, bits = table
    tb = bits | {"auto": 0, "wide": pkg._native.TABLE_WIDE, "compact": pkg._native.TABLE_COMPACT}[fmt]
    for name, codes in _refs():
        ix = pkg.GenieIndex.build(codes, K, table_bits=bits, table_format=fmt)
        bound = L.genie_index_device_image_bound(codes.size, K, 7, tb)
        tmp = L.genie_index_device_build_tmp_bytes(codes.size, K, 7, tb)
        assert tmp > 0, name
        for flags in (0, pkg._native.IMAGE_NO_SEED_TABLE):
            assert bound >= L.genie_index_image_bytes(ix._h, flags) > 0, (name, flags)


def test_bound_rejects_what_create_rejects(pkg):
    L = pkg._native.lib()
    assert L.genie_index_device_image_bound(0, 8, 7, 0) == -1
    assert L.genie_index_device_image_bound(100, 17, 7, 0) == -1
    assert L.genie_index_device_image_bound(100, 8, 7, 7) == -1          # table_bits must exceed dir_bits
    assert L.genie_index_device_image_bound(100, 8, 7, 13) == -1
    assert L.genie_index_device_image_bound(1 << 24, 8, 7, pkg._native.TABLE_COMPACT) == -1
    assert L.genie_index_device_build_tmp_bytes(-5, 8, 7, 0) == -1


def test_create_device_checks_arguments_before_device_work(pkg):
    """Every refusal here happens on the host: the pointers are never dereferenced (fake, 256-byte aligned)."""
    L = pkg._native.lib()
    n, K = 1000, 8
    cap = L.genie_index_device_image_bound(n, K, 7, 0)
    tmp = L.genie_index_device_build_tmp_bytes(n, K, 7, 0)
    fake = C.c_void_p(1 << 20)
    nbytes = C.c_int64(0)
    h = C.c_void_p(0)

    def call(codes=fake, n=n, K=K, tb=0, flags=0, image=fake, cap=cap, out_bytes=True, tmp_p=fake, tmp_b=tmp, out=True):
        return L.genie_index_create_device(codes, n, K, 7, tb, flags, image, cap, C.byref(nbytes) if out_bytes else None,
                                           tmp_p, tmp_b, 0, None, C.byref(h) if out else None)

    E = -1
    assert call(codes=None) == E
    assert call(image=None) == E
    assert call(tmp_p=None) == E
    assert call(out_bytes=False) == E
    assert call(out=False) == E
    assert call(n=0) == E
    assert call(n=-3) == E
    assert call(K=17) == E
    assert call(K=-1) == E
    assert call(tb=7) == E
    assert call(tb=13) == E
    assert call(tb=3 << 8) == E
    assert call(flags=2) == E
    assert call(cap=cap - 1) == E
    assert call(tmp_b=tmp - 1) == E
    assert call(image=C.c_void_p((1 << 20) + 16)) == E                  # image must be 256-byte aligned
    assert not h.value
