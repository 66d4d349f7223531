"""CPU-only tests of the long-read feature (genie_find_smems_long): the symbols and the workspace function, the C ABI's
argument checks (they come before the device check, so a host-only handle reaches them), and a numpy restatement of the
parallel traversal the kernels implement -- next(i) as a range argmax, the chain from 0 by pointer jumping -- checked
against the CPU oracle's get_SMEMS rows."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def pkg():
    import genie_smem_amd as g
    g._native.build()
    return g


def test_long_symbols_exported(pkg):
    lib = pkg._native.lib()
    for name in ("genie_find_smems_long", "genie_find_smems_long_workspace_bytes"):
        assert name in pkg._native.SYMBOLS
        getattr(lib, name)
    assert lib.genie_abi_version() == 2
    assert pkg._native.MAX_READ_LEN == 8192


def test_long_workspace_bytes(pkg):
    lib = pkg._native.lib()
    assert lib.genie_find_smems_long_workspace_bytes(-1, 100, 10) < 0
    assert lib.genie_find_smems_long_workspace_bytes(1, -1, 10) < 0
    assert lib.genie_find_smems_long_workspace_bytes(1, 100, -1) < 0
    assert lib.genie_find_smems_long_workspace_bytes(1, 100, 2**31) < 0
    w = [lib.genie_find_smems_long_workspace_bytes(10, t, 2**31 - 1) for t in (0, 10**4, 10**6, 10**8)]
    assert 0 < w[0] < w[1] < w[2] < w[3]
    assert w[3] < 20 * 10**8 + 10**6                          # about 17 bytes per base


def test_long_argument_checks_before_device(pkg):
    lib = pkg._native.lib()
    ref = np.random.default_rng(1).integers(0, 4, 2000).astype(np.uint8)
    h = C.c_void_p(0)
    assert lib.genie_index_create(ref.ctypes.data_as(C.POINTER(C.c_uint8)), ref.size, 8, 0, C.byref(h)) == 0
    try:
        ws = np.zeros(1 << 16, np.uint8)
        buf = ws.ctypes.data
        al = (buf + 255) & ~255
        p = C.c_void_p(al)
        bytes_ok = lib.genie_find_smems_long_workspace_bytes(2, 100, 100)
        assert bytes_ok <= (1 << 16) - 256

        def call(ix=h, mode=0, bases=p, offs=p, n=2, total=100, max_len=100, out_off=p, rows=p, cap=10, wsp=p, wsb=bytes_ok):
            return lib.genie_find_smems_long(ix, mode, bases, offs, n, total, max_len, 1, out_off, rows, cap, None, wsp, wsb, None)

        assert call(ix=None) == -1
        assert call(n=-1) == -1
        assert call(total=-1) == -1
        assert call(max_len=-1) == -1
        assert call(max_len=2**31) == -1
        assert call(cap=-1) == -1
        assert call(out_off=None) == -1
        assert call(offs=None) == -1
        assert call(rows=None) == -1
        assert call(wsp=None) == -1
        assert call(bases=None) == -1
        assert call(mode=3) == -1
        assert call(rows=C.c_void_p(al + 4)) == -1              # rows must be 16-byte aligned
        assert call(wsp=C.c_void_p(al + 16)) == -1              # workspace 256-byte aligned
        assert call(wsb=bytes_ok - 1) == -10                    # GENIE_E_CAPACITY
        assert call() == -4                                     # GENIE_E_NO_DEVICE: every argument was fine
        assert call(n=0, offs=None, rows=None, wsp=None, total=0, bases=None) == -4
    finally:
        lib.genie_index_destroy(h)


# ------------------------------------------------------------------ the parallel traversal, restated in numpy
def _fwd(ref, sa0, read):
    """fwd[a] = a + length of the longest prefix of read[a:] that occurs in ref, from the suffix array (binary search
    for where read[a:] would sit among the sorted suffixes; the longest match is with one of the two neighbours)."""
    rb, qb = bytes(ref), bytes(read)
    sufs = [rb[s:] for s in sa0]
    L = len(qb)
    out = np.empty(L, np.int64)
    import bisect
    for a in range(L):
        q = qb[a:]
        k = bisect.bisect_left(sufs, q)
        best = 0
        for j in (k - 1, k):
            if 0 <= j < len(sufs):
                s = sufs[j]
                m = min(len(s), len(q))
                l = 0
                while l < m and s[l] == q[l]:
                    l += 1
                best = max(best, l)
        out[a] = a + best
    return out


def _next_all(fwd):
    """next(i) for every end i: the first maximum of fwd[b] - b over b in [lo(i), i], lo(i) = first b with fwd[b] > i.
    Returns (b*, next end); b* = -1 where no candidate covers i (the base occurs nowhere)."""
    L = fwd.size
    bstar = np.full(L + 1, -1, np.int64)
    nxt = np.full(L + 1, L, np.int64)
    for i in range(L):
        lo = int(np.searchsorted(fwd, i, side="right"))          # fwd is non-decreasing
        if lo > i:
            continue
        c = np.arange(lo, i + 1)
        b = int(c[np.argmax(fwd[c] - c)])                        # np.argmax: the first maximum
        bstar[i], nxt[i] = b, fwd[b]
    return bstar, nxt


def _chain(nxt, L):
    """The ends reached from 0, by pointer jumping: up[k][i] = the 2^k-th successor, dist[i] = steps to L (list ranking),
    then the t-th successor of 0 for every t < dist[0] from the binary digits of t."""
    up = [nxt.copy()]
    dist = (np.arange(L + 1) < L).astype(np.int64)
    cur = nxt.copy()
    while True:
        d2 = dist + dist[cur]
        nxt2 = cur[cur]
        done = (cur == nxt2).all() and (d2 == dist).all()
        dist, cur = d2, nxt2
        if done:
            break
        up.append(cur.copy())
    steps = int(dist[0])
    t = np.arange(steps)
    node = np.zeros(steps, np.int64)
    for k in range(len(up)):
        sel = (t >> k) & 1 == 1
        node[sel] = up[k][node[sel]]
    return node


def _restated_rows(ref, sa0, read, min_len):
    fwd = _fwd(ref, sa0, read)
    L = read.size
    if L == 0:
        return np.zeros((0, 2), np.int64), True
    bstar, nxt = _next_all(fwd)
    ends = _chain(nxt, L)
    if (bstar[ends] < 0).any():
        return None, False                                       # an absent base on the chain
    b = bstar[ends]
    e = fwd[b]
    keep = e - b >= min_len
    return np.stack([b[keep], e[keep]], 1), True


@pytest.mark.parametrize("kind", ["random", "repeats", "no_t"])
def test_parallel_traversal_restated(pkg, oracle_mod, kind):
    rng = np.random.default_rng({"random": 1, "repeats": 2, "no_t": 3}[kind])
    if kind == "random":
        ref = rng.integers(0, 4, 3000).astype(np.uint8)
    elif kind == "repeats":
        unit = rng.integers(0, 4, 37).astype(np.uint8)
        ref = np.concatenate([unit] * 40 + [rng.integers(0, 4, 500).astype(np.uint8)] + [unit[:20]] * 30)
        ref[rng.integers(0, ref.size, 40)] = rng.integers(0, 4, 40)
    else:
        ref = rng.integers(0, 3, 2500).astype(np.uint8)
    o = oracle_mod.Oracle(ref, 8)
    sa0 = o.suffix_array[1:] - 1                                  # 0-based starts, without the '$' row
    checked = 0
    for t in range(40):
        L = int(rng.integers(0, 2001)) if t > 2 else [0, 1, 2000][t]
        if t % 3 == 0:
            read = rng.integers(0, 4 if kind != "no_t" else 3, L).astype(np.uint8)
        else:                                                     # pieces of the reference, some long
            parts, have = [], 0
            while have < L:
                s = int(rng.integers(1, 400))
                p = int(rng.integers(0, ref.size - s))
                parts.append(ref[p:p + s])
                have += s
            read = np.concatenate(parts)[:L] if parts else np.zeros(0, np.uint8)
        if kind == "no_t" and t % 7 == 5 and L > 10:
            read = read.copy()
            read[L // 2] = 3                                      # a base the reference lacks
        for ml in (1, 20):
            rows, ok = _restated_rows(ref, sa0, read, ml)
            rc, want = o.find_smems("bwa", read, ml)
            if not ok:
                assert rc < 0 and kind == "no_t"
                continue
            assert rc >= 0
            assert rows.tolist() == want[:, :2].tolist(), (kind, t, L, ml)
            checked += 1
    assert checked > 40
