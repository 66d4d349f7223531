"""The specification of genie_reference_segments and genie_segment_coords restated in Python, the raw ctypes calls and the
cases the host and GPU tests share.  Nothing here comes from the library under test.

The given reference is codes[0 .. n) with a record table off (records + 1 values, off[0] = 0, non-decreasing, off[-1] = n;
None: one record).  A break is a code > 3.  A segment is a maximal run of non-break positions inside one record; the record
of position i is the last r with off[r] <= i.  cut() walks the positions once, in order."""
import ctypes as C
import re

import numpy as np

from ingest_calls import SPARE, Call

OK, INVALID, NO_DEVICE, TOO_LONG, CAPACITY = 0, -1, -4, -6, -10
POSITIONS, HITS = 0, 1
TILE = 4096                     # bytes of the given reference per block in csrc/segments.inc (on the 16-byte grid of the address)
BREAKS = (4, 5, 0x4E, 0xFF)


def cut(codes, record_offsets=None):
    """-> (bases uint8, seg_offsets int64 [S + 1], seg_record int32 [S], seg_origin int64 [S], longest segment)."""
    codes = np.asarray(codes, np.uint8)
    off = [0, len(codes)] if record_offsets is None else [int(x) for x in record_offsets]
    assert off[0] == 0 and off[-1] == len(codes) and all(a <= b for a, b in zip(off[:-1], off[1:]))
    bases, seg_offsets, seg_record, seg_origin = [], [], [], []
    r, inside, longest = 0, False, 0
    for i, code in enumerate(codes.tolist()):
        while r + 2 < len(off) and off[r + 1] <= i:
            r += 1
            inside = False                                          # a record boundary ends the segment
        if code > 3:
            inside = False
            continue
        if not inside:
            seg_offsets.append(len(bases))
            seg_record.append(r)
            seg_origin.append(i - off[r])
            inside = True
        bases.append(code)
        longest = max(longest, len(bases) - seg_offsets[-1])
    seg_offsets.append(len(bases))
    return (np.asarray(bases, np.uint8), np.asarray(seg_offsets, np.int64), np.asarray(seg_record, np.int32),
            np.asarray(seg_origin, np.int64), longest)


def coords_expected(seg_offsets, seg_record, seg_origin, pos):
    """(record, 1-based offset in the given record) of 1-based squeezed positions; (-1, -1) outside [1, n_kept]."""
    out = np.full((len(pos), 2), -1, np.int64)
    n = int(seg_offsets[-1])
    for k, p in enumerate(np.asarray(pos, np.int64).tolist()):
        if 1 <= p <= n:
            s = int(np.searchsorted(seg_offsets, p - 1, side="right")) - 1      # segments are not empty: the offsets increase
            out[k] = (seg_record[s], seg_origin[s] + p - seg_offsets[s])
    return out


def hit_coords_expected(seg_offsets, seg_record, seg_origin, hits):
    """The same for (segment, 1-based offset inside it) pairs; (-1, -1) for a segment or an offset that does not exist."""
    hits = np.asarray(hits, np.int64).reshape(-1, 2)
    out = np.full((len(hits), 2), -1, np.int64)
    for k, (s, o) in enumerate(hits.tolist()):
        if 0 <= s < len(seg_record) and 1 <= o <= seg_offsets[s + 1] - seg_offsets[s]:
            out[k] = (seg_record[s], seg_origin[s] + o)
    return out


# ------------------------------------------------------------------ the shared cases
def _random(n, seed):
    return np.random.default_rng(seed).integers(0, 4, n).astype(np.uint8)


def patterns(n, brk=4):
    """name -> codes of n bytes: the break patterns of the tile and lane edge sweep."""
    out = {}

    def add(name, at):
        c = _random(n, n + len(out))
        at = np.asarray([a for a in at if 0 <= a < n], np.int64)
        c[at] = brk
        out[name] = c

    add("none", [])
    add("all", range(n))
    add("first", [0])
    add("last", [n - 1])
    add("at4095", [TILE - 1])
    add("at4096", [TILE])
    add("both", [TILE - 1, TILE])
    add("alternating", range(1, n, 2))                              # kept, break, kept, ...: (n + 1) / 2 segments
    add("alternating1", range(0, n, 2))
    add("one_per_tile", [i for i in range(n) if i % TILE != 77 % max(n, 1)])
    add("spanning", [0, n - 1])                                     # one segment over every tile between
    return out


EDGE_SIZES = (0, 1, 15, 16, 17, TILE - 1, TILE, TILE + 1, 3 * TILE + 5)


def record_cases():
    """name -> (codes, record offsets or None)."""
    n = 3 * TILE + 5
    plain = _random(n, 1)
    holes = plain.copy()
    holes[np.random.default_rng(2).random(n) < 0.02] = 4
    out = {"touching": (plain, [0, 100, n]),
           "tile_edges": (plain, [0, TILE - 1, TILE, 2 * TILE - 1, 2 * TILE, n]),
           "tile_edges_holes": (holes, [0, TILE - 1, TILE, 2 * TILE - 1, 2 * TILE, n]),
           "empties": (holes, [0] * 4 + [5000] * 5001 + [9000, 9001] + [n] * 3),
           "every_byte": (holes[:300], list(range(301))),
           "null_table": (holes, None), "one_record": (holes, [0, n])}
    only = holes.copy()
    only[6000:6500] = 0x4E
    out["break_record"] = (only, [0, 6000, 6500, n])
    out["break_record_inside"] = (only, [0, 6100, 6400, n])
    return out


def random_case(density, seed, n=300000, records=700):
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 4, n).astype(np.uint8)
    codes[rng.random(n) < density] = rng.choice(BREAKS)
    off = np.sort(np.concatenate([[0, n], rng.integers(0, n + 1, records - 1)])).astype(np.int64)
    return codes, off


RANDOM = [(d, s) for d in (1 / 3, 1 / 50, 1 / 5000) for s in (11, 12, 13)]


# ------------------------------------------------------------------ the end-to-end case
E2E_RUNS = (1, 400, 2, 350, 37, 300, 150, 400, 260)               # the nine N runs
E2E_M = 12


def e2e_case():
    """(strings, names, text, reads): about 5900 given bases in 3 records with nine N runs, as FASTA text wrapped at 60
    columns with \\r\\n, the second record in lower case; 200 reads of 120 bases sampled from the given sequence, N -> code 4."""
    rng = np.random.default_rng(2024)
    pieces = []
    lens = rng.integers(220, 420, len(E2E_RUNS) + 3)               # at most 4096 kept bases: lookup_util's brute force
    for k, L in enumerate(lens.tolist()):
        pieces.append("".join("ACGT"[c] for c in rng.integers(0, 4, L)))
        if k < len(E2E_RUNS):
            pieces.append("N" * E2E_RUNS[k])
    given = "".join(pieces)
    cuts = [0, len(given) // 3 + 17, 2 * len(given) // 3 - 5, len(given)]
    strings = [given[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    strings[1] = strings[1].lower()
    names = ["chrA", "chrB", "chrC"]
    text = "".join(">%s some words\r\n%s" % (nm, "".join(s[i:i + 60] + "\r\n" for i in range(0, len(s), 60)))
                   for nm, s in zip(names, strings)).encode()
    reads = []
    runs = [(m.start(), m.end()) for m in re.finditer("N+", given)]
    for k in range(200):
        j, side = k // len(runs), k % len(runs)
        if j < 4:                                                   # 30, 50, 70, 90 bases in front of every N run ...
            at = runs[side][0] - (30 + 20 * j)
        elif j < 8:                                                 # ... and behind it
            at = runs[side][1] - 120 + (30 + 20 * (j - 4))
        else:
            at = int(rng.integers(0, len(given) - 120))
        at = min(max(at, 0), len(given) - 120)
        reads.append(np.asarray(["ACGTN".index(ch) for ch in given[at:at + 120].upper()], np.uint8))
    return strings, names, text, reads


# ------------------------------------------------------------------ the raw calls
def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr() if t is not None and t.numel() else 0)


CALL = Call("genie_reference_segments", [("int64", 1), ("int32", 0), ("int64", 0)], 4, null_cap=-5)


def segments_call(lib, codes, off=None, cap_bases=None, cap_segs=None, sizing=False, lead=0, fill=0xA5, want_rc=OK, spare=SPARE):
    """ingest_calls.Call.run of genie_reference_segments with the record table `off` (None: NULL, one record) -> dict of numpy
    arrays (out4; bases, seg_offsets, seg_record, seg_origin whole, spare included).  Default capacities: the true sizes."""
    import torch
    nrec = 1 if off is None else len(off) - 1
    d_off = None if off is None else torch.as_tensor(np.asarray(off, np.int64)).cuda()
    got = CALL.run(lib, codes, (_p(d_off), nrec), lambda cap: CALL.tmp_bytes(lib, np.asarray(codes).size, nrec), cap_bases, cap_segs,
                   sizing, lead, fill, spare)
    assert got[0] == want_rc, got[0]
    if sizing:
        return {"out4": got[1]}
    return {"out4": got[1], "bases": got[2], "seg_offsets": got[3][0], "seg_record": got[3][1], "seg_origin": got[3][2], "fill": fill}


def same_as_cut(got, want, spare=SPARE):
    """The outputs of a filling segments_call with the true capacities against cut()'s; everything behind them untouched."""
    bases, so, sr, sg, longest = want
    S, kept = len(sr), len(bases)
    assert got["out4"] == [S, kept, longest, 0], (got["out4"], [S, kept, longest, 0])
    assert np.array_equal(got["bases"][:kept], bases) and (got["bases"][kept:] == got["fill"]).all()
    assert np.array_equal(got["seg_offsets"][:S + 1], so) and (got["seg_offsets"][S + 1:] == -7).all()
    assert np.array_equal(got["seg_record"][:S], sr) and (got["seg_record"][S:] == -7).all()
    assert np.array_equal(got["seg_origin"][:S], sg) and (got["seg_origin"][S:] == -7).all()
    assert got["bases"].size == kept + spare


def coords_call(lib, ix, so, sr, sg, form, values, stride, count=None, fill=-7):
    """One raw genie_segment_coords -> int64 [count, 2]."""
    import torch
    values = np.asarray(values, np.int32).reshape(-1)
    if count is None:
        count = (values.size + stride - 1) // stride if form == POSITIONS else (values.size + stride - 2) // stride
    d = [torch.as_tensor(np.ascontiguousarray(x)).cuda() for x in (np.asarray(so, np.int64), np.asarray(sr, np.int32),
                                                                   np.asarray(sg, np.int64), values if values.size else np.zeros(2, np.int32))]
    out = torch.full((max(count, 1), 2), fill, dtype=torch.int64, device="cuda")
    rc_ = lib.genie_segment_coords(ix._h, _p(d[0]), _p(d[1]), _p(d[2]), len(sr), form, _p(d[3]), stride, count, _p(out), _stream())
    torch.cuda.synchronize()
    assert rc_ == 0, rc_
    return out.cpu().numpy()[:count]


def guarded_segments(lib, a, s, codes, off, nrec, cap_bases, cap_segs):
    """genie_reference_segments on the guarded buffers of tests/guarded.py: the inputs frozen, the outputs and the scratch
    cut from the arena `a` with exactly the declared bytes and the weakest alignment the header allows, on stream `s`,
    synchronised by the call itself -> (status, out4)."""
    import contract_calls as CC
    pc = CC._inp(a, "codes", np.asarray(codes, np.uint8))
    po = CC._inp(a, "record_offsets", None if off is None else np.asarray(off, np.int64), 8)
    a.alloc("bases", cap_bases, 1)
    a.alloc("seg_offsets", 8 * (cap_segs + 1), 8)
    a.alloc("seg_record", 4 * cap_segs, 4)
    a.alloc("seg_origin", 8 * cap_segs, 8)
    tb = lib.genie_reference_segments_tmp_bytes(len(codes), nrec)
    a.alloc("tmp", tb, 256)
    out4 = (C.c_int64 * 4)(-9, -9, -9, -9)
    rc_ = lib.genie_reference_segments(CC._vp(pc), len(codes), CC._vp(po), nrec, CC._vp(a.addr("bases")), cap_bases,
                                       CC._vp(a.addr("seg_offsets")), CC._vp(a.addr("seg_record")), CC._vp(a.addr("seg_origin")), cap_segs,
                                       out4, CC._vp(a.addr("tmp")), tb, CC._vp(s))
    return rc_, list(out4)
