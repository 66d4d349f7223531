"""Wide batches for the CSR calls (genie_find_smems_long / _long_ex, genie_match_stats, genie_exact_match, genie_reads_from_text,
genie_reads_from_fasta, genie_locate): batches whose windows, bases, bytes or positions leave 24, 31 or 32 bits, checked without
a CPU reference of that size.

The method: a BLOCK of reads (Nb reads, Lb bases) small enough for the brute force or the oracle, and the wide batch = c copies
of the block back to back.  Reads do not see each other, so the wide result is the block's result tiled:
  offsets[k SNb + r] = off_B[r] + k rows_B; rows, statuses, ms, lohi, counts the same in every copy; with both strands copy k
  owns the virtual positions [2 k Lb, 2 (k + 1) Lb) because a strand-read's virtual position is S times its read's offset.
The checkers below state that rule on torch tensors of any device: the host test applies them to the brute force of a tiled tiny
batch (proving the rule), the GPU tests to the device's wide output (never copied to the host).  Lb is odd, so the copies start
at every residue modulo 32 and 256: packed words and windows of different copies are not aligned alike.

Also the blocks, the shapes' sizes with the thresholds they are named for, and raw calls on device tensors whose return code
is looked at before anything is compared."""
import ctypes as C

import numpy as np

import exact_match_util as EM
import lookup_util as U
import match_stats_util as MS
import smem_util as SM

BOTH, SPLIT = MS.BOTH, MS.SPLIT
SM_MODES = {"bwa": 0, "lut": 1, "rmi": 2}

# the launch geometry of long_reads.inc that the shapes are sized against
WINDOW = 256                        # positions per window; lr_walk_kernel / lr_ms_kernel: one block of 256 threads per window
FWD_WINDOWS_PER_BLOCK = 4           # lr_fwd_kernel: blocks of 256 threads, four windows each
LAUNCH_LIMIT = 1 << 32              # HIP launches gridDim.x * blockDim.x < 2^32 threads

# shape A1: many tiny reads
A1_READS, A1_COPIES, A1_COPIES_FWD = 4099, 4100, 16400
A1_K = 3                            # the LUT key of the edge references' index: reads of 0 .. 2 bases are too short
# shape A2: dense breaks
A2_SEGMENTS, A2_COPIES = 4100, 4100
# shape B: bases past 2^31, positions past 2^32
B_BASES, B_COPIES = 1_048_613, 2050
B_REF = 100_000                     # test_long_reads_gpu._ref's synthetic reference
TEXT_COPIES = 2100
LOCATE_N, LOCATE_COPIES = 1 << 20, 2100


def windows(total, units):
    """long_layout's window count: one more than every unit can need."""
    return total // WINDOW + units + 1


def walk_threads(total, units):
    """Threads of a one-block-per-window launch over the whole batch."""
    return windows(total, units) * WINDOW


def fwd_threads(total, units):
    return -(-windows(total, units) // FWD_WINDOWS_PER_BLOCK) * 256


# ------------------------------------------------------------------ the blocks
def _odd(reads):
    assert sum(len(r) for r in reads) % 2 == 1, "a block has an odd number of bases"
    return reads


def a1_block(name):
    """A1_READS reads of 0 .. 5 bases on a reference of lookup_util.family(): every length (empty ones too), random bases and
    pieces of the reference, a few with a code 7 and, where the reference lacks a base, a few with that base."""
    ref = U.family()[name]
    rng = np.random.default_rng(len(ref) + 41)
    present = np.unique(ref)
    lacks = np.setdiff1d(np.arange(4, dtype=np.uint8), present)
    reads = []
    for i in range(A1_READS):
        L = i % 6
        if i % 3 == 0:
            s = int(rng.integers(0, len(ref) - 5))
            reads.append(ref[s:s + L].astype(np.uint8))
        else:
            reads.append(present[rng.integers(0, len(present), L)].astype(np.uint8))
    for i, at in ((5, 0), (1001, 2), (4097, 4), (2, 1), (7, 0)):
        reads[i][at] = SM.BAD_CODE
    if len(lacks):
        for i, at in ((11, 0), (2003, 3), (4091, 4), (1, 0)):
            reads[i][at] = lacks[-1]
    return _odd(reads)


def a2_block(name, segments=A2_SEGMENTS, reads=5, open_end=False):
    """`reads` reads that begin and end with a break and hold `segments` segments of 1 .. 3 bases in all, single and double
    breaks between them: a code 7, or the base the reference lacks where it lacks one, else a code 4.  open_end: the last
    read ends with its last segment instead."""
    ref = U.family()[name]
    rng = np.random.default_rng(len(ref) + 43)
    present = np.unique(ref)
    lacks = np.setdiff1d(np.arange(4, dtype=np.uint8), present)
    breaks = [SM.BAD_CODE, int(lacks[-1]) if len(lacks) else 4]
    out = []
    for r in range(reads):
        nseg = segments // reads + (1 if r < segments % reads else 0)
        parts = [np.asarray([breaks[r & 1]], np.uint8)]
        for s in range(nseg):
            parts.append(present[rng.integers(0, len(present), int(rng.integers(1, 4)))].astype(np.uint8))
            if not (open_end and r == reads - 1 and s == nseg - 1):
                parts.append(np.asarray([breaks[int(b)] for b in rng.integers(0, 2, 1 + (s % 5 == 0))], np.uint8))
        out.append(np.concatenate(parts))
    if sum(len(r) for r in out) % 2 == 0:                          # one more break in front of the first read
        out[0] = np.concatenate([[breaks[0]], out[0]]).astype(np.uint8)
    return _odd(out)


def forward_segments(ref, reads):
    """Segments of the forward strand under SPLIT_BREAKS: maximal runs of bases that the reference holds."""
    n = 0
    for r in reads:
        good = np.isin(r, np.unique(ref)).astype(np.int8)
        n += int((np.diff(np.concatenate([[0], good])) == 1).sum())
    return n


def b_block(codes):
    """The large block on the 100 000-base synthetic reference: B_BASES bases exactly.  3000 reads of 150 bases (verbatim cuts,
    cuts with one substitution, and pieces of 1 .. 30 bases stitched together), a dozen stitched reads of 1 000 .. 20 000
    bases, one mosaic of verbatim pieces of 300 000 bases, one read with a code 4, and a last stitched read that fills up."""
    from genie_smem_amd import synth
    import test_long_reads_gpu as LR
    rng = np.random.default_rng(77)
    n = len(codes)
    reads = []
    stitched = synth.reads_from_ref_fast(codes, 1000, 150, 78)
    for i in range(3000):
        if i % 3 == 2:
            reads.append(stitched[i // 3].copy())
            continue
        s = int(rng.integers(0, n - 150))
        r = codes[s:s + 150].astype(np.uint8)
        if i % 3 == 1:
            at = int(rng.integers(0, 150))
            r[at] = (r[at] + 1 + int(rng.integers(0, 3))) & 3
        reads.append(r)
    for i, L in enumerate([1000, 20000] + [int(x) for x in rng.integers(1000, 20001, 10)]):
        reads.append(LR._from_ref(codes, L, 200 + i))
    reads.append(LR._mosaic(codes, 300_000, 79, lo=300, hi=2500))
    bad = LR._from_ref(codes, 777, 80)
    bad[333] = 4
    reads.append(bad)
    rest = B_BASES - sum(len(r) for r in reads)
    assert rest > 1000
    reads.append(LR._from_ref(codes, rest, 81))
    assert sum(len(r) for r in reads) == B_BASES
    return _odd(reads)


def lines_block():
    """A text of whole lines, a little over 1 MB and of odd length: lines of 0 .. 300 symbols and one of 100 000, some ending
    in CR LF, with N and lower case among the symbols."""
    rng = np.random.default_rng(91)
    alphabet = np.frombuffer(b"ACGTACGTACGTNacgt", np.uint8)
    out, size = [], 0
    while size < (1 << 20):
        L = 100_000 if len(out) == 17 else int(rng.integers(0, 301))
        line = alphabet[rng.integers(0, len(alphabet), L)].tobytes() + (b"\r\n" if len(out) % 7 == 3 else b"\n")
        out.append(line)
        size += len(line)
    if size % 2 == 0:
        out.append(b"\n")
    text = b"".join(out)
    assert len(text) % 2 == 1 and text.endswith(b"\n")
    return text


def fasta_block():
    """A FASTA text of whole records, a little over 1 MB and of odd length: sequences of 0 .. 5000 symbols and one of 200 000,
    wrapped at 70, some lines ending in CR LF, an empty line here and there."""
    rng = np.random.default_rng(92)
    alphabet = np.frombuffer(b"ACGTACGTACGTNacgt", np.uint8)
    out, size, rec = [], 0, 0
    while size < (1 << 20):
        L = 200_000 if rec == 5 else (0 if rec % 50 == 7 else int(rng.integers(1, 5001)))
        seq = alphabet[rng.integers(0, len(alphabet), L)].tobytes()
        eol = b"\r\n" if rec % 9 == 4 else b"\n"
        body = b"".join(seq[i:i + 70] + eol for i in range(0, L, 70)) + (b"\n" if rec % 11 == 3 else b"")
        piece = b">r%d some words" % rec + eol + body
        out.append(piece)
        size += len(piece)
        rec += 1
    if size % 2 == 0:
        out.append(b"\n")
    text = b"".join(out)
    assert len(text) % 2 == 1 and text.endswith(b"\n") and text.startswith(b">")
    return text


# ------------------------------------------------------------------ the brute force of a block (tiny blocks only)
def brute_smems(ref, reads, mode, flags, K=A1_K):
    """(offsets [S N + 1], rows [R, 4], status [S N]) of genie_find_smems_long_ex by smem_util's brute force."""
    sreads = MS.strand_reads(reads, 2 if flags & BOTH else 1)
    return SM.expected_batch(ref, sreads, mode, 1, K, split=bool(flags & SPLIT))


def brute_match_stats(ref, reads, flags):
    """(ms, lohi, status) of genie_match_stats by match_stats_util's brute force."""
    return MS.expected(ref, reads, flags)


def brute_exact(ref, reads, flags):
    """(lohi, counts, status) of genie_exact_match by exact_match_util's brute force."""
    return EM.expected(ref, reads, flags)


def csr(reads):
    return SM.csr(reads)


def tile_csr(bases, off, c):
    """The CSR batch of c copies, on tensors or arrays of any device: (bases tiled, offsets shifted by the block's bases)."""
    import torch
    bases, off = torch.as_tensor(bases), torch.as_tensor(off)
    Lb = int(off[-1])
    assert int(off[0]) == 0 and Lb == bases.numel()
    shift = torch.arange(c, dtype=torch.int64, device=off.device)[:, None] * Lb
    wide_off = torch.cat([(off[:-1][None, :] + shift).reshape(-1), torch.tensor([c * Lb], dtype=torch.int64, device=off.device)])
    return bases.repeat(c), wide_off


# ------------------------------------------------------------------ the tiling rule, on torch tensors of any device
def first_bad_copy(wide, block, c, budget=1 << 27):
    """None if `wide` is `block` c times back to back (along dimension 0), else the first copy that differs.  Compared in
    slabs of copies, so that the temporaries stay small."""
    import torch
    block = torch.as_tensor(block).to(wide.device)
    assert wide.dtype == block.dtype, (wide.dtype, block.dtype)
    assert tuple(wide.shape) == (c * block.shape[0],) + tuple(block.shape[1:]), (tuple(wide.shape), c, tuple(block.shape))
    if block.numel() == 0:
        return None
    w = wide.view((c,) + tuple(block.shape))
    step = max(1, budget // block.numel())
    for k in range(0, c, step):
        same = (w[k:k + step] == block).reshape(min(step, c - k), -1).all(1)
        if not bool(same.all()):
            return k + int((~same).nonzero()[0])
    return None


def assert_tiled(wide, block, c, what):
    bad = first_bad_copy(wide, block, c)
    assert bad is None, f"{what}: copy {bad} of {c} differs from the block's result"


def assert_tiled_offsets(wide_off, block_off, c, what):
    """offsets[k M + r] = off_B[r] + k off_B[M] for the M entries of every copy, and the total behind the last."""
    import torch
    block_off = torch.as_tensor(block_off).to(wide_off.device)
    assert wide_off.dtype == block_off.dtype == torch.int64
    M, step = block_off.numel() - 1, int(block_off[-1])
    assert wide_off.numel() == c * M + 1, (what, wide_off.numel(), c, M)
    assert int(wide_off[-1]) == c * step, f"{what}: the total is {int(wide_off[-1])}, not {c} x {step}"
    if M == 0:
        return
    w = wide_off[:-1].view(c, M)
    per = max(1, (1 << 25) // M)
    for k in range(0, c, per):
        shift = torch.arange(k, min(k + per, c), dtype=torch.int64, device=w.device)[:, None] * step
        same = (w[k:k + per] == block_off[:-1][None, :] + shift).all(1)
        assert bool(same.all()), f"{what}: the offsets of copy {k + int((~same).nonzero()[0])} of {c} are not the block's, shifted"


def assert_tiled_csr(wide, block, c, what):
    """wide, block: (offsets, rows, status) of an SMEM call."""
    assert_tiled_offsets(wide[0], block[0], c, what + " offsets")
    assert_tiled(wide[1], block[1], c, what + " rows")
    assert_tiled(wide[2], block[2], c, what + " status")


def assert_tiled_all(wide, block, c, what, names):
    """wide, block: tuples of per-position or per-pattern outputs (None where an output was not asked for)."""
    for w, b, name in zip(wide, block, names):
        assert (w is None) == (b is None)
        if w is not None:
            assert_tiled(w, b, c, f"{what} {name}")


def to_torch(arrays):
    import torch
    return tuple(None if a is None else torch.as_tensor(np.ascontiguousarray(a)) for a in arrays)


# ------------------------------------------------------------------ raw calls on device tensors
def ok(lib, rc, what):
    """The return code comes first: a nonzero one fails the test with both error texts, and nothing is compared."""
    if rc != 0:
        raise AssertionError(f"{what}: {lib.genie_strerror(rc).decode()} (status {rc}) [{lib.genie_last_hip_error().decode()}]")


def _p(t):
    return C.c_void_p(t.data_ptr() if t is not None and t.numel() else 0)


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _empty(n, dtype):
    import torch
    return torch.empty(max(int(n), 1), dtype=dtype, device="cuda")


def smems_bytes(lib, flags, n, total, max_len, cap_rows, ws_units=0):
    """Bytes of run_smems's workspace and outputs."""
    S = 2 if flags & BOTH else 1
    ws = lib.genie_find_smems_long_ex_workspace_bytes(max(n, ws_units), total, max_len, flags)
    assert ws >= 0
    return ws, ws + 8 * (S * n + 1) + 16 * cap_rows + 4 * S * n


def run_smems(lib, ix, mode, flags, bases, offs, max_len, cap_rows, ws_units=0, long_call=False, what="smems"):
    """genie_find_smems_long_ex (long_call: genie_find_smems_long, flags 0) on device tensors -> (offsets [S N + 1], rows
    [offsets[-1], 4], status [S N]) on the device.  cap_rows must hold every row.  ws_units: the workspace is the size
    function's for that many reads if more than N, so that it holds that many units in one pass."""
    import torch
    n, total = offs.numel() - 1, bases.numel()
    S = 2 if flags & BOTH else 1
    ws_bytes, _ = smems_bytes(lib, flags, n, total, max_len, cap_rows, ws_units)
    ws = _empty(ws_bytes, torch.uint8)
    out_off = torch.full((S * n + 1,), -7, dtype=torch.int64, device="cuda")
    rows = torch.full((max(cap_rows, 1), 4), -7, dtype=torch.int32, device="cuda")
    st = torch.full((S * n,), -7, dtype=torch.int32, device="cuda")
    if long_call:
        assert flags == 0
        rc = lib.genie_find_smems_long(ix._h, SM_MODES[mode], _p(bases), _p(offs), n, total, max_len, 1, _p(out_off), _p(rows),
                                       cap_rows, _p(st), _p(ws), ws_bytes, _stream())
    else:
        rc = lib.genie_find_smems_long_ex(ix._h, SM_MODES[mode], flags, _p(bases), _p(offs), n, total, max_len, 1, _p(out_off),
                                          _p(rows), cap_rows, _p(st), _p(ws), ws_bytes, _stream())
    torch.cuda.synchronize()
    ok(lib, rc, what)
    del ws
    produced = int(out_off[-1])
    assert 0 <= produced <= cap_rows, f"{what}: {produced} rows for a capacity of {cap_rows}"
    return out_off, rows[:produced], st



def match_stats_bytes(lib, flags, n, total, max_len, intervals=True, ws_units=0):
    S = 2 if flags & BOTH else 1
    ws = lib.genie_match_stats_workspace_bytes(max(n, ws_units), total, max_len, flags)
    assert ws >= 0
    return ws, ws + 4 * S * total + (8 * S * total if intervals else 0) + 4 * S * n


def run_match_stats(lib, ix, flags, bases, offs, max_len, intervals=True, ws_units=0, what="match_stats"):
    """genie_match_stats on device tensors -> (ms [S total], lohi [S total, 2] or None, status [S N]) on the device."""
    import torch
    n, total = offs.numel() - 1, bases.numel()
    S = 2 if flags & BOTH else 1
    ws_bytes, _ = match_stats_bytes(lib, flags, n, total, max_len, intervals, ws_units)
    ws = _empty(ws_bytes, torch.uint8)
    ms = torch.full((S * total,), -7, dtype=torch.int32, device="cuda")
    lohi = torch.full((S * total, 2), -7, dtype=torch.int32, device="cuda") if intervals else None
    st = torch.full((S * n,), -7, dtype=torch.int32, device="cuda")
    rc = lib.genie_match_stats(ix._h, flags, _p(bases), _p(offs), n, total, max_len, _p(ms), _p(lohi), _p(st), _p(ws), ws_bytes,
                               _stream())
    torch.cuda.synchronize()
    ok(lib, rc, what)
    return ms, lohi, st


def exact_bytes(lib, flags, n, total, max_len):
    S = 2 if flags & BOTH else 1
    ws = lib.genie_exact_match_workspace_bytes(n, total, max_len, flags)
    assert ws >= 0
    return ws, ws + 16 * S * n


def run_exact(lib, ix, flags, bases, offs, max_len, what="exact_match"):
    """genie_exact_match on device tensors -> (lohi [S N, 2], counts [S N], status [S N]) on the device."""
    import torch
    n, total = offs.numel() - 1, bases.numel()
    S = 2 if flags & BOTH else 1
    ws_bytes, _ = exact_bytes(lib, flags, n, total, max_len)
    ws = _empty(ws_bytes, torch.uint8)
    lohi = torch.full((S * n, 2), -7, dtype=torch.int32, device="cuda")
    counts = torch.full((S * n,), -7, dtype=torch.int32, device="cuda")
    st = torch.full((S * n,), -7, dtype=torch.int32, device="cuda")
    rc = lib.genie_exact_match(ix._h, flags, _p(bases), _p(offs), n, total, max_len, _p(lohi), _p(counts), _p(st), _p(ws), ws_bytes,
                               _stream())
    torch.cuda.synchronize()
    ok(lib, rc, what)
    return lohi, counts, st
