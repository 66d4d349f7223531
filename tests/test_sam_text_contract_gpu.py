"""GPU: the memory contract of genie_sam_text, on the guarded buffers of tests/guarded.py through the raw call of
tests/sam_text_util.py, the way tests/test_pair_contract_gpu.py checks genie_pair_alignments:

  - d_line_offsets, d_text, d_totals and the workspace have exactly the declared bytes, the weakest alignment the header allows
    and 4 KiB of guard on each side; every guard holds its poison afterwards, the fourteen inputs and the index image are
    unchanged; line offsets past n_lines and text bytes at or past min(cap_text, total) are not written;
  - the result does not depend on what outputs and workspace held before: the same bytes under the poisons 0x00, 0xFF, 0x5A;
  - records, pairing rows, info rows and ops that break the call's assumptions (in-range garbage: the kernels clamp record,
    contig and reference indices and end every store below the line's end) change no byte outside the outputs, and the call
    returns; offsets that decrease give GENIE_E_INVALID.  These are runs on valid allocations; none is meant to fault.

Every well-formed result is also compared with the brute force.  All comparisons are exact."""
import numpy as np
import pytest

import contract_calls as CC
import sam_text_util as ST
from guarded import POISONS, Arena

pytestmark = pytest.mark.gpu

N_REF = 1 << 14
TABLE = np.asarray([0, 6000, 11000, N_REF], np.int64)
ALL = 31
COUNTS = [3, 2, 0, 4, 1, 1, 0, 0, 2, 5, 1, 0]


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import genie_smem_amd as g

    class Env:
        pass
    e = Env()
    e.lib = g._native.lib()
    e.T = np.random.default_rng(8).integers(0, 4, N_REF).astype(np.uint8)
    e.ix = g.GenieIndex.build(e.T, 0).to("cuda")
    rng = np.random.default_rng(97)
    e.b = ST.make_batch(rng, ST.random_reads(rng, COUNTS, TABLE, max_ops=140), contig_offsets=TABLE)
    return e


def _three(env, b, **kw):
    import torch
    results = []
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    for poison in POISONS:
        a = Arena("cuda", poison)
        a.freeze(env.ix.blob, "index image")
        torch.cuda.synchronize()                       # the arena's fill is done before anything runs on another stream
        with torch.cuda.stream(stream):                # the input copies go ahead of the call on its stream
            call = ST.guarded_call(env.lib, env.ix, a, stream.cuda_stream, b, **kw)
        torch.cuda.synchronize()
        a.check()
        a.check_frozen()
        if kw.get("want_rc"):
            assert call.rc == kw["want_rc"], call.rc
            continue
        results.append(call.result())
    for other in results[1:]:
        CC.same(results[0], other)
    return results[0] if results else None


def test_memory_contract(env):
    b = env.b
    total = int(ST.expected(b, env.T, ALL)["totals"][1])
    T = b["records"].shape[0]
    for kw in (dict(tags=ALL, cap_text=total), dict(tags=ALL, cap_text=total, totals=False), dict(tags=ALL, fill=False),
               dict(tags=ALL, cap_text=total // 2 + 1), dict(tags=ALL, cap_text=1), dict(tags=ST.MD, flags=ST.NO_SEQ, cap_text=total),
               dict(tags=ALL, cap_text=total, n_records=T - 2), dict(tags=ALL, cap_text=total, n_records=0)):
        want = ST.expected(b, env.T, kw.get("tags", 3), kw.get("flags", 0), kw.get("n_records"))
        res = _three(env, b, **kw)
        ST.agrees(res, want, kw.get("cap_text"))
        assert ("totals" in res) == kw.get("totals", True) and ("text" in res) == kw.get("fill", True)
    for variant in (dict(b, sam=None), dict(b, quals=None), dict(b, contig_offsets=None, contig_names=[b"one"])):
        ST.agrees(_three(env, variant, tags=ALL, cap_text=total), ST.expected(variant, env.T, ALL), total)


@pytest.mark.parametrize("what", ["records", "sam", "info", "ops", "everything"])
def test_inputs_that_break_the_assumptions_stay_inside_the_outputs(env, what):
    rng = np.random.default_rng(98)
    b = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in env.b.items()}
    T = b["records"].shape[0]
    wild = [-2**31, -10**6, -41, -1, 0, 1, 2, 3, 500, 10**6, 2**30, 2**31 - 1]
    if what in ("records", "everything"):
        for col in (0, 2, 3, 4, 5, 6, 9, 11):
            hit = rng.random(T) < 0.5
            b["records"][hit, col] = rng.choice(wild, int(hit.sum())).astype(np.int32)
    if what in ("sam", "everything"):
        b["sam"][:] = rng.choice(wild, (T, 4)).astype(np.int32)
    if what in ("info", "everything"):
        b["info"][:] = rng.choice(wild, (T, 8)).astype(np.int32)
    if what in ("ops", "everything"):
        # any code; lengths that stay small on X and D, whose letters the brute force below would have to write out
        n = b["cigar"].size
        code = rng.integers(0, 16, n).astype(np.uint32)
        length = np.where((code == ST.X) | (code == ST.D), rng.integers(0, 50, n), rng.choice([0, 1, 9, 10**5, 2**28 - 1], n)).astype(np.uint32)
        b["cigar"] = (length << 4) | code
    total = int(ST.expected(b, env.T, ALL)["totals"][1])
    for kw in (dict(cap_text=total), dict(cap_text=total // 3), dict(cap_text=total, n_records=T - 3)):
        res = _three(env, b, tags=ALL, **kw)                         # guards, inputs and poison-independence
        # in-range garbage: the brute force clamps as the header says, so even these bytes are the same
        ST.agrees(res, ST.expected(b, env.T, ALL, 0, kw.get("n_records")), kw["cap_text"])


def test_long_deletions_stop_at_the_lines_end(env):
    # an X and a D of 2^28 - 1 bases: the sizing call counts them, the filling call writes what cap_text holds and stops
    rng = np.random.default_rng(99)
    reads = [(10, [dict(ops=[ST.op(4, ST.EQ), ST.op(2**28 - 1, ST.D), ST.op(2**28 - 1, ST.X), ST.op(6, ST.EQ)], contig=0, offset=10)]), (10, [])]
    b = ST.make_batch(rng, reads, contig_offsets=TABLE)
    res = _three(env, b, tags=ST.MD, cap_text=4096)
    bare = ST.expected(b, env.T, 0)["line_offsets"]                  # the lines without tags: the brute force need not write MD out
    md = 1 + 1 + (2**28 - 1) + 1 + 1 + 2 * (2**28 - 2) + 1            # 4 ^ letters, 0 letter, (0 letter) ..., 6
    assert res["line_offsets"].tolist() == [0, int(bare[1]) + len("\tMD:Z:") + md, int(bare[2]) + len("\tMD:Z:") + md]
    head = bytes(res["text"][:200]).decode("latin-1")
    assert head.startswith("read0\t") and "4=268435455D268435455X6=" in head and "\tMD:Z:4^" in head and res["text"].size == 4096
    at = head.index("MD:Z:4^") + 7
    assert bytes(res["text"][at:at + 50]).decode() == "".join("ACGT"[c] for c in env.T[13:63])


def test_decreasing_offsets_are_refused(env):
    b = env.b
    for key in ("read_offsets", "sel_offsets", "cigar_offsets"):
        off = b[key]
        for bad in (off[::-1].copy(), np.concatenate([[1], off[1:]]), -off, np.concatenate([off[:3], off[2:3] - 1, off[4:]])):
            assert not ((np.diff(bad) >= 0).all() and bad[0] == 0)
            _three(env, dict(b, **{key: bad}), tags=ALL, cap_text=100, want_rc=ST.INVALID)      # the guards and the inputs hold here too
    _three(env, dict(b, read_offsets=b["read_offsets"] * 2), tags=ALL, cap_text=100, want_rc=ST.INVALID)      # past total_bases
