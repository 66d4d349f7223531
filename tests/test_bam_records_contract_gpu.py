"""GPU: the memory contract of genie_bam_records, on the guarded buffers of tests/guarded.py through the raw call of
tests/bam_util.py, the way tests/test_sam_text_contract_gpu.py checks genie_sam_text:

  - d_record_offsets, d_data, d_totals and the workspace have exactly the declared bytes, the weakest alignment the header
    allows and 4 KiB of guard on each side; every guard holds its poison afterwards, the fourteen inputs and the index image are
    unchanged; record offsets past n and data bytes at or past min(cap_data, total) are not written;
  - the result does not depend on what outputs and workspace held before: the same bytes under the poisons 0x00, 0xFF, 0x5A;
  - records, pairing rows, info rows and ops that break the call's assumptions (in-range garbage: the kernels clamp record,
    contig and reference indices and end every store below the record's end) change no byte outside the outputs, and the call
    returns; offsets that decrease give GENIE_E_INVALID.  These are runs on valid allocations; none is meant to fault.

Every well-formed result is also compared with the brute force.  All comparisons are exact."""
import numpy as np
import pytest

import bam_util as BU
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
    rng = np.random.default_rng(197)
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
            call = BU.guarded_call(env.lib, env.ix, a, stream.cuda_stream, b, **kw)
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
    total = int(BU.host_bam_records(b, env.T, ALL)["totals"][1])
    T = b["records"].shape[0]
    for kw in (dict(tags=ALL, cap_data=total), dict(tags=ALL, cap_data=total, totals=False), dict(tags=ALL, fill=False),
               dict(tags=ALL, cap_data=total // 2 + 1), dict(tags=ALL, cap_data=1), dict(tags=ST.MD, flags=ST.NO_SEQ, cap_data=total),
               dict(tags=ALL, cap_data=total, n_records=T - 2), dict(tags=ALL, cap_data=total, n_records=0)):
        want = BU.host_bam_records(b, env.T, kw.get("tags", 3), kw.get("flags", 0), kw.get("n_records"))
        res = _three(env, b, **kw)
        BU.agrees(res, want, kw.get("cap_data"))
        assert ("totals" in res) == kw.get("totals", True) and ("data" in res) == kw.get("fill", True)
    for variant in (dict(b, sam=None), dict(b, quals=None), dict(b, contig_offsets=None, contig_names=[b"one"])):
        BU.agrees(_three(env, variant, tags=ALL, cap_data=total), BU.host_bam_records(variant, env.T, ALL), total)


@pytest.mark.parametrize("what", ["records", "sam", "info", "ops", "everything"])
def test_inputs_that_break_the_assumptions_stay_inside_the_outputs(env, what):
    rng = np.random.default_rng(198)
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
    total = int(BU.host_bam_records(b, env.T, ALL)["totals"][1])
    for kw in (dict(cap_data=total), dict(cap_data=total // 3), dict(cap_data=total, n_records=T - 3)):
        res = _three(env, b, tags=ALL, **kw)                         # guards, inputs and poison-independence
        # in-range garbage: the brute force clamps as the header says, so even these bytes are the same
        BU.agrees(res, BU.host_bam_records(b, env.T, ALL, 0, kw.get("n_records")), kw["cap_data"])


def test_long_deletions_stop_at_the_records_end(env):
    # an X and a D of 2^28 - 1 bases: the sizing call counts MD's letters, the filling call writes what cap_data holds and stops
    rng = np.random.default_rng(199)
    ops = [ST.op(4, ST.EQ), ST.op(2**28 - 1, ST.D), ST.op(2**28 - 1, ST.X), ST.op(6, ST.EQ)]
    b = ST.make_batch(rng, [(10, [dict(ops=ops, contig=0, offset=10)]), (10, [])], contig_offsets=TABLE)
    res = _three(env, b, tags=ST.MD, cap_data=4096)
    bare = BU.host_bam_records(b, env.T, 0)                          # the records without tags: the brute force need not write MD out
    md = 1 + 1 + (2**28 - 1) + 1 + 1 + 2 * (2**28 - 2) + 1            # 4 ^ letters, 0 letter, (0 letter) ..., 6
    first = int(bare["record_offsets"][1]) + 3 + md + 1
    assert res["record_offsets"].tolist() == [0, first, first + int(bare["record_offsets"][2] - bare["record_offsets"][1])]
    assert res["data"].size == 4096
    head = int(bare["record_offsets"][1])                            # up to the tags the record is the bare one, but for block_size
    assert bytes(res["data"][4:head]) == bytes(bare["data"][4:head]) and bytes(res["data"][:4]) == (first - 4).to_bytes(4, "little")
    assert bytes(res["data"][head:head + 5]) == b"MDZ4^"
    assert bytes(res["data"][head + 5:head + 55]).decode() == "".join("ACGT"[c] for c in env.T[13:63])


def test_decreasing_offsets_are_refused(env):
    b = env.b
    for key in ("read_offsets", "sel_offsets", "cigar_offsets"):
        off = b[key]
        for bad in (off[::-1].copy(), np.concatenate([[1], off[1:]]), -off, np.concatenate([off[:3], off[2:3] - 1, off[4:]])):
            assert not ((np.diff(bad) >= 0).all() and bad[0] == 0)
            _three(env, dict(b, **{key: bad}), tags=ALL, cap_data=100, want_rc=ST.INVALID)      # the guards and the inputs hold here too
    _three(env, dict(b, read_offsets=b["read_offsets"] * 2), tags=ALL, cap_data=100, want_rc=ST.INVALID)      # past total_bases
