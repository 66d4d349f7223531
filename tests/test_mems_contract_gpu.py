"""GPU: the memory contract of genie_find_mems, on the guarded buffers of tests/guarded.py through the raw call of
tests/mems_util.py, the way tests/test_memory_contract_gpu.py checks the other entry points:

  - d_offsets, d_rows, d_status, d_totals and the workspace have exactly the declared bytes, the weakest alignment the
    header allows and 4 KiB of guard on each side; every guard holds its poison afterwards, the inputs and the index image
    are unchanged; with out_cap_rows below the total the rows past the capacity are not written;
  - the result does not depend on what outputs and workspace held before: the same bytes under the poisons 0x00, 0xFF, 0x5A;
  - the call runs on an explicit non-null stream.

Every result is also compared with the brute force (tests/mems_util.py).  All comparisons are exact."""
import numpy as np
import pytest

import contract_calls as CC
import lookup_util as U
import match_stats_util as MS
import mems_util as MM
from guarded import POISONS, Arena

pytestmark = pytest.mark.gpu

BOTH, SPLIT = MM.BOTH, MM.SPLIT
NAME = "noT"
MIN_LEN = 5                                                     # a 5-mer of three letters: a dozen occurrences


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
    e.ref = U.family()[NAME]
    e.ix = g.GenieIndex.build(e.ref, 0, dir_bits=7).to("cuda")
    e.reads = MS.break_reads(e.ref) + MS.window_reads(e.ref)
    return e


def _three(env, flags, cap, max_occ, status, totals, m=MIN_LEN):
    import torch
    results = []
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    for poison in POISONS:
        a = Arena("cuda", poison)
        a.freeze(env.ix.blob, "index image")
        torch.cuda.synchronize()                       # the arena's fill is done before anything runs on another stream
        with torch.cuda.stream(stream):                # the input copies go ahead of the call on its stream
            call = MM.guarded_call(env.lib, env.ix, a, stream.cuda_stream, flags, env.reads, m, max_occ, cap, 77, 13, status,
                                   totals)
        torch.cuda.synchronize()
        res = call.result()
        a.check()
        a.check_frozen()
        results.append(res)
    for other in results[1:]:
        CC.same(results[0], other)
    return results[0]


@pytest.mark.parametrize("flags", [0, BOTH, SPLIT, BOTH | SPLIT])
def test_memory_contract(env, flags):
    w_off, w_rows, w_st, _ = MM.expected(env.ref, env.reads, flags, MIN_LEN)
    total = w_rows.shape[0]
    assert total > 50
    for cap, status, totals in ((total, True, True), (total // 3, True, False), (total + 9, False, True)):
        res = _three(env, flags, cap, 0, status, totals)
        assert set(res) == {"offsets", "rows"} | ({"status"} if status else set()) | ({"totals"} if totals else set())
        assert np.array_equal(res["offsets"], w_off)
        assert np.array_equal(res["rows"], w_rows[:min(cap, total)])
        assert not status or np.array_equal(res["status"], w_st)
        assert not totals or res["totals"].tolist() == [total, 0]
    w_off, w_rows, w_st, w_skip = MM.expected(env.ref, env.reads, flags, MIN_LEN, 12)
    assert w_skip > 100 and 100 < w_rows.shape[0] < total
    res = _three(env, flags, w_rows.shape[0], 12, True, True)
    assert np.array_equal(res["offsets"], w_off) and np.array_equal(res["rows"], w_rows) and res["totals"].tolist() == [w_rows.shape[0], w_skip]
