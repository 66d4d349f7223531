"""GPU: the memory contract of genie_exact_match, on the guarded buffers of tests/guarded.py through the raw call of
tests/exact_match_calls.py, the way tests/test_memory_contract_gpu.py checks the other entry points:

  - d_lohi, d_counts, d_status and the workspace have exactly the declared bytes, the weakest alignment the header allows and
    4 KiB of guard on each side; every guard holds its poison afterwards, the inputs and the index image are unchanged;
  - the result does not depend on what outputs and workspace held before: the same bytes under the poisons 0x00, 0xFF, 0x5A;
  - the result is the same on a non-null stream.

Every result is also compared with the brute force (tests/exact_match_util.py).  All comparisons are exact."""
import numpy as np
import pytest

import contract_calls as CC
import exact_match_calls as EC
import exact_match_util as EM
import lookup_util as U
from guarded import POISONS, Arena

pytestmark = pytest.mark.gpu

BOTH = EM.BOTH
NAME = "noT"


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
    e.rows = U.suffix_rows(e.ref)
    e.ix = g.GenieIndex.build(e.ref, 0, dir_bits=7).to("cuda")
    fam = U.patterns(NAME, e.ref, 7, 8, 600, 9)
    bad = next(p for p in fam if len(p) == 33).copy()
    bad[16] = 200
    # lengths 0 .. 42 and the word boundaries, a bad pattern, empty ones at both ends, a number of patterns that is no
    # multiple of the block
    e.pats = [np.zeros(0, np.uint8)] + fam + [bad, np.zeros(0, np.uint8)]
    assert len(e.pats) % 256 and {0, 1, 63, 64, 65, 1000} <= {len(p) for p in e.pats}
    # the same without the patterns above 64 bases: the call then runs without its pack stage
    e.short = [p for p in e.pats if len(p) <= 64]
    assert len(e.short) % 256 and len(e.short) > 300 and max(len(p) for p in e.short) == 64
    return e


def _three(env, pats, flags, counts, status, stream=None):
    import torch
    results = []
    for poison in POISONS:
        a = Arena("cuda", poison)
        a.freeze(env.ix.blob, "index image")
        torch.cuda.synchronize()                       # the arena's fill is done before anything runs on another stream
        s = stream if stream is not None else torch.cuda.current_stream()
        with torch.cuda.stream(s):                     # the input copies go ahead of the call on its stream
            call = EC.guarded_call(env.lib, env.ix, a, s.cuda_stream, flags, pats, 77, 13, counts, status)
        torch.cuda.synchronize()
        res = call.result()
        a.check()
        a.check_frozen()
        results.append(res)
    for other in results[1:]:
        CC.same(results[0], other)
    return results[0]


@pytest.mark.parametrize("which", ["all", "short"])
@pytest.mark.parametrize("flags", [0, BOTH])
def test_memory_contract(env, flags, which):
    pats = env.pats if which == "all" else env.short
    want = EM.expected(env.ref, pats, flags, env.rows)
    assert (want[2] == EM.READ_BAD_BASE).sum() == (2 if flags else 1) and (want[1] > 32).any() and (want[1] == 0).any()
    for counts, status in ((True, True), (False, True), (True, False), (False, False)):
        res = _three(env, pats, flags, counts, status)
        assert set(res) == {"lohi"} | ({"counts"} if counts else set()) | ({"status"} if status else set())
        assert np.array_equal(res["lohi"], want[0])
        assert not counts or np.array_equal(res["counts"], want[1])
        assert not status or np.array_equal(res["status"], want[2])


@pytest.mark.parametrize("which", ["all", "short"])
@pytest.mark.parametrize("flags", [0, BOTH])
def test_non_null_stream(env, flags, which):
    import torch
    pats = env.pats if which == "all" else env.short
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    res = _three(env, pats, flags, True, True, stream)
    for got, want in zip((res["lohi"], res["counts"], res["status"]), EM.expected(env.ref, pats, flags, env.rows)):
        assert np.array_equal(got, want)
