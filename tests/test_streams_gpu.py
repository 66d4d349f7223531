"""GPU tests of the stream promises of include/genie_smem.h (run with -m gpu on an MI355X): every launch of a call goes to
the stream it is given, and "any number of concurrent calls on distinct streams may share" an index handle.  The calls are
raw C ABI calls on guarded buffers (tests/contract_calls.py); every comparison is exact, against the same call run alone
on the default stream.  No queue-related environment variable is set: the process has the hardware queues it is given."""
import threading

import numpy as np
import pytest

import contract_calls as CC
import match_stats_util as MS
from guarded import Arena

pytestmark = pytest.mark.gpu

K = 11
POISON = 0x5A


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import genie_smem_amd as g
    from genie_smem_amd import synth

    class Env:
        pass
    e = Env()
    e.lib = g._native.lib()
    e.codes = synth.synth_ref(50_000, 50_000)
    ix = g.GenieIndex.build(e.codes, K)
    ix.train_rmi([100])
    e.ix = ix.to("cuda")
    return e


def _steps(env, L, n, seed):
    """Eight different calls on n reads of up to L bases: [(name, fn(arena, stream) -> Call, synchronises its stream)]."""
    from genie_smem_amd import synth
    lib, ix = env.lib, env.ix
    rng = np.random.default_rng(seed)
    mat = synth.reads_from_ref_fast(env.codes, n, L, seed)
    lens = rng.integers(K, L + 1, n).astype(np.int32)
    lens[0], lens[1] = L, 0
    broken = mat.copy()
    broken[rng.random(mat.shape) < 0.01] = 4
    reads = [mat[i, :lens[i]] for i in range(n)]
    cap = n * (L // 4 + 8)
    steps = [
        ("csr bwa", lambda a, s: CC.find_csr(lib, ix, a, s, "csr", "bwa", mat, lens, L, 12, cap), False),
        ("both lut", lambda a, s: CC.find_csr(lib, ix, a, s, "both", "lut", mat, None, L, 1, 2 * cap), False),
        ("split", lambda a, s: CC.find_csr(lib, ix, a, s, "split", None, broken, lens, L, 1, cap), True),
        ("long rmi", lambda a, s: CC.find_long(lib, ix, a, s, None, "rmi", reads, 1, cap, first=3), True),
        ("csr rmi", lambda a, s: CC.find_csr(lib, ix, a, s, "csr", "rmi", mat, None, L, 1, cap), False),
        ("long_ex both+split", lambda a, s: CC.find_long(lib, ix, a, s, CC.BOTH | CC.SPLIT, "bwa", [broken[i, :lens[i]] for i in range(n)],
                                                         1, 2 * cap), True),
        ("sa_interval", lambda a, s: CC.sa_interval(lib, ix, a, s, mat[:, :min(L, 60)].copy(), None, min(L, 60)), False),
    ]
    if L <= 255:
        steps.append(("packed lut", lambda a, s: CC.find_packed(lib, ix, a, s, 8, "lut", mat, lens, 1, cap, 16), False))
    else:
        steps.append(("both bwa", lambda a, s: CC.find_csr(lib, ix, a, s, "both", "bwa", mat, lens, L, 20, 2 * cap), False))
    return steps


def _broken_reads(env, L, n, seed):
    """n reads of K .. L bases cut from the reference (one of L bases, one empty), one position in a hundred a break."""
    from genie_smem_amd import synth
    rng = np.random.default_rng(seed)
    mat = synth.reads_from_ref_fast(env.codes, n, L, seed).copy()
    mat[rng.random(mat.shape) < 0.01] = 4
    lens = rng.integers(K, L + 1, n)
    lens[0], lens[1] = L, 0
    return [mat[i, :lens[i]] for i in range(n)]


def _alone(step):
    """The result of one step on the default stream, nothing else running."""
    import torch
    a = Arena("cuda", POISON)
    call = step[1](a, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    res = call.result()
    a.check()
    a.check_frozen()
    if "offsets" in res:
        assert 0 < int(res["offsets"][-1]) == len(res["rows"])          # the row capacity held everything
    return res


def test_explicit_stream(env):
    """genie_find_smems_csr, _both, _split, _long_ex, genie_locate and genie_match_stats (both strands, breaks, bases in front
    of the first read and behind the last one, so that the kernel that fills those edges runs too) on a stream of their own:
    the results of the default-stream run.  (Nothing waits for the call but a synchronisation of that stream.)"""
    import torch
    steps = [s for s in _steps(env, 150, 300, 1) + _steps(env, 1000, 24, 2) if s[0] in ("csr bwa", "both lut", "split", "long_ex both+split")]
    rows = _alone(steps[0])["rows"]
    lohi = np.ascontiguousarray(rows[:, 2:4])
    total = int((lohi[:, 1] - lohi[:, 0] + 1).sum())
    steps.append(("locate", lambda a, s: CC.locate(env.lib, env.ix, a, s, lohi, total), False))
    steps.append(("match_stats both+split", lambda a, s: MS.guarded_call(env.lib, env.ix, a, s, MS.BOTH | MS.SPLIT, _broken_reads(env, 150, 300, 3),
                                                                         lead=37, tail=5), True))
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != torch.cuda.current_stream().cuda_stream
    for step in steps:
        want = _alone(step)
        a = Arena("cuda", POISON)
        with torch.cuda.stream(stream):               # the arena's fill and the input copies go ahead of the call on its stream
            call = step[1](a, stream.cuda_stream)
        stream.synchronize()
        CC.same(call.result(), want)
        torch.cuda.synchronize()
        a.check()
        a.check_frozen()


def test_four_streams_one_thread(env):
    """Four different batches through the calls that do not synchronise (_csr, _both, _packed, genie_sa_interval), each on its
    own stream with its own buffers, all launched back to back before one synchronisation."""
    import torch
    by_name = [dict((s[0], s) for s in _steps(env, L, n, 10 + i)) for i, (L, n) in enumerate(((100, 400), (150, 300), (255, 200), (60, 500)))]
    steps = [by_name[0]["csr bwa"], by_name[1]["both lut"], by_name[2]["packed lut"], by_name[3]["sa_interval"]]
    assert not any(s[2] for s in steps)
    want = [_alone(s) for s in steps]
    streams = [torch.cuda.Stream() for _ in steps]
    for _ in range(2):                                # twice: the second round starts while nothing is cold
        arenas = [Arena("cuda", POISON) for _ in steps]
        torch.cuda.synchronize()
        calls = []
        for step, a, st in zip(steps, arenas, streams):
            with torch.cuda.stream(st):
                calls.append(step[1](a, st.cuda_stream))
        torch.cuda.synchronize()
        for call, a, w in zip(calls, arenas, want):
            CC.same(call.result(), w)
            a.check()
            a.check_frozen()


def test_four_threads_one_handle(env):
    """Four host threads share one index handle; each has its own stream and buffers and makes eight calls, one fixed pass.
    The longest reads differ from thread to thread (100, 150, 1000, 8192 bases), so the launches ask for different amounts
    of LDS, and genie_find_smems_split / _long, which synchronise their stream, are among the calls.  Every status is 0
    and every result is the serial one.  This is a smoke test of the header's promise, not a proof: a race that needs a
    rarer interleaving than eight calls per thread produce passes it."""
    import torch
    plans = [_steps(env, L, n, 20 + i) for i, (L, n) in enumerate(((100, 300), (150, 300), (1000, 24), (8192, 6)))]
    assert all(len(p) == 8 for p in plans)
    want = [[_alone(s) for s in plan] for plan in plans]
    torch.cuda.synchronize()
    device = torch.cuda.current_device()
    gate = threading.Barrier(len(plans))
    failures = [None] * len(plans)

    def work(t):
        try:
            torch.cuda.set_device(device)
            stream = torch.cuda.Stream()
            gate.wait(timeout=120)
            with torch.cuda.stream(stream):
                for i, step in enumerate(plans[t]):
                    a = Arena("cuda", POISON)
                    call = step[1](a, stream.cuda_stream)
                    stream.synchronize()
                    CC.same(call.result(), want[t][i])
                    a.check()
                    a.check_frozen()
        except BaseException as e:  # noqa: BLE001 - reported by the main thread
            failures[t] = (plans[t][i][0] if "i" in locals() else "start", e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(len(plans))]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=600)
    assert not any(th.is_alive() for th in threads)
    for t, f in enumerate(failures):
        if f is not None:
            raise AssertionError(f"thread {t}, call '{f[0]}': {f[1]!r}") from f[1]
