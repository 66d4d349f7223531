"""Cost of genie_find_smems_both on BASELINE config 1 (100 kb synthetic reference, 10^6 x 150-base reads drawn from it,
LUT mode): (a) genie_find_smems_csr on the N reads, (b) genie_find_smems_both on the same N reads, (c) genie_find_smems_csr
on the 2N interleaved batch [r0, rc(r0), r1, rc(r1), ...] prepared beforehand in HBM.  Each call is timed with HIP events
(torch.cuda.Event) on preallocated buffers, the cases interleaved round by round after a warm-up of each; one JSON line
with the median and the spread.  --len 1000 exercises the long-read kernel.
Usage: python tools/time_both_strands.py [--reads 1000000] [--len 150] [--mode lut] [--reps 15]"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import genie_smem_amd as g  # noqa: E402
from genie_smem_amd import synth  # noqa: E402
from genie_smem_amd.index import _ptr  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--ref", type=int, default=100_000)
    ap.add_argument("--mode", default="lut")
    ap.add_argument("--reps", type=int, default=15)
    a = ap.parse_args()
    N, L, mode = a.reads, a.len, g._native.MODES[a.mode]
    L_ = g._native.lib()
    codes = synth.synth_ref(a.ref, a.ref)
    ix = g.GenieIndex.build(codes, 15).to("cuda")
    reads = synth.reads_from_ref_device(codes, N, L, 1, device="cuda")
    inter = torch.empty((2 * N, L), dtype=torch.uint8, device="cuda")       # the reverse strand already in HBM
    inter[0::2] = reads
    inter[1::2] = torch.flip(reads, dims=[1]) ^ 3                            # packing.reverse_complement, on the device
    stream = torch.cuda.current_stream()
    sp = C.c_void_p(stream.cuda_stream)
    cap = 2 * N * max(8, L // 6)
    rows = torch.empty((cap, 4), dtype=torch.int32, device="cuda")
    off = torch.empty(2 * N + 1, dtype=torch.int64, device="cuda")
    st = torch.empty(2 * N, dtype=torch.int32, device="cuda")
    ws_bytes = max(int(L_.genie_find_smems_both_workspace_bytes(N, L)), int(L_.genie_find_smems_workspace_bytes(2 * N, L)))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")

    def run(kind):
        if kind == "a_csr_n":
            rc = L_.genie_find_smems_csr(ix._h, mode, _ptr(reads), None, N, L, L, 1, _ptr(off), _ptr(rows), cap, _ptr(st),
                                         _ptr(ws), ws_bytes, sp)
        elif kind == "b_both_n":
            rc = L_.genie_find_smems_both(ix._h, mode, _ptr(reads), None, N, L, L, 1, _ptr(off), _ptr(rows), cap, _ptr(st),
                                          _ptr(ws), ws_bytes, sp)
        else:
            rc = L_.genie_find_smems_csr(ix._h, mode, _ptr(inter), None, 2 * N, L, L, 1, _ptr(off), _ptr(rows), cap, _ptr(st),
                                         _ptr(ws), ws_bytes, sp)
        g._native.check(rc, kind)

    cases = ["a_csr_n", "b_both_n", "c_csr_2n_interleaved"]
    rows_out, times = {}, {c: [] for c in cases}
    same = None
    for name in cases:                                             # warm-up + row totals
        run(name)
        torch.cuda.synchronize()
        rows_out[name] = int(off[N if name == "a_csr_n" else 2 * N].item())
        if name == "b_both_n":
            same = (off.clone(), rows[:rows_out[name]].clone())
        elif name == "c_csr_2n_interleaved":
            same = bool(torch.equal(same[0], off) and torch.equal(same[1], rows[:rows_out[name]]))
    for _ in range(a.reps):
        for name in cases:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(name)
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3)
    out = {"config": f"{a.ref // 1000} kb ref, {N} x {L} bp, {a.mode}", "reps": a.reps, "unit": "us per call"}
    for name in cases:
        t = np.asarray(times[name])
        out[name] = {"median": round(float(np.median(t)), 1), "min": round(float(t.min()), 1),
                     "max": round(float(t.max()), 1), "rows": rows_out[name]}
    out["both_equals_interleaved"] = same
    out["b_over_c"] = round(out["b_both_n"]["median"] / out["c_csr_2n_interleaved"]["median"], 4)
    out["b_over_a"] = round(out["b_both_n"]["median"] / out["a_csr_n"]["median"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
