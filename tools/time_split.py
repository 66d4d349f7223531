"""Cost of genie_find_smems_split on BASELINE config 1 (100 kb synthetic reference, 10^6 x 150-base reads drawn from it):
the split call against genie_find_smems_csr (BWA) on the same reads without breaks, and the split call on reads with 1 % and
10 % of their positions replaced by N (code 4).  Each call is timed with HIP events (torch.cuda.Event) on preallocated
buffers, the cases interleaved round by round after a warm-up of each; one JSON line with the median and the spread.
Usage: python tools/time_split.py [--reads 1000000] [--len 150] [--reps 15]"""
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
    ap.add_argument("--reps", type=int, default=15)
    a = ap.parse_args()
    N, L = a.reads, a.len
    L_ = g._native.lib()
    codes = synth.synth_ref(a.ref, a.ref)
    ix = g.GenieIndex.build(codes, 15).to("cuda")
    clean = torch.as_tensor(synth.reads_from_ref_fast(codes, N, L, 1)).cuda()
    gen = torch.Generator(device="cuda").manual_seed(2)
    batches = {"clean": clean}
    for rate in (0.01, 0.10):
        hit = torch.rand(clean.shape, device="cuda", generator=gen) < rate
        batches[f"n{int(rate * 100)}pct"] = torch.where(hit, torch.full_like(clean, 4), clean)
    stream = torch.cuda.current_stream()
    sp = C.c_void_p(stream.cuda_stream)
    cap = N * 40
    rows = torch.empty((cap, 4), dtype=torch.int32, device="cuda")
    off = torch.empty(N + 1, dtype=torch.int64, device="cuda")
    st = torch.empty(N, dtype=torch.int32, device="cuda")
    ws_csr = int(L_.genie_find_smems_workspace_bytes(N, L))
    ws_split = int(L_.genie_find_smems_split_workspace_bytes(N, L))
    ws = torch.empty(max(ws_csr, ws_split), dtype=torch.uint8, device="cuda")

    def run(kind, reads):
        if kind == "csr":
            rc = L_.genie_find_smems_csr(ix._h, 0, _ptr(reads), None, N, L, L, 1, _ptr(off), _ptr(rows), cap, _ptr(st),
                                         _ptr(ws), ws_csr, sp)
        else:
            rc = L_.genie_find_smems_split(ix._h, _ptr(reads), None, N, L, L, 1, _ptr(off), _ptr(rows), cap, _ptr(st),
                                           _ptr(ws), ws_split, sp)
        g._native.check(rc, kind)

    cases = [("csr_clean", "csr", "clean"), ("split_clean", "split", "clean"), ("split_n1pct", "split", "n1pct"),
             ("split_n10pct", "split", "n10pct")]
    rows_out, times = {}, {c[0]: [] for c in cases}
    for name, kind, b in cases:                                    # warm-up + row totals
        run(kind, batches[b])
        torch.cuda.synchronize()
        rows_out[name] = int(off[-1].item())
    for _ in range(a.reps):
        for name, kind, b in cases:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(kind, batches[b])
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3)
    out = {"config": f"{a.ref // 1000} kb ref, {N} x {L} bp", "reps": a.reps, "unit": "us per call"}
    for name in times:
        t = np.asarray(times[name])
        out[name] = {"median": round(float(np.median(t)), 1), "min": round(float(t.min()), 1),
                     "max": round(float(t.max()), 1), "rows": rows_out[name]}
    out["split_clean_over_csr"] = round(out["split_clean"]["median"] / out["csr_clean"]["median"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
