"""Cost of genie_find_smems_long (BWA mode) against genie_find_smems_csr.  Per synthetic reference (100 kb, 1 Mb), 10^8
query bases drawn from it (create_query_from_ref distribution) as reads of 10^4, 10^5 and 10^6 bases through the long
call; the same number of bases as 8192-base reads through genie_find_smems_csr; and 10^6 x 150-base reads through both.
Each call is timed with HIP events (torch.cuda.Event) on preallocated buffers, the cases interleaved round by round after
a warm-up of each; one JSON line with the median and the spread per case, in us per call and G query bases per second.
Usage: python tools/time_long_reads.py [--bases 100000000] [--reps 5] [--refs 100000,1000000]"""
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
    ap.add_argument("--bases", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--refs", default="100000,1000000")
    a = ap.parse_args()
    L_ = g._native.lib()
    stream = torch.cuda.current_stream()
    sp = C.c_void_p(stream.cuda_stream)
    out = {"bases": a.bases, "reps": a.reps, "unit": "us per call; rate in G query bases/s"}
    for n in [int(x) for x in a.refs.split(",")]:
        codes = synth.synth_ref(n, n)
        ix = g.GenieIndex.build(codes, 15).to("cuda")
        batches = {}
        for L in (10_000, 100_000, 1_000_000, 8192):
            N = max(1, a.bases // L)
            batches[L] = synth.reads_from_ref_device(codes, N, L, 1, device="cuda").reshape(N, L)
        batches[150] = synth.reads_from_ref_device(codes, 1_000_000, 150, 2, device="cuda").reshape(1_000_000, 150)
        total_max = max(b.numel() for b in batches.values())
        cap = total_max // 3
        rows = torch.empty((cap, 4), dtype=torch.int32, device="cuda")
        n_max = max(b.shape[0] for b in batches.values())
        off = torch.empty(n_max + 1, dtype=torch.int64, device="cuda")
        st = torch.empty(n_max, dtype=torch.int32, device="cuda")
        ws_bytes = max(max(int(L_.genie_find_smems_long_workspace_bytes(b.shape[0], b.numel(), b.shape[1])) for b in batches.values()),
                       max(int(L_.genie_find_smems_workspace_bytes(batches[L].shape[0], L)) for L in (8192, 150)))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
        roff = {L: torch.arange(b.shape[0] + 1, device="cuda", dtype=torch.int64) * L for L, b in batches.items()}

        def run(kind, L):
            b = batches[L]
            N = b.shape[0]
            if kind == "csr":
                rc = L_.genie_find_smems_csr(ix._h, 0, _ptr(b), None, N, L, L, 1, _ptr(off), _ptr(rows), cap, _ptr(st), _ptr(ws),
                                             ws_bytes, sp)
            else:
                rc = L_.genie_find_smems_long(ix._h, 0, _ptr(b), _ptr(roff[L]), N, b.numel(), L, 1, _ptr(off), _ptr(rows), cap,
                                              _ptr(st), _ptr(ws), ws_bytes, sp)
            g._native.check(rc, kind)

        cases = [("long_1e4", "long", 10_000), ("long_1e5", "long", 100_000), ("long_1e6", "long", 1_000_000),
                 ("csr_8192", "csr", 8192), ("csr_150", "csr", 150), ("long_150", "long", 150)]
        rows_out, times = {}, {c[0]: [] for c in cases}
        for name, kind, L in cases:                                # warm-up + row totals
            run(kind, L)
            torch.cuda.synchronize()
            rows_out[name] = int(off[batches[L].shape[0]].item())
        for _ in range(a.reps):
            for name, kind, L in cases:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(kind, L)
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3)
        res = {}
        for name, kind, L in cases:
            t = np.asarray(times[name])
            med = float(np.median(t))
            res[name] = {"median": round(med, 1), "min": round(float(t.min()), 1), "max": round(float(t.max()), 1),
                         "rows": rows_out[name], "bases": int(batches[L].numel()),
                         "rate": round(batches[L].numel() / med / 1e3, 2)}
        res["long_1e5_over_csr_8192_rate"] = round(res["long_1e5"]["rate"] / res["csr_8192"]["rate"], 3)
        out[f"ref_{n // 1000}kb"] = res
        del batches, rows, ws, roff
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
