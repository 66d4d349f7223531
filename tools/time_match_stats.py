"""Cost of genie_match_stats (matching statistics of every read position) against its yardstick,
genie_find_smems_long on the same batch and the same handle, in the same run.  Reads drawn from the 100 kb synthetic
reference of BASELINE config 1 (create_query_from_ref distribution):
  ms_1Mx150     10^6 x 150-base reads
  ms_1kx100k    10^3 x 10^5-base reads
Per batch, three calls on preallocated buffers, each with its synchronisation(s) included, timed with HIP events
(torch.cuda.Event) after warm-up runs and interleaved round by round:
  lengths     genie_match_stats with d_lohi = NULL
  intervals   genie_match_stats with d_lohi
  long        genie_find_smems_long (BWA mode, min_len 1, room for every row)
The median and the spread (min, max) of --reps repeats in us, ns per base, and the ratio of each form's median to the long
call's; `yardstick_spread_us` (max - min of the long call's repeats) is the margin to read the lengths-only ratio by.  The
outputs are checked against each other once: every row (s, e, lo, hi) of the long call has ms[s] = e - s and lohi[s] = (lo,
hi).
One JSON line.
Usage: python tools/time_match_stats.py [--reps 20] [--scale 1.0] [--out profiles/match_stats_time.json]"""
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


def stats(t, digits=1):
    t = np.asarray(t)
    return {"median": round(float(np.median(t)), digits), "min": round(float(t.min()), digits), "max": round(float(t.max()), digits)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the batch sizes (a quick look)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L_ = g._native.lib()
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    codes = synth.synth_ref(100_000, 100_000)
    ix = g.GenieIndex.build(codes, 15).to("cuda")
    batches = [("ms_1Mx150", max(1, int(1_000_000 * a.scale)), 150, 1), ("ms_1kx100k", max(1, int(1_000 * a.scale)), 100_000, 2)]
    out = {"reps": a.reps, "scale": a.scale, "device": torch.cuda.get_device_name(0), "reference_bases": int(codes.size), "units": "us"}
    for name, n, L, seed in batches:
        total = n * L
        bases = torch.from_numpy(synth.reads_from_ref_fast(codes, n, L, seed).reshape(-1)).cuda()
        offs = torch.arange(n + 1, dtype=torch.int64, device="cuda") * L
        ms = torch.empty(total, dtype=torch.int32, device="cuda")
        lohi = torch.empty((total, 2), dtype=torch.int32, device="cuda")
        st = torch.empty(n, dtype=torch.int32, device="cuda")
        ws_ms = torch.empty(int(L_.genie_match_stats_workspace_bytes(n, total, L, 0)), dtype=torch.uint8, device="cuda")
        ws_long = torch.empty(int(L_.genie_find_smems_long_workspace_bytes(n, total, L)), dtype=torch.uint8, device="cuda")
        row_off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        rows = torch.empty((1, 4), dtype=torch.int32, device="cuda")

        def match_stats(with_lohi):
            rc = L_.genie_match_stats(ix._h, 0, _ptr(bases), _ptr(offs), n, total, L, _ptr(ms), _ptr(lohi if with_lohi else None),
                                      _ptr(st), _ptr(ws_ms), ws_ms.numel(), sp)
            g._native.check(rc, "genie_match_stats")

        def long_call():
            rc = L_.genie_find_smems_long(ix._h, g._native.MODE_BWA, _ptr(bases), _ptr(offs), n, total, L, 1, _ptr(row_off), _ptr(rows),
                                          rows.shape[0], _ptr(st), _ptr(ws_long), ws_long.numel(), sp)
            g._native.check(rc, "genie_find_smems_long")

        long_call()                                                  # learns the row total
        torch.cuda.synchronize()
        n_rows = int(row_off[-1].item())
        rows = torch.empty((n_rows, 4), dtype=torch.int32, device="cuda")
        fns = (("lengths", lambda: match_stats(False)), ("intervals", lambda: match_stats(True)), ("long", long_call))
        for _, fn in fns + fns:                                      # warm-up
            fn()
        torch.cuda.synchronize()
        at = torch.repeat_interleave(offs[:-1], row_off[1:] - row_off[:-1]) + rows[:, 0]
        assert torch.equal(ms[at], rows[:, 1] - rows[:, 0]) and torch.equal(lohi[at], rows[:, 2:]) and not bool(st.any())
        del at
        times = {k: [] for k, _ in fns}
        for _ in range(a.reps):
            for key, fn in fns:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                times[key].append(e0.elapsed_time(e1) * 1e3)
        res = {"reads": n, "read_len": L, "smem_rows": n_rows, "workspace_bytes": {"match_stats": ws_ms.numel(), "long": ws_long.numel()}}
        for key, _ in fns:
            res[key] = stats(times[key])
            res[key]["ns_per_base"] = round(res[key]["median"] * 1e3 / total, 4)
        for key in ("lengths", "intervals"):
            res[key]["ratio_to_long"] = round(res[key]["median"] / res["long"]["median"], 3)
        res["yardstick_spread_us"] = round(res["long"]["max"] - res["long"]["min"], 1)
        out[name] = res
        print(f"# {name}: {json.dumps(res)}", file=sys.stderr, flush=True)
        del bases, offs, ms, lohi, st, ws_ms, ws_long, row_off, rows
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
