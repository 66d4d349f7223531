"""Cost of genie_find_smems_long_ex (BWA mode) against genie_find_smems_long, which is unchanged and is the yardstick of
every line.  Per synthetic reference (100 kb, 1 Mb), 10^8 query bases drawn from it (create_query_from_ref distribution)
as 10^3 x 10^5-base and 10^4 x 10^4-base reads:
  both        GENIE_READS_BOTH_STRANDS on N reads           against  long on the explicit batch [r, rc(r), ...] of 2N reads
  split       GENIE_READS_SPLIT_BREAKS, reads without breaks  against  long on the same reads
  split_1pct / split_10pct  1 % / 10 % of the positions N     against  long on N reads with as many bases as are not N
  both_split  both flags, reads without breaks                against  long on the explicit 2N batch
Each call is timed with HIP events (torch.cuda.Event) on preallocated buffers, the cases interleaved round by round after a
warm-up of each; one JSON line with the median and the spread per case in us per call, and each ratio to its yardstick.
The explicit 2N batch is already in device memory when the clock starts: what BOTH_STRANDS saves its caller -- building
the reverse complements and uploading twice the bases -- is not in these numbers.
Usage: python tools/time_long_ex.py [--bases 100000000] [--reps 5] [--refs 100000,1000000] [--out profiles/long_ex_time.json]"""
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

BOTH, SPLIT = g._native.READS_BOTH_STRANDS, g._native.READS_SPLIT_BREAKS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--refs", default="100000,1000000")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L_ = g._native.lib()
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = {"bases": a.bases, "reps": a.reps, "unit": "us per call"}
    for n in [int(x) for x in a.refs.split(",")]:
        codes = synth.synth_ref(n, n)
        ix = g.GenieIndex.build(codes, 15).to("cuda")
        res = {}
        for L in (100_000, 10_000):
            N = max(1, a.bases // L)
            fwd = synth.reads_from_ref_device(codes, N, L, 1, device="cuda").reshape(N, L)
            inter = torch.stack([fwd, fwd.flip(1) ^ 3], 1).reshape(2 * N, L).contiguous()
            gen = torch.Generator(device="cuda").manual_seed(7)
            batches = {"fwd": fwd, "inter": inter}
            for tag, rate in (("1pct", 0.01), ("10pct", 0.1)):
                hit = torch.rand(fwd.shape, device="cuda", generator=gen) < rate
                batches["n_" + tag] = torch.where(hit, torch.full_like(fwd, 4), fwd)
                Lg = int(round(int((~hit).sum().item()) / N))      # as many bases as are not N
                batches["good_" + tag] = fwd[:, :Lg].contiguous()
            roff = {k: torch.arange(b.shape[0] + 1, device="cuda", dtype=torch.int64) * b.shape[1] for k, b in batches.items()}
            # (name, flags or None for the long call, batch, yardstick)
            cases = [("long", None, "fwd", None), ("long_2N", None, "inter", None),
                     ("both", BOTH, "fwd", "long_2N"), ("split", SPLIT, "fwd", "long"), ("both_split", BOTH | SPLIT, "fwd", "long_2N"),
                     ("long_good_1pct", None, "good_1pct", None), ("split_1pct", SPLIT, "n_1pct", "long_good_1pct"),
                     ("long_good_10pct", None, "good_10pct", None), ("split_10pct", SPLIT, "n_10pct", "long_good_10pct")]
            ws_bytes = 0
            for name, flags, key, _ in cases:
                b = batches[key]
                ws_bytes = max(ws_bytes, int(L_.genie_find_smems_long_ex_workspace_bytes(b.shape[0], b.numel(), b.shape[1], flags or 0)))
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
            cap = 2 * fwd.numel() // 3
            rows = torch.empty((cap, 4), dtype=torch.int32, device="cuda")
            off = torch.empty(2 * N + 1, dtype=torch.int64, device="cuda")
            st = torch.empty(2 * N, dtype=torch.int32, device="cuda")

            def run(flags, key):
                b = batches[key]
                if flags is None:
                    rc = L_.genie_find_smems_long(ix._h, 0, _ptr(b), _ptr(roff[key]), b.shape[0], b.numel(), b.shape[1], 1, _ptr(off),
                                                  _ptr(rows), cap, _ptr(st), _ptr(ws), ws_bytes, sp)
                else:
                    rc = L_.genie_find_smems_long_ex(ix._h, 0, flags, _ptr(b), _ptr(roff[key]), b.shape[0], b.numel(), b.shape[1], 1,
                                                     _ptr(off), _ptr(rows), cap, _ptr(st), _ptr(ws), ws_bytes, sp)
                g._native.check(rc, "genie_find_smems_long" + ("" if flags is None else "_ex"))

            rows_out, times = {}, {c[0]: [] for c in cases}
            for name, flags, key, _ in cases:                      # warm-up + row totals
                run(flags, key)
                torch.cuda.synchronize()
                strands = 2 if (flags or 0) & BOTH else 1
                rows_out[name] = int(off[strands * batches[key].shape[0]].item())
            for _ in range(a.reps):
                for name, flags, key, _y in cases:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    run(flags, key)
                    e1.record()
                    torch.cuda.synchronize()
                    times[name].append(e0.elapsed_time(e1) * 1e3)
            shape = {}
            for name, flags, key, yard in cases:
                t = np.asarray(times[name])
                shape[name] = {"median": round(float(np.median(t)), 1), "min": round(float(t.min()), 1), "max": round(float(t.max()), 1),
                               "rows": rows_out[name], "reads": int(batches[key].shape[0]), "bases": int(batches[key].numel())}
            for name, flags, key, yard in cases:
                if yard:
                    shape[name]["against"] = yard
                    shape[name]["ratio"] = round(shape[name]["median"] / shape[yard]["median"], 3)
            res[f"{N}x{L}"] = shape
            del batches, rows, ws, roff, fwd, inter
            torch.cuda.empty_cache()
        out[f"ref_{n // 1000}kb"] = res
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
