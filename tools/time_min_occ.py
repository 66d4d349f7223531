"""Cost of the min_occ calls against their yardsticks, on the batches of tools/time_mems.py:
  cfg1_1Mx150      10^6 x 150-base reads drawn from the 100 kb synthetic reference of BASELINE config 1
  tandem7_20kx150  2 x 10^4 x 150-base reads cut from a 3000-base tandem repeat of GATTACA
each with k = 1, 2, 11, 32, 33 and 64 (32 and 33 sit on either side of the switch from fact 5 to fact 4).
Per batch, calls on preallocated buffers, each with its synchronisation(s) included, timed with HIP events
(torch.cuda.Event) after warm-up runs and interleaved round by round in one process:
  ms              genie_match_stats with intervals                  (yardstick: the same build, the same batch)
  ms_k<k>         genie_match_stats_min_occ with intervals
  smems           genie_find_smems_long_ex, BWA mode, min_len 19    (yardstick)
  smems_k<k>      genie_find_smems_min_occ
The median and the spread (min, max) of --reps repeats in us, each call's median as a ratio to its yardstick's, the
positions shortened, the run starts per read and the share of them whose interval has fewer than k rows (fact 3 fails; from
the yardstick's ms and intervals).  With k = 1 the outputs are checked to be the yardsticks'.  --once runs every min_occ call
of the cfg1 batch a single time and nothing else: the run to put under a kernel trace.  One JSON line.
Usage: python tools/time_min_occ.py [--reps 10] [--scale 1.0] [--once] [--out profiles/min_occ_time.json]"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import genie_smem_amd as g  # noqa: E402
from genie_smem_amd import synth  # noqa: E402
from genie_smem_amd.index import _ptr  # noqa: E402
from time_mems import tandem_batch  # noqa: E402
from time_mems_contigs import timed  # noqa: E402

KS = (1, 2, 11, 32, 33, 64)
MIN_LEN = 19


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the batch sizes (a quick look)")
    ap.add_argument("--once", action="store_true", help="one run of the min_occ calls alone, for a kernel trace")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L_ = g._native.lib()
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = {"reps": a.reps, "scale": a.scale, "device": torch.cuda.get_device_name(0), "units": "us", "k": list(KS), "min_len": MIN_LEN}
    codes = synth.synth_ref(100_000, 100_000)
    n1 = max(1, int(1_000_000 * a.scale))
    n2 = max(2, int(20_000 * a.scale))
    tref, treads = tandem_batch(n2, 150, 3)
    batches = [("cfg1_1Mx150", codes, 15, synth.reads_from_ref_fast(codes, n1, 150, 1)), ("tandem7_20kx150", tref, 0, treads)]
    if a.once:
        batches = batches[:1]
    for name, ref, K, reads in batches:
        ix = g.GenieIndex.build(ref, K).to("cuda")
        n, L = reads.shape
        total = n * L
        bases = torch.from_numpy(reads.reshape(-1)).cuda()
        offs = torch.arange(n + 1, dtype=torch.int64, device="cuda") * L
        st = torch.empty(n, dtype=torch.int32, device="cuda")
        ws = torch.empty(int(max(L_.genie_match_stats_min_occ_workspace_bytes(n, total, L, 0),
                                 L_.genie_find_smems_min_occ_workspace_bytes(n, total, L, 0))), dtype=torch.uint8, device="cuda")
        row_off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        totals = torch.zeros(1, dtype=torch.int64, device="cuda")
        ms = {k: torch.empty(total, dtype=torch.int32, device="cuda") for k in ("y", "k")}
        lohi = {k: torch.empty((total, 2), dtype=torch.int32, device="cuda") for k in ("y", "k")}

        def stats_y():
            g._native.check(L_.genie_match_stats(ix._h, 0, _ptr(bases), _ptr(offs), n, total, L, _ptr(ms["y"]), _ptr(lohi["y"]), _ptr(st),
                                                 _ptr(ws), ws.numel(), sp), "genie_match_stats")

        def stats_k(k):
            g._native.check(L_.genie_match_stats_min_occ(ix._h, 0, k, _ptr(bases), _ptr(offs), n, total, L, _ptr(ms["k"]), _ptr(lohi["k"]),
                                                         _ptr(st), _ptr(totals), _ptr(ws), ws.numel(), sp), "genie_match_stats_min_occ")

        def smems_y(rows):
            g._native.check(L_.genie_find_smems_long_ex(ix._h, 0, 0, _ptr(bases), _ptr(offs), n, total, L, MIN_LEN, _ptr(row_off), _ptr(rows),
                                                        rows.shape[0], _ptr(st), _ptr(ws), ws.numel(), sp), "genie_find_smems_long_ex")

        def smems_k(k, rows):
            g._native.check(L_.genie_find_smems_min_occ(ix._h, 0, 0, _ptr(bases), _ptr(offs), n, total, L, MIN_LEN, k, _ptr(row_off),
                                                        _ptr(rows), rows.shape[0], _ptr(st), _ptr(totals), _ptr(ws), ws.numel(), sp),
                            "genie_find_smems_min_occ")

        rows = torch.empty((16 * n, 4), dtype=torch.int32, device="cuda")      # room for every row (checked below)
        rows_k = torch.empty_like(rows)
        if a.once:
            for k in KS:
                stats_k(k)
                smems_k(k, rows_k)
            torch.cuda.synchronize()
            out[name] = {"reads": n}
            continue
        res = {"reference_bases": int(ref.size), "reads": n, "read_len": L, "shortened": {}, "smem_rows": {}, "failed_run_starts": {}}
        stats_y()
        fwd = ms["y"].view(n, L) + torch.arange(L, dtype=torch.int32, device="cuda")
        start = torch.ones((n, L), dtype=torch.bool, device="cuda")
        start[:, 1:] = fwd[:, 1:] != fwd[:, :-1]
        start &= ms["y"].view(n, L) > 0
        occ = (lohi["y"][:, 1] - lohi["y"][:, 0] + 1).view(n, L)
        res["run_starts_per_read"] = round(float(start.sum().item()) / n, 2)
        for k in KS:
            res["failed_run_starts"][f"k{k}"] = round(float((start & (occ < k)).sum().item()) / max(1, int(start.sum().item())), 4)
        del fwd, start, occ
        smems_y(rows)
        res["smem_rows"]["smems"] = int(row_off[-1].item())
        assert res["smem_rows"]["smems"] <= rows.shape[0]
        for k in KS:
            stats_k(k)
            res["shortened"][f"k{k}"] = int(totals.item())
            smems_k(k, rows_k)
            res["smem_rows"][f"smems_k{k}"] = int(row_off[-1].item())
            assert res["smem_rows"][f"smems_k{k}"] <= rows_k.shape[0]
            if k == 1:
                r = res["smem_rows"]["smems"]
                assert torch.equal(ms["k"], ms["y"]) and torch.equal(lohi["k"], lohi["y"]) and torch.equal(rows_k[:r], rows[:r])
        fns = ((("ms", stats_y),) + tuple((f"ms_k{k}", lambda k=k: stats_k(k)) for k in KS) +
               (("smems", lambda: smems_y(rows)),) + tuple((f"smems_k{k}", lambda k=k: smems_k(k, rows_k)) for k in KS))
        res.update(timed(fns, a.reps))
        res["ratio_to_ms"] = {f"ms_k{k}": round(res[f"ms_k{k}"]["median"] / res["ms"]["median"], 3) for k in KS}
        res["ratio_to_smems"] = {f"smems_k{k}": round(res[f"smems_k{k}"]["median"] / res["smems"]["median"], 3) for k in KS}
        out[name] = res
        print(f"# {name}: {json.dumps(res)}", file=sys.stderr, flush=True)
        del bases, offs, st, ws, row_off, totals, ms, lohi, rows, rows_k
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
