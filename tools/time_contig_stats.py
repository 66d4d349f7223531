"""Cost of the contig-exact calls against their yardsticks, on the batches of tools/time_mems.py:
  cfg1_1Mx150      10^6 x 150-base reads drawn from the 100 kb synthetic reference of BASELINE config 1
  tandem7_20kx150  2 x 10^4 x 150-base reads cut from a 3000-base tandem repeat of GATTACA
each with the reference cut into 1, 25 and 10^4 equal contigs, and
  junction_25      10^6 x 150-base reads of the cfg1 reference in 25 contigs, every one of them across a boundary (read i
                   has 20 + i mod 111 bases in front of it): every read has a flagged run, which prices the slow kernel.
Per batch, calls on preallocated buffers, each with its synchronisation(s) included, timed with HIP events
(torch.cuda.Event) after warm-up runs and interleaved round by round in one process:
  ms              genie_match_stats with intervals             (yardstick: the same build, the same batch)
  ms_contigs_<c>  genie_match_stats_contigs with intervals
  smems           genie_find_smems_long_ex, BWA mode, min_len 19    (yardstick)
  smems_contigs_<c>  genie_find_smems_contigs
The median and the spread (min, max) of --reps repeats in us, each call's median as a ratio to its yardstick's, the clipped
positions and the run starts per read (from the yardstick's ms).  With one contig the outputs are checked to be the
yardsticks'.  --once runs every contig call of the 25-contig cfg1 and the junction batch a single time and nothing else:
the run to put under a kernel trace.  One JSON line.
Usage: python tools/time_contig_stats.py [--reps 10] [--scale 1.0] [--once] [--out profiles/contig_stats_time.json]"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import genie_smem_amd as g  # noqa: E402
from genie_smem_amd import synth  # noqa: E402
from genie_smem_amd.index import _ptr  # noqa: E402
from time_mems import tandem_batch  # noqa: E402
from time_mems_contigs import timed  # noqa: E402

CONTIGS = (1, 25, 10_000)
MIN_LEN = 19


def junction_reads(codes, n, L, contigs):
    cuts = np.linspace(0, codes.size, contigs + 1).astype(np.int64)[1:-1]
    i = np.arange(n)
    start = cuts[i % cuts.size] - (20 + i % 111)
    return codes[start[:, None] + np.arange(L)[None, :]].astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the batch sizes (a quick look)")
    ap.add_argument("--once", action="store_true", help="one run of the contig calls alone, for a kernel trace")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L_ = g._native.lib()
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = {"reps": a.reps, "scale": a.scale, "device": torch.cuda.get_device_name(0), "units": "us", "contigs": list(CONTIGS),
           "min_len": MIN_LEN}
    codes = synth.synth_ref(100_000, 100_000)
    n1 = max(1, int(1_000_000 * a.scale))
    n2 = max(2, int(20_000 * a.scale))
    tref, treads = tandem_batch(n2, 150, 3)
    batches = [("cfg1_1Mx150", codes, 15, synth.reads_from_ref_fast(codes, n1, 150, 1), CONTIGS),
               ("tandem7_20kx150", tref, 0, treads, CONTIGS), ("junction_25", codes, 15, junction_reads(codes, n1, 150, 25), (25,))]
    if a.once:
        batches = [(nm, ref, K, reads, (25,)) for nm, ref, K, reads, _ in batches if not nm.startswith("tandem")]
    for name, ref, K, reads, contigs in batches:
        ix = g.GenieIndex.build(ref, K).to("cuda")
        n, L = reads.shape
        total = n * L
        bases = torch.from_numpy(reads.reshape(-1)).cuda()
        offs = torch.arange(n + 1, dtype=torch.int64, device="cuda") * L
        st = torch.empty(n, dtype=torch.int32, device="cuda")
        ws = torch.empty(int(max(L_.genie_match_stats_contigs_workspace_bytes(n, total, L, 0, max(contigs)),
                                 L_.genie_find_smems_contigs_workspace_bytes(n, total, L, 0, max(contigs)))), dtype=torch.uint8, device="cuda")
        row_off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        totals = torch.zeros(1, dtype=torch.int64, device="cuda")
        ms = {k: torch.empty(total, dtype=torch.int32, device="cuda") for k in ("y", "c")}
        lohi = {k: torch.empty((total, 2), dtype=torch.int32, device="cuda") for k in ("y", "c")}
        tables = {c: torch.from_numpy(np.linspace(0, ref.size, c + 1).astype(np.int64)).cuda() for c in contigs}
        for c, t in tables.items():
            g._native.check(L_.genie_contigs_validate(ix._h, _ptr(t), c, sp), "genie_contigs_validate")

        def stats_y():
            g._native.check(L_.genie_match_stats(ix._h, 0, _ptr(bases), _ptr(offs), n, total, L, _ptr(ms["y"]), _ptr(lohi["y"]), _ptr(st),
                                                 _ptr(ws), ws.numel(), sp), "genie_match_stats")

        def stats_c(c):
            g._native.check(L_.genie_match_stats_contigs(ix._h, _ptr(tables[c]), c, 0, _ptr(bases), _ptr(offs), n, total, L, _ptr(ms["c"]),
                                                         _ptr(lohi["c"]), _ptr(st), _ptr(totals), _ptr(ws), ws.numel(), sp),
                            "genie_match_stats_contigs")

        def smems_y(rows):
            g._native.check(L_.genie_find_smems_long_ex(ix._h, 0, 0, _ptr(bases), _ptr(offs), n, total, L, MIN_LEN, _ptr(row_off), _ptr(rows),
                                                        rows.shape[0], _ptr(st), _ptr(ws), ws.numel(), sp), "genie_find_smems_long_ex")

        def smems_c(c, rows):
            g._native.check(L_.genie_find_smems_contigs(ix._h, _ptr(tables[c]), c, 0, 0, _ptr(bases), _ptr(offs), n, total, L, MIN_LEN,
                                                        _ptr(row_off), _ptr(rows), rows.shape[0], _ptr(st), _ptr(totals), _ptr(ws),
                                                        ws.numel(), sp), "genie_find_smems_contigs")

        rows = torch.empty((16 * n, 4), dtype=torch.int32, device="cuda")      # room for every row (checked below)
        rows_c = torch.empty_like(rows)
        if a.once:
            stats_c(25)
            smems_c(25, rows_c)
            torch.cuda.synchronize()
            out[name] = {"reads": n, "clipped": int(totals.item())}
            continue
        res = {"reference_bases": int(ref.size), "reads": n, "read_len": L, "clipped": {}, "smem_rows": {}}
        stats_y()
        fwd = ms["y"].view(n, L) + torch.arange(L, dtype=torch.int32, device="cuda")
        res["run_starts_per_read"] = round(1.0 + float((fwd[:, 1:] != fwd[:, :-1]).sum().item()) / n, 2)
        del fwd
        smems_y(rows)
        res["smem_rows"]["smems"] = int(row_off[-1].item())
        assert res["smem_rows"]["smems"] <= rows.shape[0]
        for c in contigs:
            stats_c(c)
            res["clipped"][f"contigs_{c}"] = int(totals.item())
            smems_c(c, rows_c)
            res["smem_rows"][f"smems_contigs_{c}"] = int(row_off[-1].item())
            if c == 1:
                k = res["smem_rows"]["smems"]
                assert torch.equal(ms["c"], ms["y"]) and torch.equal(lohi["c"], lohi["y"]) and torch.equal(rows_c[:k], rows[:k])
        fns = ((("ms", stats_y),) + tuple((f"ms_contigs_{c}", lambda c=c: stats_c(c)) for c in contigs) +
               (("smems", lambda: smems_y(rows)),) + tuple((f"smems_contigs_{c}", lambda c=c: smems_c(c, rows_c)) for c in contigs))
        res.update(timed(fns, a.reps))
        res["ratio_to_ms"] = {f"ms_contigs_{c}": round(res[f"ms_contigs_{c}"]["median"] / res["ms"]["median"], 3) for c in contigs}
        res["ratio_to_smems"] = {f"smems_contigs_{c}": round(res[f"smems_contigs_{c}"]["median"] / res["smems"]["median"], 3)
                                 for c in contigs}
        out[name] = res
        print(f"# {name}: {json.dumps(res)}", file=sys.stderr, flush=True)
        del bases, offs, st, ws, row_off, totals, tables, ms, lohi, rows, rows_c
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
