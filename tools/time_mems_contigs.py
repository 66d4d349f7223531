"""Cost of the contig calls against their yardsticks, on the batches of tools/time_mems.py:
  cfg1_1Mx150      10^6 x 150-base reads drawn from the 100 kb synthetic reference of BASELINE config 1
  tandem7_20kx150  2 x 10^4 x 150-base reads cut from a 3000-base tandem repeat of GATTACA: seeds of hundreds of rows, so
                   that the call's time is the number of seed occurrences and the lookup's cost per occurrence shows
each at min_len 19 and 33.  Per batch and min_len, calls on preallocated buffers with room for every row, each with its
synchronisation(s) included, timed with HIP events (torch.cuda.Event) after warm-up runs and interleaved round by round:
  mems            genie_find_mems                              (the yardstick: the same build, the same batch)
  contigs_<c>     genie_find_mems_contigs with c equal contigs (c = 1, 25, 10^4: LDS alone, LDS alone, LDS + 4 L2 loads)
and, on the SMEM rows of cfg1 (genie_find_smems_long, min_len 19),
  locate          genie_locate on the (lo, hi) columns
  locate_<c>      genie_locate_contigs with c equal contigs
The median and the spread (min, max) of --reps repeats in us, the rows (hits), and each call's median as a ratio to its
yardstick's.  With one contig the rows are checked to be those of genie_find_mems.  One JSON line.
Usage: python tools/time_mems_contigs.py [--reps 10] [--scale 1.0] [--out profiles/mems_contigs_time.json]"""
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
from time_mems import stats, tandem_batch  # noqa: E402

CONTIGS = (1, 25, 10_000)


def timed(fns, reps):
    for _, fn in fns + fns:                                          # warm-up
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k, _ in fns}
    for _ in range(reps):
        for key, fn in fns:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[key].append(e0.elapsed_time(e1) * 1e3)
    return {k: stats(v) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the batch sizes (a quick look)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L_ = g._native.lib()
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = {"reps": a.reps, "scale": a.scale, "device": torch.cuda.get_device_name(0), "units": "us", "contigs": list(CONTIGS)}
    codes = synth.synth_ref(100_000, 100_000)
    n1 = max(1, int(1_000_000 * a.scale))
    n2 = max(2, int(20_000 * a.scale))
    tref, treads = tandem_batch(n2, 150, 3)
    batches = [("cfg1_1Mx150", codes, 15, synth.reads_from_ref_fast(codes, n1, 150, 1)), ("tandem7_20kx150", tref, 0, treads)]
    for name, ref, K, reads in batches:
        ix = g.GenieIndex.build(ref, K).to("cuda")
        n, L = reads.shape
        total = n * L
        bases = torch.from_numpy(reads.reshape(-1)).cuda()
        offs = torch.arange(n + 1, dtype=torch.int64, device="cuda") * L
        st = torch.empty(n, dtype=torch.int32, device="cuda")
        ws = torch.empty(int(L_.genie_find_mems_contigs_workspace_bytes(n, total, L, 0, max(CONTIGS))), dtype=torch.uint8, device="cuda")
        row_off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        totals = torch.empty(2, dtype=torch.int64, device="cuda")
        tables = {c: torch.from_numpy(np.linspace(0, ref.size, c + 1).astype(np.int64)).cuda() for c in CONTIGS}
        for c, t in tables.items():
            g._native.check(L_.genie_contigs_validate(ix._h, _ptr(t), c, sp), "genie_contigs_validate")
        res = {"reference_bases": int(ref.size), "reads": n, "read_len": L}
        for m in (19, 33):
            bufs = {}

            def mems(rows):
                g._native.check(L_.genie_find_mems(ix._h, 0, _ptr(bases), _ptr(offs), n, total, L, m, 0, _ptr(row_off), _ptr(rows),
                                                   rows.shape[0] if rows is not None else 0, _ptr(st), _ptr(totals), _ptr(ws),
                                                   ws.numel(), sp), "genie_find_mems")

            def contigs(c, rows):
                g._native.check(L_.genie_find_mems_contigs(ix._h, _ptr(tables[c]), c, 0, _ptr(bases), _ptr(offs), n, total, L, m, 0,
                                                           _ptr(row_off), _ptr(rows), rows.shape[0] if rows is not None else 0,
                                                           _ptr(st), _ptr(totals), _ptr(ws), ws.numel(), sp), "genie_find_mems_contigs")

            r = {"rows": {}}
            for key, sizing in [("mems", lambda: mems(None))] + [(f"contigs_{c}", lambda c=c: contigs(c, None)) for c in CONTIGS]:
                sizing()                                             # learns the row total
                r["rows"][key] = int(totals[0].item())
                bufs[key] = torch.empty((max(r["rows"][key], 1), 4), dtype=torch.int32, device="cuda")
            fns = (("mems", lambda: mems(bufs["mems"])),) + tuple((f"contigs_{c}", lambda c=c: contigs(c, bufs[f"contigs_{c}"]))
                                                                  for c in CONTIGS)
            r.update(timed(fns, a.reps))
            assert r["rows"]["contigs_1"] == r["rows"]["mems"] and torch.equal(bufs["contigs_1"], bufs["mems"])
            r["ratio_to_mems"] = {f"contigs_{c}": round(r[f"contigs_{c}"]["median"] / r["mems"]["median"], 3) for c in CONTIGS}
            res[f"min_len_{m}"] = r
            del bufs
        if name.startswith("cfg1"):
            smem = ix.find_smems_long("bwa", bases, offs, 19)[1].contiguous()
            S = smem.shape[0]
            tmp = torch.empty(int(max(L_.genie_locate_tmp_bytes(S), L_.genie_locate_contigs_tmp_bytes(S))), dtype=torch.uint8, device="cuda")
            hit_off = torch.empty(S + 1, dtype=torch.int64, device="cuda")
            lohi = C.c_void_p(smem.data_ptr() + 8)
            bufs, hits = {}, {}

            def locate(pos):
                g._native.check(L_.genie_locate(ix._h, lohi, 4, S, _ptr(hit_off), _ptr(pos), pos.numel() if pos is not None else 0,
                                                _ptr(tmp), tmp.numel(), sp), "genie_locate")

            def locate_contigs(c, buf):
                g._native.check(L_.genie_locate_contigs(ix._h, _ptr(tables[c]), c, _ptr(smem), S, _ptr(hit_off), _ptr(buf),
                                                        buf.shape[0] if buf is not None else 0, _ptr(totals), _ptr(tmp), tmp.numel(), sp),
                                "genie_locate_contigs")

            locate(None)
            hits["locate"] = int(hit_off[-1].item())
            bufs["locate"] = torch.empty(max(hits["locate"], 1), dtype=torch.int32, device="cuda")
            dropped = {}
            for c in CONTIGS:
                locate_contigs(c, None)
                hits[f"locate_{c}"], dropped[f"locate_{c}"] = (int(x) for x in totals.tolist())
                bufs[f"locate_{c}"] = torch.empty((max(hits[f"locate_{c}"], 1), 2), dtype=torch.int32, device="cuda")
            fns = (("locate", lambda: locate(bufs["locate"])),) + tuple((f"locate_{c}", lambda c=c: locate_contigs(c, bufs[f"locate_{c}"]))
                                                                        for c in CONTIGS)
            r = {"smem_rows": S, "hits": hits, "dropped_as_bridging": dropped}
            r.update(timed(fns, a.reps))
            r["ratio_to_locate"] = {f"locate_{c}": round(r[f"locate_{c}"]["median"] / r["locate"]["median"], 3) for c in CONTIGS}
            res["locate_smems_min_len_19"] = r
            del bufs, smem, tmp, hit_off
        out[name] = res
        print(f"# {name}: {json.dumps(res)}", file=sys.stderr, flush=True)
        del bases, offs, st, ws, row_off, totals, tables
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
