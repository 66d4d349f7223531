"""Cost of genie_pair_alignments (the alignments of paired-end reads with SAM's per-record fields) next to
genie_select_alignments, taken in the same run on the same batches, the reads taken two by two as mates:
  cfg1_500kx2x150   batch (a) of tools/time_select.py read as 5 x 10^5 pairs: 10^6 x 150-base reads drawn
                    from the 100 kb synthetic reference of BASELINE config 1 cut into 25 equal contigs, min_len 19, max_secondary 5
  tandem7_10kx2x150 the tandem batch of tools/time_mems.py (one contig) read as 10^4 pairs, min_len 19, chained at max_pred 64 and
                    bandwidth 64, selected with max_secondary 16: 17 records per read, 289 combinations per pair, so that every pair
                    is wide
with the wrapper's default pairing parameters except orient, which allows every orientation: the reads of both batches are drawn
from the forward strand.  Calls on preallocated buffers, each with its synchronisation included, timed with HIP events
(torch.cuda.Event) after warm-up runs and interleaved round by round:
  select     genie_select_alignments with every output, d_sel sized by the wrapper's call beforehand
  pair       genie_pair_alignments with every output
The median and the spread (min, max) of --reps repeats in us, the records per read, the pairs on the wave path, the totals, and
the ratio of the call's median to the select call's.  The result is checked once: the totals are those of the d_pairs flags, every
record of a proper pair carries 0x2, and the chosen records name each other as mates.  One JSON line.
Usage: python tools/time_pair.py [--reps 10] [--scale 1.0] [--out profiles/pair_time.json]"""
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
from tools.time_align import ALIGN  # noqa: E402
from tools.time_chains import DEFAULTS  # noqa: E402
from tools.time_mems import stats, tandem_batch  # noqa: E402

SELECT = dict(mask_level=50, pri_ratio=80, max_secondary=5, min_score=1, mapq_full=40)
PAIR = dict(orient=7, isize_min=0, isize_max=1000, isize_mean=300, pen_slope=8, pen_max=16, pen_unpaired=17, mapq_boost=40)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the batch sizes (a quick look)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L_ = g._native.lib()
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = {"reps": a.reps, "scale": a.scale, "device": torch.cuda.get_device_name(0), "units": "us", "chain": DEFAULTS, "align": ALIGN,
           "pair": PAIR, "lane_max": g._native.PAIR_LANE_MAX, "tile": g._native.PAIR_TILE}
    codes = synth.synth_ref(100_000, 100_000)
    n1, n3 = 2 * max(1, int(500_000 * a.scale)), 2 * max(1, int(10_000 * a.scale))
    tref, treads = tandem_batch(n3, 150, 3)
    batches = [("cfg1_500kx2x150", codes, 25, synth.reads_from_ref_fast(codes, n1, 150, 1), 19, DEFAULTS, SELECT),
               ("tandem7_10kx2x150", tref, 1, treads, 19, dict(DEFAULTS, max_pred=64, bandwidth=64), dict(SELECT, max_secondary=16))]
    for name, ref, n_contigs, reads, m, cprm, sprm in batches:
        ix = g.GenieIndex.build(ref, 0).to("cuda")
        if isinstance(reads, np.ndarray):
            n, L = reads.shape
            lens = np.full(n, L, np.int64)
            flat = reads.reshape(-1)
        else:
            n, lens = len(reads), np.asarray([len(r) for r in reads], np.int64)
            flat = np.concatenate(reads)
        bases = torch.from_numpy(np.ascontiguousarray(flat)).cuda()
        offs = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).cuda()
        rs = g.ReferenceSet([str(i) for i in range(n_contigs)], np.linspace(0, ref.size, n_contigs + 1).astype(np.int64), ref)
        table = torch.from_numpy(rs.offsets).cuda()
        row_off, rows, _, _ = ix.find_mems_contigs(rs, bases, offs, m)
        chained = ix.chain_mems(row_off, rows, rs, **cprm)
        co, chains = chained[:2]
        aln, _ = ix.align_chains((bases, offs), row_off, rows, chained, rs, **ALIGN)
        kept = chains.shape[0]
        p5 = [sprm[k] for k in ("mask_level", "pri_ratio", "max_secondary", "min_score", "mapq_full")]
        p8 = [PAIR[k] for k in ("orient", "isize_min", "isize_max", "isize_mean", "pen_slope", "pen_max", "pen_unpaired", "mapq_boost")]
        ws_s = torch.empty(max(256, int(L_.genie_select_alignments_workspace_bytes(n, kept))), dtype=torch.uint8, device="cuda")
        klass = torch.empty((max(kept, 1), 4), dtype=torch.int32, device="cuda")
        s_off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        counts = torch.empty((n, 4), dtype=torch.int32, device="cuda")
        tt = torch.empty(4, dtype=torch.int64, device="cuda")
        sel, rec = (t.contiguous() for t in ix.select_alignments(offs, co, chains, aln, rs, False, **sprm)[1:3])
        cap = rec.shape[0]

        def select():
            g._native.check(L_.genie_select_alignments(ix._h, _ptr(table), n_contigs, 0, _ptr(offs), n, _ptr(co), n, _ptr(chains), _ptr(aln),
                                                       kept, *p5, _ptr(klass), _ptr(s_off), _ptr(sel), _ptr(rec), cap, _ptr(counts), _ptr(tt),
                                                       _ptr(ws_s), ws_s.numel(), sp), "genie_select_alignments")

        ws_p = torch.empty(max(256, int(L_.genie_pair_alignments_workspace_bytes(n, cap))), dtype=torch.uint8, device="cuda")
        pairs = torch.empty((n // 2, 8), dtype=torch.int32, device="cuda")
        sam = torch.empty((max(cap, 1), 4), dtype=torch.int32, device="cuda")
        pt = torch.empty(4, dtype=torch.int64, device="cuda")

        def pair():
            g._native.check(L_.genie_pair_alignments(ix._h, n, _ptr(s_off), _ptr(rec), cap, _ptr(klass), kept, *p8, _ptr(pairs), _ptr(sam),
                                                     _ptr(pt), _ptr(ws_p), ws_p.numel(), sp), "genie_pair_alignments")

        select()
        pair()
        torch.cuda.synchronize()
        flags, got = pairs[:, 2], sam[:cap]
        both, one = (flags & 6) == 6, ((flags & 6) == 2) | ((flags & 6) == 4)
        want = [int(both.sum()), int((flags & 1).sum()), int(((flags >> 3) & 1).sum() + ((flags >> 4) & 1).sum()), int(one.sum())]
        if pt.tolist() != want:
            raise SystemExit(f"{name}: the totals {pt.tolist()} are not those of the flags {want}")
        proper = (flags & 1) == 1
        r0, r1 = pairs[proper, 0].long(), pairs[proper, 1].long()
        if not (torch.equal(got[r0, 2].long(), r1) and torch.equal(got[r1, 2].long(), r0) and bool((got[r0, 0] & 2).all())):
            raise SystemExit(f"{name}: the chosen records of a proper pair do not name each other")
        pair_of = rec[:cap, 0].long() // 2
        if not torch.equal((got[:, 0] & 2) != 0, proper[pair_of]):
            raise SystemExit(f"{name}: 0x2 is not on exactly the records of the proper pairs")
        fns = (("select", select), ("pair", pair))
        for _, fn in fns + fns:                                      # warm-up
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k, _ in fns}
        for _ in range(a.reps):
            for key, fn in fns:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                times[key].append(e0.elapsed_time(e1) * 1e3)
        per_read = s_off[1:] - s_off[:-1]
        combos = per_read[0::2] * per_read[1::2]
        res = {"reference_bases": int(ref.size), "contigs": n_contigs, "reads": n, "pairs": n // 2, "min_len": m, "chains": kept,
               "max_secondary": sprm["max_secondary"], "records": cap, "records_per_read_max": int(per_read.max().item()),
               "combinations": int(combos.sum().item()), "combinations_per_pair_max": int(combos.max().item()),
               "pairs_on_the_wave_path": int((combos > g._native.PAIR_LANE_MAX).sum().item()),
               "totals": dict(zip(("both_mapped", "proper", "displaced_mates", "one_mapped"), (int(v) for v in pt.tolist()))),
               "concordant_per_pair_max": int(pairs[:, 6].max().item()), "workspace_bytes": ws_p.numel()}
        for key, fn in fns:
            res[key] = stats(times[key])
        res["pair"]["ratio_to_select_alignments"] = round(res["pair"]["median"] / res["select"]["median"], 3)
        out[name] = res
        print(f"# {name}: {json.dumps(res)}", file=sys.stderr, flush=True)
        del bases, offs, rows, row_off, chained, aln, ws_s, ws_p, klass, sel, rec, sam, pairs
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
