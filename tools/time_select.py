"""Cost of genie_select_alignments (primary, supplementary and secondary alignments of every read with a mapping quality,
DESIGN.md section 25) next to the torch selection block of SMEM.map_reads and next to genie_align_chains, taken in the same run
on the same batch.  Batches: (a), (b) and the tandem batch of tools/time_align.py:
  cfg1_1Mx150      10^6 x 150-base reads drawn from the 100 kb synthetic reference of BASELINE config 1 cut into 25 equal
                   contigs, min_len 19
  long_1kx10k      10^3 x 10^4-base reads cut from the same reference (25 contigs), 5 % substitutions and four indels of 1 to 30
                   bases each, min_len 15, chaining bandwidth 64
  tandem7_20kx150  the tandem batch of tools/time_mems.py (one contig), min_len 19, chained at max_pred 64 and bandwidth 64: reads
                   that carry hundreds of chains
with the wrappers' default parameters (mask_level 50, pri_ratio 80, max_secondary 5, min_score 1, mapq_full 40).  Calls on
preallocated buffers, each with its synchronisation included, timed with HIP events (torch.cuda.Event) after warm-up runs and
interleaved round by round:
  align      genie_align_chains with its totals
  select     genie_select_alignments with every output, d_sel sized by a sizing call beforehand
  sizing     the same call with d_sel = NULL
  torch      the selection block of SMEM.map_reads: the best chain of every read that was not skipped, the smaller index on a tie
             (a repeat_interleave, two scatter_reduces and the element-wise calls around them), up to the selection tensor
The median and the spread (min, max) of --reps repeats in us, the chains per read (mean, largest), the reads on the wave path,
the totals, and the ratios of the call's median to the two yardsticks'.  The result is checked once: the kind-0 chain of every
read is the chain the torch block picks.  One JSON line.
Usage: python tools/time_select.py [--reps 10] [--scale 1.0] [--out profiles/select_time.json]"""
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
from tools.time_chains import DEFAULTS, long_reads  # noqa: E402
from tools.time_mems import stats, tandem_batch  # noqa: E402

SELECT = dict(mask_level=50, pri_ratio=80, max_secondary=5, min_score=1, mapq_full=40)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the batch sizes (a quick look)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L_ = g._native.lib()
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    none = C.c_void_p(0)
    out = {"reps": a.reps, "scale": a.scale, "device": torch.cuda.get_device_name(0), "units": "us", "chain": DEFAULTS, "align": ALIGN,
           "select": SELECT, "lane_max": g._native.SELECT_LANE_MAX, "tile": g._native.SELECT_TILE}
    codes = synth.synth_ref(100_000, 100_000)
    n1, n2, n3 = max(1, int(1_000_000 * a.scale)), max(1, int(1_000 * a.scale)), max(2, int(20_000 * a.scale))
    tref, treads = tandem_batch(n3, 150, 3)
    batches = [("cfg1_1Mx150", codes, 25, synth.reads_from_ref_fast(codes, n1, 150, 1), 19, DEFAULTS),
               ("long_1kx10k", codes, 25, long_reads(codes, n2, 10_000, 2), 15, dict(DEFAULTS, bandwidth=64)),
               ("tandem7_20kx150", tref, 1, treads, 19, dict(DEFAULTS, max_pred=64, bandwidth=64))]
    for name, ref, n_contigs, reads, m, cprm in batches:
        ix = g.GenieIndex.build(ref, 0).to("cuda")
        if isinstance(reads, np.ndarray):
            n, L = reads.shape
            lens = np.full(n, L, np.int64)
            flat = reads.reshape(-1)
        else:
            n, lens = len(reads), np.asarray([len(r) for r in reads], np.int64)
            flat = np.concatenate(reads)
        total, max_len = int(flat.size), int(lens.max())
        bases = torch.from_numpy(np.ascontiguousarray(flat)).cuda()
        offs = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).cuda()
        rs = g.ReferenceSet([str(i) for i in range(n_contigs)], np.linspace(0, ref.size, n_contigs + 1).astype(np.int64), ref)
        table = torch.from_numpy(rs.offsets).cuda()
        row_off, rows, _, _ = ix.find_mems_contigs(rs, bases, offs, m)
        chained = ix.chain_mems(row_off, rows, rs, **cprm)
        co, chains, ac, apred = chained[:4]
        R, kept = rows.shape[0], chains.shape[0]
        p7 = [ALIGN[k] for k in ("match", "mismatch", "gap_open", "gap_extend", "band", "max_indel", "end_bonus")]
        p5 = [SELECT[k] for k in ("mask_level", "pri_ratio", "max_secondary", "min_score", "mapq_full")]
        ws_a = torch.empty(max(256, int(L_.genie_align_chains_workspace_bytes(n, kept))), dtype=torch.uint8, device="cuda")
        aln = torch.empty((max(kept, 1), 8), dtype=torch.int32, device="cuda")
        at = torch.empty(2, dtype=torch.int64, device="cuda")

        def align():
            g._native.check(L_.genie_align_chains(ix._h, _ptr(table), n_contigs, 0, _ptr(bases), _ptr(offs), n, total, max_len, _ptr(row_off),
                                                  _ptr(rows), n, R, _ptr(ac), _ptr(apred), _ptr(co), _ptr(chains), kept, *p7, _ptr(aln), _ptr(at),
                                                  _ptr(ws_a), ws_a.numel(), sp), "genie_align_chains")

        align()
        torch.cuda.synchronize()
        ws_s = torch.empty(max(256, int(L_.genie_select_alignments_workspace_bytes(n, kept))), dtype=torch.uint8, device="cuda")
        klass = torch.empty((max(kept, 1), 4), dtype=torch.int32, device="cuda")
        s_off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        counts = torch.empty((n, 4), dtype=torch.int32, device="cuda")
        tt = torch.empty(4, dtype=torch.int64, device="cuda")
        bufs = {"cap": 0, "sel": None, "rec": None}

        def select(sizing=False):
            given = not sizing and bufs["cap"] > 0
            g._native.check(L_.genie_select_alignments(ix._h, _ptr(table), n_contigs, 0, _ptr(offs), n, _ptr(co), n, _ptr(chains), _ptr(aln),
                                                       kept, *p5, _ptr(klass), _ptr(s_off), _ptr(bufs["sel"]) if given else none,
                                                       _ptr(bufs["rec"]) if given else none, bufs["cap"] if given else 0, _ptr(counts), _ptr(tt),
                                                       _ptr(ws_s), ws_s.numel(), sp), "genie_select_alignments")

        select(True)
        bufs["cap"] = int(s_off[n].item())
        bufs["sel"] = torch.empty(max(bufs["cap"], 1), dtype=torch.int64, device="cuda")
        bufs["rec"] = torch.empty((max(bufs["cap"], 1), 12), dtype=torch.int32, device="cuda")
        picked = {}

        def torch_block():
            unit = torch.repeat_interleave(torch.arange(n, device="cuda"), co[1:] - co[:-1])
            live = (aln[:kept, 5] & 4) == 0
            score = torch.where(live, aln[:kept, 0].long(), torch.full((kept,), -(1 << 40), dtype=torch.int64, device="cuda"))
            best = torch.full((n,), -(1 << 40), dtype=torch.int64, device="cuda").scatter_reduce(0, unit, score, "amax")
            index = torch.arange(kept, device="cuda")
            cand = torch.where(live & (score == best[unit]), index, torch.full_like(index, kept))
            pick = torch.full((n,), kept, dtype=torch.int64, device="cuda").scatter_reduce(0, unit, cand, "amin")
            picked["sel"] = pick[pick < kept]

        select()
        torch_block()
        torch.cuda.synchronize()
        rec = bufs["rec"][:bufs["cap"]]
        # the torch block knows no min_score: a read whose best chain scores below it has a pick there and no primary here
        scored = aln[picked["sel"], 0] >= SELECT["min_score"]
        want, got = picked["sel"][scored], rec[rec[:, 2] == 0, 1].long()
        if not torch.equal(got, want):
            k = min(got.numel(), want.numel())
            at = int((got[:k] != want[:k]).nonzero()[0].item()) if k and bool((got[:k] != want[:k]).any()) else k
            rows_ = {w: aln[v[at:at + 1]].tolist() for w, v in (("select", got), ("torch", want))}
            raise SystemExit(f"{name}: the primary of a read is not the chain the torch block picks: {got.numel()} against {want.numel()}, "
                             f"first at {at}: {got[at:at + 3].tolist()} against {want[at:at + 3].tolist()}, aln rows {rows_}")
        per_read = (co[1:] - co[:-1])
        fns = (("align", align), ("select", select), ("sizing", lambda: select(True)), ("torch", torch_block))
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
        select()
        torch.cuda.synchronize()
        res = {"reference_bases": int(ref.size), "contigs": n_contigs, "reads": n, "bases": total, "min_len": m, "rows": R, "chains": kept,
               "skipped": int(at[1].item()), "chains_per_read_mean": round(kept / n, 3), "chains_per_read_max": int(per_read.max().item()),
               "reads_on_the_wave_path": int((per_read > g._native.SELECT_LANE_MAX).sum().item()),
               "totals": dict(zip(("candidates", "primaries", "secondaries", "selected"), (int(v) for v in tt.tolist()))),
               "primaries_per_read_max": int(counts[:, 1].max().item()), "workspace_bytes": ws_s.numel(),
               "reads_whose_best_chain_is_below_min_score": int((~scored).sum().item())}
        for key, fn in fns:
            res[key] = stats(times[key])
        res["select"]["ratio_to_torch_block"] = round(res["select"]["median"] / res["torch"]["median"], 3)
        res["select"]["ratio_to_align_chains"] = round(res["select"]["median"] / res["align"]["median"], 4)
        out[name] = res
        print(f"# {name}: {json.dumps(res)}", file=sys.stderr, flush=True)
        del bases, offs, rows, row_off, chained, aln, ws_a, ws_s, klass, bufs
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
