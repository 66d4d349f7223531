"""Cost of genie_align_chains (every chain aligned on the device: banded gap fill and end extension) next to
the two calls that feed it, taken in the same run on the same batch: genie_find_mems_contigs and genie_chain_mems.  Batches:
those of tools/time_chains.py:
  cfg1_1Mx150      10^6 x 150-base reads drawn from the 100 kb synthetic reference of BASELINE config 1 cut into 25 equal
                   contigs, min_len 19
  long_1kx10k      10^3 x 10^4-base reads cut from the same reference (25 contigs), 5 % substitutions and four indels of 1 to 30
                   bases each, min_len 15
  tandem7_20kx150  the tandem batch of tools/time_mems.py (one contig), min_len 19, chained at max_pred 64
The chaining and alignment parameters are the Python wrappers' defaults (match 1, mismatch 4, gap_open 6, gap_extend 1, band 32,
max_indel 64, end_bonus 5) unless the batch says otherwise.  Calls on preallocated buffers, each with its synchronisation
included, timed with HIP events (torch.cuda.Event) after warm-up runs and interleaved round by round:
  mems     genie_find_mems_contigs with room for every row
  chains   genie_chain_mems with every output
  align    genie_align_chains with its totals
The median and the spread (min, max) of --reps repeats in us, the rows, chains and members, the rows of the dynamic programs
(query bases of the gaps that are not one-sided, and of the extensions) counted on the host from the outputs, and the ratios of
the align call's median to the two others'.  The result is checked once: no chain of these batches is skipped by max_indel
where bandwidth <= max_indel, every score is at most match x the read's length + 2 end_bonus, and matched <= q_end - q_begin.
One JSON line.
Usage: python tools/time_align.py [--reps 10] [--scale 1.0] [--out profiles/align_time.json]"""
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
from tools.time_chains import DEFAULTS, long_reads  # noqa: E402
from tools.time_mems import stats, tandem_batch  # noqa: E402

ALIGN = dict(match=1, mismatch=4, gap_open=6, gap_extend=1, band=32, max_indel=64, end_bonus=5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the batch sizes (a quick look)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L_ = g._native.lib()
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = {"reps": a.reps, "scale": a.scale, "device": torch.cuda.get_device_name(0), "units": "us", "chain": DEFAULTS, "align": ALIGN}
    codes = synth.synth_ref(100_000, 100_000)
    n1, n2, n3 = max(1, int(1_000_000 * a.scale)), max(1, int(1_000 * a.scale)), max(2, int(20_000 * a.scale))
    tref, treads = tandem_batch(n3, 150, 3)
    short = synth.reads_from_ref_fast(codes, n1, 150, 1)
    # max_indel follows the chaining bandwidth on the long reads: their indels reach 30 bases, the default bandwidth 500
    batches = [("cfg1_1Mx150", codes, 25, short, 19, DEFAULTS, ALIGN),
               ("long_1kx10k", codes, 25, long_reads(codes, n2, 10_000, 2), 15, dict(DEFAULTS, bandwidth=64), ALIGN),
               ("tandem7_20kx150", tref, 1, treads, 19, dict(DEFAULTS, max_pred=64, bandwidth=64), ALIGN)]
    for name, ref, n_contigs, reads, m, cprm, aprm in batches:
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
        table = torch.from_numpy(np.linspace(0, ref.size, n_contigs + 1).astype(np.int64)).cuda()
        st = torch.empty(n, dtype=torch.int32, device="cuda")
        ws_m = torch.empty(int(L_.genie_find_mems_contigs_workspace_bytes(n, total, max_len, 0, n_contigs)), dtype=torch.uint8, device="cuda")
        row_off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        totals = torch.empty(2, dtype=torch.int64, device="cuda")
        rows = torch.empty((1, 4), dtype=torch.int32, device="cuda")

        def mems(cap):
            g._native.check(L_.genie_find_mems_contigs(ix._h, _ptr(table), n_contigs, 0, _ptr(bases), _ptr(offs), n, total, max_len, m, 0,
                                                       _ptr(row_off), _ptr(rows), cap, _ptr(st), _ptr(totals), _ptr(ws_m), ws_m.numel(), sp),
                            "genie_find_mems_contigs")

        mems(0)
        R = int(totals[0].item())
        rows = torch.empty((max(R, 1), 4), dtype=torch.int32, device="cuda")
        mems(R)
        ws_c = torch.empty(int(L_.genie_chain_mems_workspace_bytes(n, R, n_contigs)), dtype=torch.uint8, device="cuda")
        co = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        an = [torch.empty(max(R, 1), dtype=torch.int32, device="cuda") for _ in range(3)]
        ct = torch.empty(2, dtype=torch.int64, device="cuda")
        p5 = [cprm[k] for k in ("max_dist", "bandwidth", "gap_cost", "max_pred", "min_score")]
        chains = torch.empty((1, 8), dtype=torch.int32, device="cuda")

        def chain(cap):
            g._native.check(L_.genie_chain_mems(ix._h, _ptr(table), n_contigs, _ptr(row_off), _ptr(rows), n, R, *p5, _ptr(co), _ptr(chains),
                                                cap, *[_ptr(t) for t in an], _ptr(ct), _ptr(ws_c), ws_c.numel(), sp), "genie_chain_mems")

        chain(0)
        kept = int(ct[0].item())
        chains = torch.empty((max(kept, 1), 8), dtype=torch.int32, device="cuda")
        chain(kept)
        p7 = [aprm[k] for k in ("match", "mismatch", "gap_open", "gap_extend", "band", "max_indel", "end_bonus")]
        ws_a = torch.empty(max(256, int(L_.genie_align_chains_workspace_bytes(n, kept))), dtype=torch.uint8, device="cuda")
        aln = torch.empty((max(kept, 1), 8), dtype=torch.int32, device="cuda")
        at = torch.empty(2, dtype=torch.int64, device="cuda")

        def align():
            g._native.check(L_.genie_align_chains(ix._h, _ptr(table), n_contigs, 0, _ptr(bases), _ptr(offs), n, total, max_len, _ptr(row_off),
                                                  _ptr(rows), n, R, _ptr(an[0]), _ptr(an[1]), _ptr(co), _ptr(chains), kept, *p7, _ptr(aln),
                                                  _ptr(at), _ptr(ws_a), ws_a.numel(), sp), "genie_align_chains")

        fns = (("mems", lambda: mems(R)), ("chains", lambda: chain(kept)), ("align", align))
        for _, fn in fns + fns:                                      # warm-up
            fn()
        torch.cuda.synchronize()
        al = aln[:kept].cpu().numpy().astype(np.int64)
        ch = chains[:kept].cpu().numpy().astype(np.int64)
        co_h = co.cpu().numpy()
        read_len = np.repeat(lens, np.diff(co_h))
        aligned, skipped = (int(x) for x in at.tolist())
        ok = al[:, 5] != 4
        assert aligned + skipped == kept and skipped == int((~ok).sum())
        assert cprm["bandwidth"] > aprm["max_indel"] or skipped == 0
        assert (al[ok, 0] <= aprm["match"] * read_len[ok] + 2 * aprm["end_bonus"]).all() and (al[ok, 7] <= al[ok, 2] - al[ok, 1]).all()
        times = {k: [] for k, _ in fns}
        for _ in range(a.reps):
            for key, fn in fns:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                times[key].append(e0.elapsed_time(e1) * 1e3)
        # the rows of the extensions' programs: the query bases outside the chain's span, at both ends
        ext_rows = int((ch[ok, 0] + read_len[ok] - ch[ok, 1]).sum())
        res = {"reference_bases": int(ref.size), "contigs": n_contigs, "reads": n, "bases": total, "min_len": m, "rows": R, "chains": kept,
               "members": int(ch[:, 5].sum()), "members_used": int(al[:, 6].sum()), "skipped": skipped, "extension_rows": ext_rows,
               "to_both_ends": int(((al[:, 5] & 3) == 3).sum()), "mean_score": round(float(al[ok, 0].mean()), 1) if ok.any() else 0.0,
               "workspace_bytes": {"align_chains": ws_a.numel(), "chain_mems": ws_c.numel(), "find_mems_contigs": ws_m.numel()}}
        for key, _ in fns:
            res[key] = stats(times[key])
        res["ratio_to_find_mems_contigs"] = round(res["align"]["median"] / res["mems"]["median"], 3)
        res["ratio_to_chain_mems"] = round(res["align"]["median"] / res["chains"]["median"], 3)
        res["ns_per_chain"] = round(res["align"]["median"] * 1e3 / max(kept, 1), 3)
        out[name] = res
        print(f"# {name}: {json.dumps(res)}", file=sys.stderr, flush=True)
        del bases, offs, st, ws_m, ws_c, ws_a, rows, co, an, ct, at, row_off, totals, chains, aln
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
