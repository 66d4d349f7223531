"""Cost of genie_chain_cigars (the CIGAR of selected chains: the traceback of genie_align_chains) next to
genie_align_chains, taken in the same run on the same batch.  Batches: (a) and (b) of tools/time_align.py:
  cfg1_1Mx150      10^6 x 150-base reads drawn from the 100 kb synthetic reference of BASELINE config 1 cut into 25 equal
                   contigs, min_len 19
  long_1kx10k      10^3 x 10^4-base reads cut from the same reference (25 contigs), 5 % substitutions and four indels of 1 to 30
                   bases each, min_len 15, chaining bandwidth 64
with the wrappers' default parameters.  Calls on preallocated buffers, each with its synchronisation included, timed with HIP
events (torch.cuda.Event) after warm-up runs and interleaved round by round:
  align      genie_align_chains with its totals
  all        genie_chain_cigars with d_sel = NULL: every chain
  best       genie_chain_cigars on the best chain of every read (the highest score among the chains that were not skipped, the
             smaller index on a tie), chosen once beforehand with torch ops
Both cigar calls write the ops (d_cigar sized by a sizing call beforehand) with exactly the direction bytes they need.  The
median and the spread (min, max) of --reps repeats in us, the chains, ops and direction bytes of each selection, and the ratios of
the two calls' medians to genie_align_chains'.  The result is checked once: no chain is flagged but those genie_align_chains
skipped, and every CIGAR consumes its read.  One JSON line.
Usage: python tools/time_cigars.py [--reps 10] [--scale 1.0] [--out profiles/cigars_time.json]"""
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
from tools.time_mems import stats  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the batch sizes (a quick look)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L_ = g._native.lib()
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    none = C.c_void_p(0)
    out = {"reps": a.reps, "scale": a.scale, "device": torch.cuda.get_device_name(0), "units": "us", "chain": DEFAULTS, "align": ALIGN}
    codes = synth.synth_ref(100_000, 100_000)
    n1, n2 = max(1, int(1_000_000 * a.scale)), max(1, int(1_000 * a.scale))
    batches = [("cfg1_1Mx150", codes, 25, synth.reads_from_ref_fast(codes, n1, 150, 1), 19, DEFAULTS),
               ("long_1kx10k", codes, 25, long_reads(codes, n2, 10_000, 2), 15, dict(DEFAULTS, bandwidth=64))]
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
        ws_a = torch.empty(max(256, int(L_.genie_align_chains_workspace_bytes(n, kept))), dtype=torch.uint8, device="cuda")
        aln = torch.empty((max(kept, 1), 8), dtype=torch.int32, device="cuda")
        at = torch.empty(2, dtype=torch.int64, device="cuda")
        head = (ix._h, _ptr(table), n_contigs, 0, _ptr(bases), _ptr(offs), n, total, max_len, _ptr(row_off), _ptr(rows), n, R, _ptr(ac),
                _ptr(apred), _ptr(co), _ptr(chains), kept, *p7)

        def align():
            g._native.check(L_.genie_align_chains(*head, _ptr(aln), _ptr(at), _ptr(ws_a), ws_a.numel(), sp), "genie_align_chains")

        align()
        torch.cuda.synchronize()
        # the best chain of every read, as SMEM.map_reads picks it
        unit = torch.repeat_interleave(torch.arange(n, device="cuda"), co[1:] - co[:-1])
        live = (aln[:kept, 5] & 4) == 0
        score = torch.where(live, aln[:kept, 0].long(), torch.full((kept,), -(1 << 40), dtype=torch.int64, device="cuda"))
        best = torch.full((n,), -(1 << 40), dtype=torch.int64, device="cuda").scatter_reduce(0, unit, score, "amax")
        index = torch.arange(kept, device="cuda")
        pick = torch.full((n,), kept, dtype=torch.int64, device="cuda").scatter_reduce(
            0, unit, torch.where(live & (score == best[unit]), index, torch.full_like(index, kept)), "amin")
        sel_best = pick[pick < kept].contiguous()

        def cigar_call(sel):
            n_sel = kept if sel is None else sel.numel()
            state = {"ops": 0, "dir": 0}
            c_off = torch.empty(n_sel + 1, dtype=torch.int64, device="cuda")
            info = torch.empty((max(n_sel, 1), 8), dtype=torch.int32, device="cuda")
            tt = torch.empty(3, dtype=torch.int64, device="cuda")
            bufs = {}

            def run():
                g._native.check(L_.genie_chain_cigars(*head, _ptr(aln), _ptr(sel) if sel is not None else none, n_sel, _ptr(c_off),
                                                      _ptr(bufs["cigar"]) if state["ops"] else none, state["ops"], _ptr(info), none, _ptr(tt),
                                                      state["dir"], _ptr(bufs["ws"]), bufs["ws"].numel(), sp), "genie_chain_cigars")

            def size():
                bufs["ws"] = torch.empty(max(256, int(L_.genie_chain_cigars_workspace_bytes(n, kept, n_sel if sel is not None else kept,
                                                                                            state["dir"]))), dtype=torch.uint8, device="cuda")
            size()
            run()                                                    # the needs
            state["dir"] = int(tt[2].item())
            size()
            run()                                                    # the sizing call
            state["ops"] = int(c_off[n_sel].item())
            bufs["cigar"] = torch.empty(max(state["ops"], 1), dtype=torch.int32, device="cuda")
            run()
            torch.cuda.synchronize()
            return run, state, c_off, bufs, info, tt, n_sel

        calls = {"all": cigar_call(None), "best": cigar_call(sel_best)}
        read_len = torch.from_numpy(lens).cuda()
        for key, (run, state, c_off, bufs, info, tt, n_sel) in calls.items():
            flagged = info[:n_sel, 1] != 0
            chain = info[:n_sel, 0].long()
            assert bool((info[:n_sel, 1][flagged] == 4).all()) and bool(((aln[chain, 5] & 4) != 0).eq(flagged).all())
            ops = bufs["cigar"][:state["ops"]].long() & 0xFFFFFFFF
            owner = torch.repeat_interleave(torch.arange(n_sel, device="cuda"), c_off[1:] - c_off[:-1])
            code = ops & 15
            used = torch.zeros(n_sel, dtype=torch.int64, device="cuda").index_add_(0, owner, torch.where((code != 2), ops >> 4, 0))
            assert bool((used[~flagged] == read_len[unit[chain[~flagged]]]).all()), "a CIGAR does not consume its read"
        fns = (("align", align), ("all", calls["all"][0]), ("best", calls["best"][0]))
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
        res = {"reference_bases": int(ref.size), "contigs": n_contigs, "reads": n, "bases": total, "min_len": m, "rows": R, "chains": kept,
               "skipped": int(at[1].item())}
        for key, fn in fns:
            res[key] = stats(times[key])
        for key, (run, state, c_off, bufs, info, tt, n_sel) in calls.items():
            res[key].update({"selected": n_sel, "written": int(tt[0].item()), "ops": state["ops"], "direction_bytes": state["dir"],
                             "workspace_bytes": bufs["ws"].numel(), "ratio_to_align_chains": round(res[key]["median"] / res["align"]["median"], 3)})
        out[name] = res
        print(f"# {name}: {json.dumps(res)}", file=sys.stderr, flush=True)
        del calls, bases, offs, rows, row_off, chained, aln, ws_a
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
