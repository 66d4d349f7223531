"""Cost of genie_chain_mems (the MEM rows of every strand-read chained on the device) against two
yardsticks taken in the same run on the same rows: genie_find_mems_contigs, the stage that feeds it, and a device-to-host
copy of the rows it consumes into pinned memory, which is what a caller paid before chaining anywhere else.  Batches:
  cfg1_1Mx150      10^6 x 150-base reads drawn from the 100 kb synthetic reference of BASELINE config 1 cut into 25 equal
                   contigs, min_len 19
  long_1kx10k      10^3 x 10^4-base reads cut from the same reference (25 contigs), 5 % substitutions and four indels of 1 to 30
                   bases each, min_len 15
  tandem7_20kx150  the tandem batch of tools/time_mems.py (one contig), min_len 19, at max_pred 0 and 64
The chaining parameters are the Python wrapper's defaults (max_dist 5000, bandwidth 500, gap_cost 2, max_pred 5000, min_score
40) unless the batch says otherwise.  Calls on preallocated buffers, each with its synchronisation included, timed with HIP
events (torch.cuda.Event) after warm-up runs and interleaved round by round:
  mems     genie_find_mems_contigs with room for every row
  sizing   genie_chain_mems with d_chains and the anchor arrays NULL   (check, contigs, forward + tops + count, scan)
  chains   genie_chain_mems with every output                           (sizing + fill)
  copy     rows -> pinned host memory (torch copy_, non_blocking, then the event)
The median and the spread (min, max) of --reps repeats in us, the rows, units and chains, and the ratios of the chain call's
median to the two yardsticks'.  The chains are checked once: every kept chain scores at least min_score and the anchors of
kept chains add up to the chains' n_anchors.  One JSON line.
Usage: python tools/time_chains.py [--reps 10] [--scale 1.0] [--out profiles/chains_time.json]"""
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
from tools.time_mems import stats, tandem_batch  # noqa: E402

DEFAULTS = dict(max_dist=5000, bandwidth=500, gap_cost=2, max_pred=5000, min_score=40)


def long_reads(ref, n, L, seed):
    """n reads of about L bases: windows of the reference with 5 % substitutions and four indels of 1 .. 30 bases."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        at = int(rng.integers(0, ref.size - L - 200))
        r = ref[at:at + L + 200].copy()
        for cut in np.sort(rng.integers(100, L - 100, 4))[::-1]:
            k = int(rng.integers(1, 31))
            if rng.random() < 0.5:
                r = np.concatenate([r[:cut], r[cut + k:]])                                     # deletion from the read
            else:
                r = np.concatenate([r[:cut], rng.integers(0, 4, k).astype(np.uint8), r[cut:]])  # insertion
        r = r[:L].copy()
        hit = rng.random(r.size) < 0.05
        r[hit] = (r[hit] + rng.integers(1, 4, int(hit.sum()))) & 3
        out.append(r.astype(np.uint8))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the batch sizes (a quick look)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L_ = g._native.lib()
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    none = C.c_void_p(0)
    out = {"reps": a.reps, "scale": a.scale, "device": torch.cuda.get_device_name(0), "units": "us", "defaults": DEFAULTS}
    codes = synth.synth_ref(100_000, 100_000)
    n1, n2, n3 = max(1, int(1_000_000 * a.scale)), max(1, int(1_000 * a.scale)), max(2, int(20_000 * a.scale))
    tref, treads = tandem_batch(n3, 150, 3)
    short = synth.reads_from_ref_fast(codes, n1, 150, 1)
    batches = [("cfg1_1Mx150", codes, 25, short, 19, [DEFAULTS]),
               ("long_1kx10k", codes, 25, long_reads(codes, n2, 10_000, 2), 15, [DEFAULTS]),
               ("tandem7_20kx150", tref, 1, treads, 19, [dict(DEFAULTS, max_pred=0), dict(DEFAULTS, max_pred=64)])]
    for name, ref, n_contigs, reads, m, settings in batches:
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
        rows = None

        def mems(fill):
            g._native.check(L_.genie_find_mems_contigs(ix._h, _ptr(table), n_contigs, 0, _ptr(bases), _ptr(offs), n, total, max_len, m, 0,
                                                       _ptr(row_off), _ptr(rows) if fill else none, rows.shape[0] if fill else 0, _ptr(st),
                                                       _ptr(totals), _ptr(ws_m), ws_m.numel(), sp), "genie_find_mems_contigs")

        mems(False)
        R = int(totals[0].item())
        rows = torch.empty((max(R, 1), 4), dtype=torch.int32, device="cuda")
        mems(True)
        pinned = torch.empty((max(R, 1), 4), dtype=torch.int32).pin_memory()
        ws_c = torch.empty(int(L_.genie_chain_mems_workspace_bytes(n, R, n_contigs)), dtype=torch.uint8, device="cuda")
        co = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        an = [torch.empty(max(R, 1), dtype=torch.int32, device="cuda") for _ in range(3)]
        ct = torch.empty(2, dtype=torch.int64, device="cuda")
        per_unit = (row_off[1:] - row_off[:-1])
        res = {"reference_bases": int(ref.size), "contigs": n_contigs, "reads": n, "bases": total, "min_len": m, "rows": R,
               "rows_per_unit": {"mean": round(R / n, 1), "max": int(per_unit.max().item())},
               "workspace_bytes": {"chain_mems": ws_c.numel(), "find_mems_contigs": ws_m.numel()}}
        for prm in settings:
            p5 = [prm[k] for k in ("max_dist", "bandwidth", "gap_cost", "max_pred", "min_score")]
            chains = None

            def chain(fill):
                g._native.check(L_.genie_chain_mems(ix._h, _ptr(table), n_contigs, _ptr(row_off), _ptr(rows), n, R, *p5, _ptr(co),
                                                    _ptr(chains) if fill else none, chains.shape[0] if fill else 0,
                                                    *[_ptr(t) if fill else none for t in an], _ptr(ct), _ptr(ws_c), ws_c.numel(), sp),
                                "genie_chain_mems")

            chain(False)
            kept, lost = (int(x) for x in ct.tolist())
            chains = torch.empty((max(kept, 1), 8), dtype=torch.int32, device="cuda")
            fns = (("mems", lambda: mems(True)), ("sizing", lambda: chain(False)), ("chains", lambda: chain(True)),
                   ("copy", lambda: pinned.copy_(rows, non_blocking=True)))
            for _, fn in fns + fns:                                  # warm-up
                fn()
            torch.cuda.synchronize()
            assert int(co[-1].item()) == kept and bool((chains[:kept, 4] >= prm["min_score"]).all())
            assert int(chains[:kept, 5].sum().item()) == int((an[0][:R] >= 0).sum().item())
            times = {k: [] for k, _ in fns}
            for _ in range(a.reps):
                for key, fn in fns:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    torch.cuda.synchronize()
                    times[key].append(e0.elapsed_time(e1) * 1e3)
            r = {"chains_kept": kept, "chains_not_kept": lost}
            for key, _ in fns:
                r[key] = stats(times[key])
            r["fill_us"] = round(r["chains"]["median"] - r["sizing"]["median"], 1)
            r["ratio_to_find_mems_contigs"] = round(r["chains"]["median"] / r["mems"]["median"], 3)
            r["ratio_to_copy"] = round(r["chains"]["median"] / r["copy"]["median"], 3)
            r["ns_per_row"] = round(r["chains"]["median"] * 1e3 / max(R, 1), 3)
            res[f"max_pred_{prm['max_pred']}"] = r
            del chains
        out[name] = res
        print(f"# {name}: {json.dumps(res)}", file=sys.stderr, flush=True)
        del bases, offs, st, ws_m, ws_c, rows, pinned, co, an, ct, row_off, totals
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
