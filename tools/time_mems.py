"""Cost of genie_find_mems (every maximal exact match of a read batch) against its yardstick: the
nearest thing the library could do before it, genie_match_stats with intervals followed by genie_locate on those intervals,
on the same batch and the same handle, in the same run.  Batches:
  cfg1_1Mx150      10^6 x 150-base reads drawn from the 100 kb synthetic reference of BASELINE config 1
  tandem7_20kx150  2 x 10^4 x 150-base reads cut from a 3000-base tandem repeat of GATTACA with one substituted base per 500,
                   every second read with one more substitution: seeds of hundreds of rows
each at min_len 19 and 33.  Per batch and min_len, calls on preallocated buffers, each with its synchronisation(s) included,
timed with HIP events (torch.cuda.Event) after warm-up runs and interleaved round by round:
  stats      genie_match_stats with d_lohi               (the first stage of the call, alone)
  sizing     genie_find_mems with d_rows = NULL          (stats, seed, count, scan, offsets)
  mems       genie_find_mems with room for every row     (sizing + fill)
  yardstick  genie_match_stats with d_lohi, then genie_locate over the intervals of the positions with ms >= min_len (the
             others masked to (-1, -1) by one torch.where, which is timed with it: a caller's filter; room for every position)
The median and the spread (min, max) of --reps repeats in us, the rows, the yardstick's positions, the ratio of the call's
median to the yardstick's, and the split by differences: seed + count = sizing - stats, fill = mems - sizing.  The rows are
checked once against the matching statistics: every row's length is at least min_len and at most ms of its start.
One JSON line.
Usage: python tools/time_mems.py [--reps 10] [--scale 1.0] [--out profiles/mems_time.json]"""
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


def tandem_batch(n, L, seed):
    rng = np.random.default_rng(seed)
    unit = np.asarray([2, 0, 3, 3, 0, 1, 0], np.uint8)               # GATTACA
    ref = np.tile(unit, 3000 // 7 + 1)[:3000].copy()
    ref[250::500] = (ref[250::500] + 2) & 3
    start = rng.integers(0, ref.size - L, n)
    reads = ref[start[:, None] + np.arange(L)[None, :]]
    odd = np.arange(1, n, 2)
    at = rng.integers(0, L, odd.size)
    reads[odd, at] = (reads[odd, at] + 1 + rng.integers(0, 3, odd.size)) & 3
    return ref, np.ascontiguousarray(reads, np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the batch sizes (a quick look)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L_ = g._native.lib()
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = {"reps": a.reps, "scale": a.scale, "device": torch.cuda.get_device_name(0), "units": "us"}
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
        ms = torch.empty(total, dtype=torch.int32, device="cuda")
        lohi = torch.empty((total, 2), dtype=torch.int32, device="cuda")
        st = torch.empty(n, dtype=torch.int32, device="cuda")
        ws_ms = torch.empty(int(L_.genie_match_stats_workspace_bytes(n, total, L, 0)), dtype=torch.uint8, device="cuda")
        ws = torch.empty(int(L_.genie_find_mems_workspace_bytes(n, total, L, 0)), dtype=torch.uint8, device="cuda")
        tmp = torch.empty(int(L_.genie_locate_tmp_bytes(total)), dtype=torch.uint8, device="cuda")
        row_off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        pos_off = torch.empty(total + 1, dtype=torch.int64, device="cuda")
        totals = torch.empty(2, dtype=torch.int64, device="cuda")
        res = {"reference_bases": int(ref.size), "reads": n, "read_len": L,
               "workspace_bytes": {"find_mems": ws.numel(), "match_stats": ws_ms.numel(), "locate": tmp.numel()}}

        def match_stats():
            g._native.check(L_.genie_match_stats(ix._h, 0, _ptr(bases), _ptr(offs), n, total, L, _ptr(ms), _ptr(lohi), _ptr(st),
                                                 _ptr(ws_ms), ws_ms.numel(), sp), "genie_match_stats")

        masked = torch.empty_like(lohi)
        none = torch.full((1, 2), -1, dtype=torch.int32, device="cuda")

        for m in (19, 33):
            rows = None

            def mems(fill):
                g._native.check(L_.genie_find_mems(ix._h, 0, _ptr(bases), _ptr(offs), n, total, L, m, 0, _ptr(row_off),
                                                   _ptr(rows if fill else None), rows.shape[0] if fill else 0, _ptr(st), _ptr(totals),
                                                   _ptr(ws), ws.numel(), sp), "genie_find_mems")

            def locate(out, cap):
                # a caller's filter, in torch: only the intervals of matches of at least min_len bases are resolved
                torch.where((ms >= m).unsqueeze(1), lohi, none, out=masked)
                g._native.check(L_.genie_locate(ix._h, _ptr(masked), 2, total, _ptr(pos_off), _ptr(out), cap, _ptr(tmp), tmp.numel(), sp),
                                "genie_locate")

            match_stats()
            locate(None, 0)                                          # learns the yardstick's positions
            n_pos = int(pos_off[-1].item())
            positions = torch.empty(max(n_pos, 1), dtype=torch.int32, device="cuda")

            def yardstick():
                match_stats()
                locate(positions, n_pos)

            mems(False)                                              # learns the row total
            n_rows = int(totals[0].item())
            rows = torch.empty((max(n_rows, 1), 4), dtype=torch.int32, device="cuda")
            fns = (("stats", match_stats), ("sizing", lambda: mems(False)), ("mems", lambda: mems(True)), ("yardstick", yardstick))
            for _, fn in fns + fns:                                  # warm-up
                fn()
            torch.cuda.synchronize()
            assert int(row_off[-1].item()) == n_rows and not bool(st.any())
            at = torch.repeat_interleave(offs[:-1], row_off[1:] - row_off[:-1]) + rows[:n_rows, 0]
            length = rows[:n_rows, 1] - rows[:n_rows, 0]
            assert bool((length <= ms[at]).all()) and bool((length >= m).all())
            del at, length
            times = {k: [] for k, _ in fns}
            for _ in range(a.reps):
                for key, fn in fns:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    torch.cuda.synchronize()
                    times[key].append(e0.elapsed_time(e1) * 1e3)
            r = {"rows": n_rows, "yardstick_positions": n_pos}
            for key, _ in fns:
                r[key] = stats(times[key])
            r["seed_count_us"] = round(r["sizing"]["median"] - r["stats"]["median"], 1)
            r["fill_us"] = round(r["mems"]["median"] - r["sizing"]["median"], 1)
            r["ratio_to_yardstick"] = round(r["mems"]["median"] / r["yardstick"]["median"], 3)
            r["ns_per_base"] = round(r["mems"]["median"] * 1e3 / total, 4)
            res[f"min_len_{m}"] = r
            del rows, positions
        out[name] = res
        print(f"# {name}: {json.dumps(res)}", file=sys.stderr, flush=True)
        del bases, offs, ms, lohi, masked, st, ws_ms, ws, tmp, row_off, pos_off, totals
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
