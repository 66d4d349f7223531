"""Cost of mate rescue, taken in one run on the 100 kb synthetic reference of BASELINE config 1 cut into
25 equal contigs:
  window_mems   genie_window_mems (min_len 12, no input rows, every output) next to genie_find_mems_contigs (min_len 19), the
                seeding it complements, on the same 150-base reads: each read a piece of the reference with a substitution at
                every 13th base, its window the 1000 bases around where it came from, with 1 %, 10 % and 100 % of the units
                searched (the others have no window)
  map_pairs     SMEM.map_pairs(rescue=True) next to rescue=False on an interleaved batch of FR pairs 400 bases end to end, mate 1
                of every tenth pair diverged in the same way
Calls with their synchronisations included, timed with HIP events (torch.cuda.Event) after warm-up runs and interleaved round by
round: the median and the spread (min, max) of --reps repeats in us, and the ratio of the medians.  The results are checked once:
every searched unit has the eleven 12-base rows of its read at least, and rescue makes every diverged pair proper.  One JSON line.
Usage: python tools/time_rescue.py [--reps 10] [--scale 1.0] [--out profiles/rescue_time.json]"""
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
from tools.time_mems import stats  # noqa: E402

L, EVERY, WINDOW, MIN_LEN, SEED_LEN = 150, 13, 1000, 12, 19


def pieces(ref, starts, diverged):
    """The L-base pieces of ref at `starts`; those marked get a substitution at every 13th base."""
    reads = ref[starts[:, None] + np.arange(L)[None, :]].copy()
    at = np.arange(EVERY - 1, L, EVERY)
    sub = reads[:, at]
    reads[:, at] = np.where(diverged[:, None], (sub + 1) % 4, sub)
    return reads


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
    out = {"reps": a.reps, "scale": a.scale, "device": torch.cuda.get_device_name(0), "units": "us", "read_len": L, "window": WINDOW,
           "min_len": MIN_LEN, "find_mems_min_len": SEED_LEN, "window_max_rows": g._native.WINDOW_MAX_ROWS}
    ref = synth.synth_ref(100_000, 100_000)
    n_contigs = 25
    rs = g.ReferenceSet([str(i) for i in range(n_contigs)], np.linspace(0, ref.size, n_contigs + 1).astype(np.int64), ref)
    rng = np.random.default_rng(27)

    # ---- genie_window_mems next to genie_find_mems_contigs
    ix = g.GenieIndex.build(ref, 0).to("cuda")
    table = torch.from_numpy(rs.offsets).cuda()
    n = max(100, int(200_000 * a.scale))
    starts = rng.integers(0, ref.size - L, n)
    reads = pieces(ref, starts, np.ones(n, bool))
    bases = torch.from_numpy(reads.reshape(-1)).cuda()
    offs = torch.from_numpy((np.arange(n + 1) * L).astype(np.int64)).cuda()
    total = n * L
    ws_f = torch.empty(max(256, int(L_.genie_find_mems_contigs_workspace_bytes(n, total, L, 0, n_contigs))), dtype=torch.uint8, device="cuda")
    ws_w = torch.empty(max(256, int(L_.genie_window_mems_workspace_bytes(n))), dtype=torch.uint8, device="cuda")
    f_off, w_off = (torch.empty(n + 1, dtype=torch.int64, device="cuda") for _ in range(2))
    f_st, w_st = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(2))
    f_tt, w_tt = torch.empty(2, dtype=torch.int64, device="cuda"), torch.empty(3, dtype=torch.int64, device="cuda")
    cap = 16 * n
    f_rows, w_rows = (torch.empty((cap, 4), dtype=torch.int32, device="cuda") for _ in range(2))
    none = C.c_void_p(0)

    def find_mems():
        g._native.check(L_.genie_find_mems_contigs(ix._h, _ptr(table), n_contigs, 0, _ptr(bases), _ptr(offs), n, total, L, SEED_LEN, 0,
                                                   _ptr(f_off), _ptr(f_rows), cap, _ptr(f_st), _ptr(f_tt), _ptr(ws_f), ws_f.numel(), sp),
                        "genie_find_mems_contigs")

    res = {"reads": n, "reference_bases": int(ref.size), "contigs": n_contigs, "workspace_bytes": ws_w.numel()}
    for share in (0.01, 0.1, 1.0):
        searched = rng.random(n) < share if share < 1 else np.ones(n, bool)
        wb = np.clip(starts - (WINDOW - L) // 2, 0, ref.size - WINDOW)
        win = np.where(searched[:, None], np.stack([wb, wb + WINDOW], axis=1), 0).astype(np.int32)
        windows = torch.from_numpy(win).cuda()

        def window_mems():
            g._native.check(L_.genie_window_mems(ix._h, 0, _ptr(bases), _ptr(offs), n, total, L, n, _ptr(windows), MIN_LEN, none, none, 0,
                                                 _ptr(w_off), _ptr(w_rows), cap, _ptr(w_st), _ptr(w_tt), _ptr(ws_w), ws_w.numel(), sp),
                            "genie_window_mems")

        window_mems()
        torch.cuda.synchronize()
        per = (w_off[1:] - w_off[:-1]).cpu().numpy()
        if int(w_tt[2]) or (per[searched] < L // EVERY).any() or per[~searched].any() or int(w_tt[0]) > cap:
            raise SystemExit(f"window_mems {share}: a searched unit lacks its rows, or an unsearched one has rows")
        t = timed((("find_mems_contigs", find_mems), ("window_mems", window_mems)), a.reps)
        t["units_searched"] = int(searched.sum())
        t["rows"] = int(w_tt[0])
        t["find_mems_rows"] = int(f_tt[0])
        t["window_mems"]["ratio_to_find_mems_contigs"] = round(t["window_mems"]["median"] / t["find_mems_contigs"]["median"], 3)
        t["window_mems"]["us_per_searched_unit"] = round(t["window_mems"]["median"] / max(1, int(searched.sum())), 4)
        res[f"searched_{share:g}"] = t
        print(f"# window_mems {share:g}: {json.dumps(t)}", file=sys.stderr, flush=True)
    out["window_mems"] = res
    del bases, offs, f_rows, w_rows, ws_f, ws_w
    torch.cuda.empty_cache()

    # ---- SMEM.map_pairs with and without rescue
    m = g.ExactMatch("time_rescue.fa")
    m.set_reference("".join("ACGT"[c] for c in ref))
    sm = g.SMEM(m, 4)
    pairs_n = max(50, int(50_000 * a.scale))
    contig_len = ref.size // n_contigs
    inside = rng.integers(0, contig_len - 400, pairs_n) + rng.integers(0, n_contigs, pairs_n) * contig_len
    diverged = np.arange(pairs_n) % 10 == 0
    mate0 = pieces(ref, inside, np.zeros(pairs_n, bool))
    mate1 = 3 - pieces(ref, inside + 400 - L, diverged)[:, ::-1]      # the reverse complement: FR
    both = np.empty((2 * pairs_n, L), np.uint8)
    both[0::2], both[1::2] = mate0, mate1
    batch = (torch.from_numpy(both.reshape(-1)).cuda(), torch.from_numpy((np.arange(2 * pairs_n + 1) * L).astype(np.int64)).cuda())
    plain = sm.map_pairs(batch, SEED_LEN, rs)
    rescued = sm.map_pairs(batch, SEED_LEN, rs, rescue=True)
    proper0, proper1 = ((r[5][:, 2] & 1).cpu().numpy().astype(bool) for r in (plain, rescued))
    if proper0[diverged].any() or not proper1[diverged].all() or not proper1[~diverged].all():
        raise SystemExit(f"map_pairs: {int(proper0[diverged].sum())} diverged pairs proper without rescue, "
                         f"{int(proper1[diverged].sum())} of {int(diverged.sum())} with it")
    t = timed((("rescue_false", lambda: sm.map_pairs(batch, SEED_LEN, rs)), ("rescue_true", lambda: sm.map_pairs(batch, SEED_LEN, rs, rescue=True))),
              a.reps)
    t.update(pairs=pairs_n, diverged_pairs=int(diverged.sum()), proper_without=int(proper0.sum()), proper_with=int(proper1.sum()),
             window_totals=[int(v) for v in rescued[7][2].tolist()])
    t["rescue_true"]["ratio_to_rescue_false"] = round(t["rescue_true"]["median"] / t["rescue_false"]["median"], 3)
    out["map_pairs"] = t
    print(f"# map_pairs: {json.dumps(t)}", file=sys.stderr, flush=True)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
