"""Cost of genie_exact_match (intervals of CSR patterns, one lane per pattern) against its yardstick,
genie_sa_interval (one wave per pattern) on the same patterns padded to the batch's longest, on the same handle, in the same
run.  Patterns are cut from the 100 kb synthetic reference of BASELINE config 1, every second one with one base changed:
  em_1Mx10 .. em_1Mx500   10^6 patterns at each length of the reference's own grid, 10 / 50 / 100 / 200 / 500 bases
  em_1Mxmixed             10^6 patterns with lengths drawn uniformly from that grid (the yardstick pads them to 500)
  em_1kx100k              10^3 patterns of 10^5 bases, the new call only (the yardstick stops at 8192 bases)
The batches of at most 64 bases also time `exact_match_packed`: the same call with max_len = 65, which sends the same patterns
through the pack stage that longer patterns take (the A/B behind the in-lane packing of short patterns).
Per batch both calls run on preallocated buffers, timed with HIP events (torch.cuda.Event) around the whole call -- the new
call's one synchronisation included -- after warm-up runs, interleaved round by round.  Before timing, the yardstick's lohi is
compared with the new call's (exact).  Recorded: the median and the spread (min, max) of --reps repeats in us, patterns / s
from the medians, `ratio` = yardstick median / new median (above 1: the new call is faster) and `yardstick_spread_us` (max -
min of the yardstick's repeats), the margin to read a difference by.
One JSON line.
Usage: python tools/time_exact_match.py [--reps 20] [--scale 1.0] [--batches a,b] [--out profiles/exact_match_time.json]"""
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

GRID = (10, 50, 100, 200, 500)
DIRECT = 64                              # kEmDirect: up to this max_len every lane packs its own pattern (no pack stage)


def stats(t, digits=1):
    t = np.asarray(t)
    return {"median": round(float(np.median(t)), digits), "min": round(float(t.min()), digits), "max": round(float(t.max()), digits)}


def make_batch(ref, lens, seed):
    """Patterns of the given lengths (int64 tensor on ref's device) cut from `ref` at random starts, every second one with
    one base changed -> (bases uint8 [total], offsets int64 [N + 1]), made on the device a slice at a time."""
    dev = ref.device
    gen = torch.Generator(device=dev).manual_seed(seed)
    n, nref = lens.numel(), ref.numel()
    offs = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    offs[1:] = torch.cumsum(lens, 0)
    bases = torch.empty(int(offs[-1].item()), dtype=torch.uint8, device=dev)
    step = max(1, (1 << 27) // max(int(lens.max().item()), 1))

    def below(bound):                                                # uniform integers in [0, bound), bound >= 1
        r = (torch.rand(bound.numel(), generator=gen, device=dev, dtype=torch.float64) * bound.double()).long()
        return torch.minimum(r, bound - 1)

    for a in range(0, n, step):
        b = min(n, a + step)
        ln, first = lens[a:b], offs[a:b] - offs[a]
        pat = torch.repeat_interleave(torch.arange(b - a, device=dev), ln)
        pos = torch.arange(int(offs[b] - offs[a]), device=dev) - first[pat]
        chunk = ref[below(nref - ln + 1)[pat] + pos]
        hit = (torch.arange(a, b, device=dev) & 1) == 1              # every second pattern: one base changed
        at = (first + below(ln))[hit]
        chunk[at] = (chunk[at] + 1 + torch.randint(0, 3, (at.numel(),), generator=gen, device=dev).to(torch.uint8)) & 3
        bases[offs[a]:offs[b]] = chunk
    return bases, offs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the batch sizes (a quick look)")
    ap.add_argument("--batches", default="", help="comma-separated batch names (default: all)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L_ = g._native.lib()
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    codes = synth.synth_ref(100_000, 100_000)
    ix = g.GenieIndex.build(codes, 15).to("cuda")
    ref = torch.from_numpy(codes).cuda()
    n1m, n1k = max(1, int(1_000_000 * a.scale)), max(1, int(1_000 * a.scale))
    batches = [(f"em_1Mx{L}", n1m, (L,), True) for L in GRID] + [("em_1Mxmixed", n1m, GRID, True), ("em_1kx100k", n1k, (100_000,), False)]
    if a.batches:
        batches = [b for b in batches if b[0] in a.batches.split(",")]
    out = {"reps": a.reps, "scale": a.scale, "device": torch.cuda.get_device_name(0), "reference_bases": int(codes.size), "units": "us"}
    for seed, (name, n, grid, yardstick) in enumerate(batches):
        pick = torch.randint(0, len(grid), (n,), generator=torch.Generator().manual_seed(seed)).cuda()
        lens = torch.tensor(grid, dtype=torch.int64, device="cuda")[pick]
        bases, offs = make_batch(ref, lens, 100 + seed)
        total, max_len = bases.numel(), int(lens.max().item())
        lohi = torch.empty((n, 2), dtype=torch.int32, device="cuda")
        cnt = torch.empty(n, dtype=torch.int32, device="cuda")
        st = torch.empty(n, dtype=torch.int32, device="cuda")
        ws = torch.empty(int(L_.genie_exact_match_workspace_bytes(n, total, max_len, 0)), dtype=torch.uint8, device="cuda")

        def new_call(bound=max_len):
            rc = L_.genie_exact_match(ix._h, 0, _ptr(bases), _ptr(offs), n, total, bound, _ptr(lohi), _ptr(cnt), _ptr(st), _ptr(ws),
                                      ws.numel(), sp)
            g._native.check(rc, "genie_exact_match")

        fns = [("exact_match", new_call)]
        if max_len <= DIRECT:                                        # the same call made to go through the pack stage
            fns.append(("exact_match_packed", lambda: new_call(DIRECT + 1)))
        if yardstick:                                                # the same patterns padded to the batch's longest
            mat = torch.zeros((n, max_len), dtype=torch.uint8, device="cuda")
            col = torch.arange(total, device="cuda") - torch.repeat_interleave(offs[:-1], lens)
            mat[torch.repeat_interleave(torch.arange(n, device="cuda"), lens), col] = bases
            del col
            lens32 = lens.to(torch.int32)
            lohi_sa = torch.empty((n, 2), dtype=torch.int32, device="cuda")

            def sa_call():
                rc = L_.genie_sa_interval(ix._h, _ptr(mat), _ptr(lens32), n, max_len, max_len, _ptr(lohi_sa), sp)
                g._native.check(rc, "genie_sa_interval")

            fns.append(("sa_interval", sa_call))
        for _, fn in fns + fns:                                      # warm-up
            fn()
        torch.cuda.synchronize()
        assert not bool(st.any()) and torch.equal(cnt, torch.where(lohi[:, 0] >= 0, lohi[:, 1] - lohi[:, 0] + 1, 0))
        if yardstick:
            assert torch.equal(lohi, lohi_sa), name
        times = {k: [] for k, _ in fns}
        for _ in range(a.reps):
            for key, fn in fns:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                times[key].append(e0.elapsed_time(e1) * 1e3)
        res = {"patterns": n, "lengths": list(grid), "total_bases": total, "present": int((cnt > 0).sum().item()),
               "workspace_bytes": ws.numel()}
        for key, _ in fns:
            res[key] = stats(times[key])
            res[key]["patterns_per_s"] = round(n / (res[key]["median"] * 1e-6))
        if "exact_match_packed" in times:
            res["packed_over_direct"] = round(res["exact_match_packed"]["median"] / res["exact_match"]["median"], 2)
        if yardstick:
            res["ratio"] = round(res["sa_interval"]["median"] / res["exact_match"]["median"], 2)
            res["yardstick_spread_us"] = round(res["sa_interval"]["max"] - res["sa_interval"]["min"], 1)
            del mat, lens32, lohi_sa
        out[name] = res
        print(f"# {name}: {json.dumps(res)}", file=sys.stderr, flush=True)
        del bases, offs, lohi, cnt, st, ws, lens, pick
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
