"""Cost of SAM text on the device (genie_sam_text), taken in one run:
  pairs      SMEM.map_pairs on 5 x 10^5 FR pairs of 150-base reads from the 100 kb synthetic reference of BASELINE config 1 cut
             into 25 contigs (mate 1 of every tenth pair with a substitution at every 20th base, so X ops and MD letters occur),
             then the text of its records
  long       10^3 reads of 10^4 bases as 500 pairs, one record each, 4000 ops a record (4= 1X throughout): synthetic records,
             since the call takes any
For each: GenieIndex.sam_text (the sizing call plus the filling call, its allocations and its one host read included) with the
tags NM | AS, with MD added, with all five, and without SEQ and QUAL; next to (a) sam_lines on the same results, copies to the
host included -- the only way to the text before this call -- and (b) a bare device-to-device copy of as many bytes as the text
has, the floor of any streaming write.  For the pairs also a whole map_pairs, to say what share the text is of it.  Device
times with HIP events (torch.cuda.Event) after warm-up runs, interleaved round by round: the median and the spread (min, max) of
--reps repeats in us; sam_lines once, by the wall clock.  The text is checked once against sam_lines, byte for byte.
One JSON line.
Usage: python tools/time_sam_text.py [--reps 10] [--scale 1.0] [--out profiles/sam_text_time.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import genie_smem_amd as g  # noqa: E402
from genie_smem_amd import synth  # noqa: E402
from tools.time_rescue import timed  # noqa: E402

N_ = g._native
TAG_SETS = (("nm_as", N_.SAM_NM | N_.SAM_AS, True), ("nm_as_md", N_.SAM_NM | N_.SAM_AS | N_.SAM_MD, True), ("all_tags", 31, True),
            ("nm_as_no_seq", N_.SAM_NM | N_.SAM_AS, False))


def measure(ix, args, kwargs, lines_of, reps, check=True):
    """args, kwargs: what GenieIndex.sam_text takes.  lines_of: () -> sam_lines' list for the same results."""
    res = {}
    text, line_offsets, totals = ix.sam_text(*args, **kwargs)
    t0 = time.perf_counter()
    want = lines_of()
    res["sam_lines_wall_us"] = round((time.perf_counter() - t0) * 1e6, 1)
    if check and bytes(text.cpu().numpy()) != ("\n".join(want) + "\n").encode():
        raise SystemExit("the text differs from sam_lines")
    del want
    res.update(lines=int(totals[0]), bytes=int(totals[1]), unmapped_lines=int(totals[2]))
    fns = [(key, (lambda t=tags, s=seq: ix.sam_text(*args, **dict(kwargs, tags=t, seq=s)))) for key, tags, seq in TAG_SETS]
    src, dst = torch.empty_like(text), torch.empty_like(text)
    fns.append(("copy_d2d", lambda: dst.copy_(src)))
    t = timed(fns, reps)
    for key, tags, seq in TAG_SETS:
        t[key]["bytes"] = int(ix.sam_text(*args, **dict(kwargs, tags=tags, seq=seq))[2][1])
    res.update(t)
    res["nm_as"]["sam_lines_over_it"] = round(res["sam_lines_wall_us"] / t["nm_as"]["median"], 1)
    res["nm_as"]["over_copy_d2d"] = round(t["nm_as"]["median"] / t["copy_d2d"]["median"], 2)
    res["nm_as"]["us_per_line"] = round(t["nm_as"]["median"] / max(res["lines"], 1), 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the batch sizes (a quick look)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    out = {"reps": a.reps, "scale": a.scale, "device": torch.cuda.get_device_name(0), "units": "us"}
    ref = synth.synth_ref(100_000, 100_000)
    n_contigs = 25
    rs = g.ReferenceSet([f"contig{i}" for i in range(n_contigs)], np.linspace(0, ref.size, n_contigs + 1).astype(np.int64), ref)
    rng = np.random.default_rng(28)
    m = g.ExactMatch("time_sam_text.fa")
    m.set_reference("".join("ACGT"[c] for c in ref))
    sm = g.SMEM(m, 4)
    ix = sm.matcher.index(sm.lut.lut_size)
    cn = g.names_csr(rs.names, "cuda")

    # ---- 150-base pairs through map_pairs
    L, pairs_n = 150, max(50, int(500_000 * a.scale))
    contig_len = ref.size // n_contigs
    inside = rng.integers(0, contig_len - 400, pairs_n) + rng.integers(0, n_contigs, pairs_n) * contig_len
    mate0 = ref[inside[:, None] + np.arange(L)[None, :]].copy()
    fwd = ref[(inside + 400 - L)[:, None] + np.arange(L)[None, :]].copy()
    hit = np.arange(pairs_n) % 10 == 0
    fwd[np.ix_(hit, np.arange(19, L, 20))] = (fwd[np.ix_(hit, np.arange(19, L, 20))] + 1) % 4
    both = np.empty((2 * pairs_n, L), np.uint8)
    both[0::2], both[1::2] = mate0, 3 - fwd[:, ::-1]
    batch = (torch.from_numpy(both.reshape(-1)).cuda(), torch.from_numpy((np.arange(2 * pairs_n + 1) * L).astype(np.int64)).cuda())
    names = [f"pair{r // 2}" for r in range(2 * pairs_n)]
    nm = g.names_csr(names, "cuda")
    quals = torch.from_numpy(rng.integers(33, 74, 2 * pairs_n * L).astype(np.uint8)).cuda()
    result = sm.map_pairs(batch, 19, rs)
    records, sel_offsets, offs, cigar, info, _, sam = result
    args = (batch[0], batch[1], sel_offsets, records, sam, info, offs, cigar, *nm, *cn)

    def lines_of():
        letters = np.frombuffer(b"ACGT", np.uint8)[both]
        seqs = [bytes(row).decode() for row in letters]
        q = quals.cpu().numpy().reshape(-1, L)
        return g.sam_lines(records, sam, info, offs, cigar, names, rs.names, seqs, [bytes(row).decode() for row in q])

    res = measure(ix, args, dict(quals=quals, contigs=rs), lines_of, a.reps)
    whole = timed([("map_pairs", lambda: sm.map_pairs(batch, 19, rs))], max(3, a.reps // 2))
    res["map_pairs"] = whole["map_pairs"]
    res["nm_as"]["share_of_map_pairs_plus_text"] = round(res["nm_as"]["median"] / (res["nm_as"]["median"] + whole["map_pairs"]["median"]), 3)
    res.update(pairs=pairs_n, read_len=L, records=int(records.shape[0]), ops=int(cigar.numel()))
    out["pairs"] = res
    print(f"# pairs: {json.dumps(res)}", file=sys.stderr, flush=True)
    del result, records, sam, info, offs, cigar, args, batch, quals
    torch.cuda.empty_cache()

    # ---- 10^4-base reads with 4000 ops each: synthetic records
    L, n = 10_000, max(2, int(1000 * a.scale)) & ~1
    where = rng.integers(0, ref.size - L, n)                         # counted from the start of contig 0: only the letters matter here
    ctg = np.zeros(n, np.int64)
    bases = torch.from_numpy(rng.integers(0, 4, n * L).astype(np.uint8)).cuda()
    read_offsets = torch.from_numpy((np.arange(n + 1) * L).astype(np.int64)).cuda()
    quals = torch.from_numpy(rng.integers(33, 74, n * L).astype(np.uint8)).cuda()
    span = L
    ops = np.tile(np.asarray([(4 << 4) | 7, (1 << 4) | 8], np.uint32), span // 5)
    rec = np.zeros((n, 12), np.int32)
    rec[:, 0], rec[:, 1], rec[:, 3], rec[:, 4], rec[:, 5], rec[:, 6] = np.arange(n), np.arange(n), np.arange(n) % 2, ctg, where + 1, span
    rec[:, 8], rec[:, 9], rec[:, 11] = span, span // 2, 60
    samrows = np.stack([np.where(np.arange(n) % 2, 147, 99), np.full(n, 60), np.arange(n) ^ 1, np.zeros(n)], 1).astype(np.int32)
    inf = np.zeros((n, 8), np.int32)
    inf[:, 3] = span // 5
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()      # noqa: E731
    t_rec, t_sam, t_info = dev(rec), dev(samrows), dev(inf)
    t_so, t_co = dev(np.arange(n + 1, dtype=np.int64)), dev(np.arange(n + 1, dtype=np.int64) * ops.size)
    t_cigar = dev(np.tile(ops, n).view(np.int32))
    lnames = [f"long{r // 2}" for r in range(n)]
    args = (bases, read_offsets, t_so, t_rec, t_sam, t_info, t_co, t_cigar, *g.names_csr(lnames, "cuda"), *cn)

    def long_lines():
        letters = np.frombuffer(b"ACGT", np.uint8)[bases.cpu().numpy().reshape(-1, L)]
        q = quals.cpu().numpy().reshape(-1, L)
        return g.sam_lines(t_rec, t_sam, t_info, t_co, t_cigar, lnames, rs.names, [bytes(r).decode() for r in letters],
                           [bytes(r).decode() for r in q])

    res = measure(ix, args, dict(quals=quals, contigs=rs), long_lines, a.reps)
    res.update(reads=n, read_len=L, ops_per_record=int(ops.size))
    out["long"] = res
    print(f"# long: {json.dumps(res)}", file=sys.stderr, flush=True)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
