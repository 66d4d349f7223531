"""Cost of BAM records on the device (genie_bam_records) next to the SAM text of the same batch
(genie_sam_text, section 28), taken in one run on section 28's two batches:
  pairs      SMEM.map_pairs on 5 x 10^5 FR pairs of 150-base reads from the 100 kb synthetic reference of BASELINE config 1 cut
             into 25 contigs (mate 1 of every tenth pair with a substitution at every 20th base), then its records
  long       10^3 reads of 10^4 bases as 500 pairs, one synthetic record each, 4000 ops a record (4= 1X throughout)
For each and for the tags NM | AS, with MD added, all five, and NM | AS without SEQ and QUAL: GenieIndex.bam_records and
GenieIndex.sam_text (each the sizing call plus the filling call, its allocations and its one host read included) and the bytes
of both; and a bare device-to-device copy of as many bytes as the BAM records have, the floor of any streaming write.  Device
times with HIP events after warm-up runs, interleaved round by round: the median and the spread (min, max) of --reps repeats in
us.  The records are checked once: decoded by tests/bam_util.py's decoder they are the text's lines.  For the pairs also
SMEM.write_bam against SMEM.write_sam into --dir, once each, by the wall clock, at level 1 and the thread count the job has.
One JSON line.
Usage: python tools/time_bam_records.py [--reps 10] [--scale 1.0] [--dir /tmp] [--out profiles/bam_records_time.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import genie_smem_amd as g  # noqa: E402
from genie_smem_amd import synth  # noqa: E402
from tools.time_rescue import timed  # noqa: E402
from tools.time_sam_text import TAG_SETS  # noqa: E402


def measure(ix, args, kwargs, contig_names, reps, check_lines=2000):
    """args, kwargs: what GenieIndex.bam_records and GenieIndex.sam_text take."""
    import bam_util as BU
    res = {}
    data, offsets, totals = ix.bam_records(*args, **dict(kwargs, tags=31))
    text, line_offsets, _ = ix.sam_text(*args, **dict(kwargs, tags=31))
    n = min(check_lines, int(totals[0]))                              # the decoder is plain Python: the first records
    lines = bytes(text[:int(line_offsets[n])].cpu().numpy()).decode("latin-1").split("\n")[:-1]
    if BU.bam_to_sam(data[:int(offsets[n])].cpu().numpy(), contig_names) != lines:
        raise SystemExit("the decoded records differ from the text")
    res.update(records=int(totals[0]), unmapped_records=int(totals[2]), checked_records=n)
    del text, line_offsets
    fns = []
    for key, tags, seq in TAG_SETS:
        fns.append(("bam_" + key, (lambda t=tags, s=seq: ix.bam_records(*args, **dict(kwargs, tags=t, seq=s)))))
        fns.append(("sam_" + key, (lambda t=tags, s=seq: ix.sam_text(*args, **dict(kwargs, tags=t, seq=s)))))
    data = ix.bam_records(*args, **dict(kwargs, tags=TAG_SETS[0][1]))[0]
    src, dst = torch.empty_like(data), torch.empty_like(data)
    fns.append(("copy_d2d_bam_nm_as", lambda: dst.copy_(src)))
    t = timed(fns, reps)
    for key, tags, seq in TAG_SETS:
        t["bam_" + key]["bytes"] = int(ix.bam_records(*args, **dict(kwargs, tags=tags, seq=seq))[2][1])
        t["sam_" + key]["bytes"] = int(ix.sam_text(*args, **dict(kwargs, tags=tags, seq=seq))[2][1])
        t["bam_" + key]["over_sam"] = round(t["bam_" + key]["median"] / t["sam_" + key]["median"], 3)
        t["bam_" + key]["bytes_over_sam"] = round(t["bam_" + key]["bytes"] / max(t["sam_" + key]["bytes"], 1), 3)
    t["bam_nm_as"]["over_copy_d2d"] = round(t["bam_nm_as"]["median"] / t["copy_d2d_bam_nm_as"]["median"], 2)
    res.update(t)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the batch sizes (a quick look)")
    ap.add_argument("--dir", default="/tmp", help="where write_bam and write_sam put their files (removed afterwards)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    out = {"reps": a.reps, "scale": a.scale, "device": torch.cuda.get_device_name(0), "units": "us",
           "threads": os.environ.get("OMP_NUM_THREADS", "")}
    ref = synth.synth_ref(100_000, 100_000)
    n_contigs = 25
    rs = g.ReferenceSet([f"contig{i}" for i in range(n_contigs)], np.linspace(0, ref.size, n_contigs + 1).astype(np.int64), ref)
    rng = np.random.default_rng(28)
    m = g.ExactMatch("time_bam_records.fa")
    m.set_reference("".join("ACGT"[c] for c in ref))
    sm = g.SMEM(m, 4)
    ix = sm.matcher.index(sm.lut.lut_size)
    cn = g.names_csr(rs.names, "cuda")

    # ---- 150-base pairs through map_pairs: tools/time_sam_text.py's batch
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
    nm = g.names_csr([f"pair{r // 2}" for r in range(2 * pairs_n)], "cuda")
    quals = torch.from_numpy(rng.integers(33, 74, 2 * pairs_n * L).astype(np.uint8)).cuda()
    result = sm.map_pairs(batch, 19, rs)
    records, sel_offsets, offs, cigar, info, _, sam = result
    args = (batch[0], batch[1], sel_offsets, records, sam, info, offs, cigar, *nm, *cn)
    res = measure(ix, args, dict(quals=quals, contigs=rs), rs.names, a.reps)
    res.update(pairs=pairs_n, read_len=L, ops=int(cigar.numel()))
    # the files, once each by the wall clock: level 1, the job's threads
    files = {}
    for key, write, name in (("write_bam", sm.write_bam, "time_bam_records.bam"), ("write_sam", sm.write_sam, "time_bam_records.sam")):
        path = os.path.join(a.dir, name)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        write(path, result, batch, nm, quals=quals, contigs=rs)
        files[key] = {"wall_us": round((time.perf_counter() - t0) * 1e6, 1), "file_bytes": os.path.getsize(path)}
        os.remove(path)
    res.update(files)
    out["pairs"] = res
    print(f"# pairs: {json.dumps(res)}", file=sys.stderr, flush=True)
    del result, records, sam, info, offs, cigar, args, batch, quals
    torch.cuda.empty_cache()

    # ---- 10^4-base reads with 4000 ops each: synthetic records
    L, n = 10_000, max(2, int(1000 * a.scale)) & ~1
    where = rng.integers(0, ref.size - L, n)                         # counted from the start of contig 0: only the letters matter here
    bases = torch.from_numpy(rng.integers(0, 4, n * L).astype(np.uint8)).cuda()
    read_offsets = torch.from_numpy((np.arange(n + 1) * L).astype(np.int64)).cuda()
    quals = torch.from_numpy(rng.integers(33, 74, n * L).astype(np.uint8)).cuda()
    span = L
    ops = np.tile(np.asarray([(4 << 4) | 7, (1 << 4) | 8], np.uint32), span // 5)
    rec = np.zeros((n, 12), np.int32)
    rec[:, 0], rec[:, 1], rec[:, 3], rec[:, 5], rec[:, 6] = np.arange(n), np.arange(n), np.arange(n) % 2, where + 1, span
    rec[:, 8], rec[:, 9], rec[:, 11] = span, span // 2, 60
    samrows = np.stack([np.where(np.arange(n) % 2, 147, 99), np.full(n, 60), np.arange(n) ^ 1, np.zeros(n)], 1).astype(np.int32)
    inf = np.zeros((n, 8), np.int32)
    inf[:, 3] = span // 5
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()      # noqa: E731
    args = (bases, read_offsets, dev(np.arange(n + 1, dtype=np.int64)), dev(rec), dev(samrows), dev(inf),
            dev(np.arange(n + 1, dtype=np.int64) * ops.size), dev(np.tile(ops, n).view(np.int32)),
            *g.names_csr([f"long{r // 2}" for r in range(n)], "cuda"), *cn)
    res = measure(ix, args, dict(quals=quals, contigs=rs), rs.names, a.reps, check_lines=20)
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
