"""Cost of the segment calls against their yardsticks.
  (a) squeeze   genie_reference_segments (the filling call on preallocated buffers, its one synchronisation included) on
                --given bytes (default 10^8) of random bases with breaks at density 1/5000 and 1/50, with a NULL table, 25
                records and 10^5 records (what resolving the boundaries costs), against genie_reads_from_fasta on a FASTA
                text of the same size (25 records wrapped at 60 columns, the same break density): the same three-pass
                compaction shape.  ns per input byte and the ratio of the two; 1.5 is the bound the squeeze should keep.
  (b) coords    genie_segment_coords on 4 * 10^6 MEM positions (stride 4 on the rows) against genie_contig_coords on the same
                positions with the same table: the same lookup, two gathers and 16-byte instead of 8-byte stores on top.
  (c) mems      genie_find_mems_contigs with a segment table: the 100 kb synthetic reference of BASELINE config 1 as the
                squeezed concatenation of a given reference with 225 N runs (the lengths of the end-to-end test, cycled) in 3
                records, 10^6 x 150-base reads, min_len 19 -- next to genie_find_mems on the same batch.
Every time: HIP events (torch.cuda.Event) after warm-up runs, the calls interleaved round by round; the median and the
spread (min, max) of --reps repeats in us.  One JSON line.
Usage: python tools/time_segments.py [--reps 10] [--given 100000000] [--scale 1.0] [--out profiles/segments_time.json]"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import genie_smem_amd as g  # noqa: E402
from genie_smem_amd import synth  # noqa: E402
from genie_smem_amd.contigs import cut_segments  # noqa: E402
from genie_smem_amd.index import _ptr  # noqa: E402
from time_mems_contigs import timed  # noqa: E402

N_RUNS = (1, 400, 2, 350, 37, 300, 150, 400, 260)


def fasta_text(nbytes, records, density, rng):
    """A FASTA text of exactly nbytes: `records` records, an 8-byte header line each, the sequence wrapped at 60 columns."""
    per = nbytes // records
    out = np.empty(nbytes, np.uint8)
    at = 0
    for r in range(records):
        size = per if r < records - 1 else nbytes - at
        rec = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size)]
        rec[rng.random(size) < density] = ord("N")
        rec[8 + 60::61] = 0x0A
        rec[:8] = np.frombuffer(b">rec%03d\n" % r, np.uint8)
        rec[-1] = 0x0A
        out[at:at + size] = rec
        at += size
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--given", type=int, default=100_000_000)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the read batch of (b) and (c) (a quick look)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L_ = g._native.lib()
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = {"reps": a.reps, "given_bytes": a.given, "scale": a.scale, "device": torch.cuda.get_device_name(0), "units": "us"}
    rng = np.random.default_rng(20)
    n = a.given
    table = np.full(256, 4, np.uint8)
    for i, ch in enumerate(b"ACGT"):
        table[ch] = i
    tab = table.ctypes.data_as(C.c_void_p)

    # ------------------------------------------------------------------ (a)
    for density in (1 / 5000, 1 / 50):
        codes = torch.randint(0, 4, (n,), dtype=torch.uint8, device="cuda")
        codes[torch.rand(n, device="cuda") < density] = 4
        text = torch.from_numpy(fasta_text(n, 25, density, rng)).cuda()
        tables = {"null": None}
        for records in (25, 100_000):
            cuts = np.sort(rng.integers(0, n + 1, records - 1))
            tables[str(records)] = torch.from_numpy(np.concatenate([[0], cuts, [n]]).astype(np.int64)).cuda()
        tmp = torch.empty(int(max(L_.genie_reference_segments_tmp_bytes(n, 100_000), L_.genie_reads_from_fasta_tmp_bytes(n, 25))),
                          dtype=torch.uint8, device="cuda")
        out4, out5 = (C.c_int64 * 4)(), (C.c_int64 * 5)()
        bases = torch.empty(n, dtype=torch.uint8, device="cuda")
        sizes, bufs = {}, {}

        def squeeze(key, fill=True):
            t = tables[key]
            so, sr, sg = bufs[key] if fill else (None, None, None)
            rc = L_.genie_reference_segments(_ptr(codes), n, _ptr(t), 1 if t is None else t.numel() - 1, _ptr(bases) if fill else None,
                                             n, _ptr(so), _ptr(sr), _ptr(sg), sizes[key][0] if fill else 0, out4, _ptr(tmp), tmp.numel(), sp)
            g._native.check(rc, "genie_reference_segments")

        for key in tables:
            squeeze(key, False)
            sizes[key] = list(out4)
            S = sizes[key][0]
            bufs[key] = (torch.empty(S + 1, dtype=torch.int64, device="cuda"), torch.empty(max(S, 1), dtype=torch.int32, device="cuda"),
                         torch.empty(max(S, 1), dtype=torch.int64, device="cuda"))
        offs, starts = torch.empty(26, dtype=torch.int64, device="cuda"), torch.empty(25, dtype=torch.int64, device="cuda")

        def fasta():
            rc = L_.genie_reads_from_fasta(_ptr(text), n, 0, tab, _ptr(bases), n, _ptr(offs), _ptr(starts), 25, out5, _ptr(tmp), tmp.numel(), sp)
            g._native.check(rc, "genie_reads_from_fasta")

        fns = (("reads_from_fasta", fasta),) + tuple((f"segments_{k}", lambda k=k: squeeze(k)) for k in tables)
        r = timed(fns, a.reps)
        for k in r:
            r[k]["ns_per_input_byte"] = round(r[k]["median"] * 1e3 / n, 5)
        r["segments"] = {k: {"n_seg": v[0], "n_kept": v[1], "longest": v[2]} for k, v in sizes.items()}
        r["ratio_to_reads_from_fasta"] = {k: round(r[f"segments_{k}"]["median"] / r["reads_from_fasta"]["median"], 3) for k in tables}
        out[f"squeeze_density_1_in_{round(1 / density)}"] = r
        print(f"# squeeze {density}: {json.dumps(r)}", file=sys.stderr, flush=True)
        del codes, text, tables, tmp, bases, bufs
        torch.cuda.empty_cache()

    # ------------------------------------------------------------------ (b), (c)
    ref = synth.synth_ref(100_000, 100_000)
    cut_at = np.sort(rng.choice(np.arange(1, ref.size), 225, replace=False))
    parts, prev = [], 0
    for k, c in enumerate(cut_at.tolist()):
        parts += [ref[prev:c], np.full(N_RUNS[k % len(N_RUNS)], 4, np.uint8)]
        prev = c
    given = np.concatenate(parts + [ref[prev:]])
    rec_off = np.asarray([0, given.size // 3, 2 * given.size // 3, given.size], np.int64)
    kept, so, sr, sg = cut_segments(given, rec_off)
    assert np.array_equal(kept, ref)
    d = g.reference_segments(given, rec_off)
    assert all(np.array_equal(x.cpu().numpy(), y) for x, y in zip(d[:4], (kept, so, sr, sg)))
    seg_off, seg_rec, seg_org = d[1], d[2], d[3]
    S = seg_rec.numel()
    ix = g.GenieIndex.build(ref, 15).to("cuda")
    g._native.check(L_.genie_contigs_validate(ix._h, _ptr(seg_off), S, sp), "genie_contigs_validate")
    reads = synth.reads_from_ref_fast(ref, max(1, int(1_000_000 * a.scale)), 150, 1)
    nr, L = reads.shape
    total = nr * L
    bases = torch.from_numpy(reads.reshape(-1)).cuda()
    offs = torch.arange(nr + 1, dtype=torch.int64, device="cuda") * L
    st = torch.empty(nr, dtype=torch.int32, device="cuda")
    ws = torch.empty(int(L_.genie_find_mems_contigs_workspace_bytes(nr, total, L, 0, S)), dtype=torch.uint8, device="cuda")
    row_off = torch.empty(nr + 1, dtype=torch.int64, device="cuda")
    totals = torch.empty(2, dtype=torch.int64, device="cuda")
    m = 19

    def mems(rows):
        g._native.check(L_.genie_find_mems(ix._h, 0, _ptr(bases), _ptr(offs), nr, total, L, m, 0, _ptr(row_off), _ptr(rows),
                                           rows.shape[0] if rows is not None else 0, _ptr(st), _ptr(totals), _ptr(ws), ws.numel(), sp),
                        "genie_find_mems")

    def contigs(rows):
        g._native.check(L_.genie_find_mems_contigs(ix._h, _ptr(seg_off), S, 0, _ptr(bases), _ptr(offs), nr, total, L, m, 0, _ptr(row_off),
                                                   _ptr(rows), rows.shape[0] if rows is not None else 0, _ptr(st), _ptr(totals), _ptr(ws),
                                                   ws.numel(), sp), "genie_find_mems_contigs")

    rows = {}
    for key, fn in (("mems", mems), ("segments", contigs)):
        fn(None)
        rows[key] = torch.empty((max(int(totals[0].item()), 1), 4), dtype=torch.int32, device="cuda")
    r = {"given_bases": int(given.size), "reference_bases": int(ref.size), "records": 3, "segments": S, "reads": nr, "read_len": L,
         "min_len": m, "rows": {k: v.shape[0] for k, v in rows.items()}}
    r.update(timed((("find_mems", lambda: mems(rows["mems"])), ("find_mems_contigs_segments", lambda: contigs(rows["segments"]))), a.reps))
    r["ratio_to_find_mems"] = round(r["find_mems_contigs_segments"]["median"] / r["find_mems"]["median"], 3)
    out["mems_cfg1_1Mx150"] = r
    print(f"# mems: {json.dumps(r)}", file=sys.stderr, flush=True)

    contigs(rows["segments"])
    count = max(1, int(4_000_000 * a.scale))
    pos = rows["segments"].repeat((count + rows["segments"].shape[0] - 1) // rows["segments"].shape[0], 1)[:count].contiguous()
    out32 = torch.empty((count, 2), dtype=torch.int32, device="cuda")
    out64 = torch.empty((count, 2), dtype=torch.int64, device="cuda")
    p2 = C.c_void_p(pos.data_ptr() + 8)                              # the pos column of the rows

    def contig_coords():
        g._native.check(L_.genie_contig_coords(ix._h, _ptr(seg_off), S, p2, 4, count, _ptr(out32), sp), "genie_contig_coords")

    def segment_coords():
        g._native.check(L_.genie_segment_coords(ix._h, _ptr(seg_off), _ptr(seg_rec), _ptr(seg_org), S, g._native.SEG_POSITIONS, p2, 4, count,
                                                _ptr(out64), sp), "genie_segment_coords")

    r = {"positions": count, "segments": S}
    r.update(timed((("contig_coords", contig_coords), ("segment_coords", segment_coords)), a.reps))
    r["ratio_to_contig_coords"] = round(r["segment_coords"]["median"] / r["contig_coords"]["median"], 3)
    # the two agree: the segment and the offset inside it name the same given position
    c32 = out32.cpu().numpy().astype(np.int64)
    assert np.array_equal(out64.cpu().numpy(), np.stack([sr[c32[:, 0]], sg[c32[:, 0]] + c32[:, 1]], 1))
    out["coords_4M"] = r
    print(f"# coords: {json.dumps(r)}", file=sys.stderr, flush=True)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
