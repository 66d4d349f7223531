"""Cost of reading a FASTA batch on the device (genie_reads_from_fasta) against the yardstick it has to meet per text byte:
genie_reads_from_text(GENIE_TEXT_LINES) on the same bases, one read per line.  Reads drawn from the 100 kb synthetic
reference (create_query_from_ref distribution):
  fasta_1kx100k_w60   10^3 x 10^5-base reads, a 32-byte header line each, the sequence wrapped at 60 columns
  fasta_1Mx150        10^6 x 150-base reads as two-line FASTA (the same header line, the sequence on one line)
Per batch:
  (a) ingest   genie_reads_from_fasta (the full call on preallocated buffers, record starts included; its one
               synchronisation included) and genie_reads_from_text on the one-per-line text, timed with HIP events
               (torch.cuda.Event) after warm-up runs and interleaved round by round: the median and the spread of --reps
               repeats in us, and ns per text byte.  `slower_per_byte_us` is what FASTA takes beyond the yardstick's time per
               byte on its own text; `yardstick_spread_us` (max - min of the yardstick's repeats) is the margin to read it by.
  (b) wall     (first batch) SMEM.find_smems_text(bytes, "fasta"), upload included, against SMEM.find_smems_long(list of the
               same strings, split_breaks=True): host wall-clock, device idle before and after, in ms.
One JSON line.
Usage: python tools/time_fasta_reads.py [--reps 20] [--list-reps 5] [--scale 1.0] [--out profiles/fasta_reads_time.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import genie_smem_amd as g  # noqa: E402
from genie_smem_amd import synth  # noqa: E402
from genie_smem_amd.index import _ptr  # noqa: E402

HEADER = b">SIM:1:FCX:1:1101:0000000:00000\n"
assert len(HEADER) == 32


def as_lines(ascii_reads):
    n, L = ascii_reads.shape
    out = np.full((n, L + 1), 0x0A, np.uint8)
    out[:, :L] = ascii_reads
    return out.tobytes()


def as_fasta(ascii_reads, width):
    """Every read: HEADER, then its bases in lines of `width` columns (the last one shorter)."""
    n, L = ascii_reads.shape
    nlines = (L + width - 1) // width
    grid = np.full((n, nlines, width + 1), 0x0A, np.uint8)
    padded = np.zeros((n, nlines * width), np.uint8)
    padded[:, :L] = ascii_reads
    grid[:, :, :width] = padded.reshape(n, nlines, width)
    flat = grid.reshape(n, nlines * (width + 1))
    keep = np.ones(nlines * (width + 1), bool)
    keep[(nlines - 1) * (width + 1) + L - (nlines - 1) * width:-1] = False       # the padding of the last line
    rec = np.empty((n, 32 + int(keep.sum())), np.uint8)
    rec[:, :32] = np.frombuffer(HEADER, np.uint8)
    rec[:, 32:] = flat[:, keep]
    return rec.tobytes()


def stats(t, digits=1):
    t = np.asarray(t)
    return {"median": round(float(np.median(t)), digits), "min": round(float(t.min()), digits), "max": round(float(t.max()), digits)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--list-reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the batch sizes (a quick look)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L_ = g._native.lib()
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    codes = synth.synth_ref(100_000, 100_000)
    ref = "".join("ACGT"[c] for c in codes)
    m = g.ExactMatch("REF_100K.fa")
    m.set_reference(ref)
    sm = g.SMEM(m, 15)
    table = m.byte_codes()
    tab = table.ctypes.data_as(C.c_void_p)
    letters = np.frombuffer(b"ACGT", np.uint8)
    long_ = letters[synth.reads_from_ref_fast(codes, max(1, int(1_000 * a.scale)), 100_000, 2)]
    short = letters[synth.reads_from_ref_fast(codes, max(1, int(1_000_000 * a.scale)), 150, 1)]
    batches = [("fasta_1kx100k_w60", as_fasta(long_, 60), long_, True), ("fasta_1Mx150", as_fasta(short, 150), short, False)]
    out = {"reps": a.reps, "list_reps": a.list_reps, "scale": a.scale, "device": torch.cuda.get_device_name(0),
           "units": {"ingest": "us", "wall": "ms"}}
    for name, fasta, ascii_reads, with_wall in batches:
        n, L = ascii_reads.shape
        lines = as_lines(ascii_reads)
        d_fasta = torch.from_numpy(np.frombuffer(fasta, np.uint8).copy()).cuda()
        d_lines = torch.from_numpy(np.frombuffer(lines, np.uint8).copy()).cuda()
        outs = {k: (torch.empty(n * L, dtype=torch.uint8, device="cuda"), torch.empty(n + 1, dtype=torch.int64, device="cuda"))
                for k in ("fasta", "lines")}
        starts = torch.empty(n, dtype=torch.int64, device="cuda")
        tmp_f = torch.empty(int(L_.genie_reads_from_fasta_tmp_bytes(len(fasta), n)), dtype=torch.uint8, device="cuda")
        tmp_l = torch.empty(int(L_.genie_reads_from_text_tmp_bytes(len(lines), n)), dtype=torch.uint8, device="cuda")
        out5 = {"fasta": (C.c_int64 * 5)(), "lines": (C.c_int64 * 5)()}

        def ingest_fasta():
            b, o = outs["fasta"]
            rc = L_.genie_reads_from_fasta(_ptr(d_fasta), len(fasta), 0, tab, _ptr(b), n * L, _ptr(o), _ptr(starts), n, out5["fasta"],
                                           _ptr(tmp_f), tmp_f.numel(), sp)
            g._native.check(rc, "genie_reads_from_fasta")

        def ingest_lines():
            b, o = outs["lines"]
            rc = L_.genie_reads_from_text(_ptr(d_lines), len(lines), g._native.TEXT_LINES, 0, tab, _ptr(b), n * L, _ptr(o), n,
                                          out5["lines"], _ptr(tmp_l), tmp_l.numel(), sp)
            g._native.check(rc, "genie_reads_from_text")

        fns = (("fasta", ingest_fasta), ("lines", ingest_lines))
        for _, fn in fns + fns:                                      # warm-up
            fn()
        torch.cuda.synchronize()
        assert list(out5["fasta"])[:3] == list(out5["lines"])[:3] == [n, n * L, L]
        assert torch.equal(outs["fasta"][0], outs["lines"][0]) and torch.equal(outs["fasta"][1], outs["lines"][1])
        assert torch.equal(starts, torch.arange(n, dtype=torch.int64, device="cuda") * (len(fasta) // n))
        times = {"fasta": [], "lines": []}
        for _ in range(a.reps):
            for key, fn in fns:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                times[key].append(e0.elapsed_time(e1) * 1e3)
        res = {"reads": n, "read_len": L, "fasta_bytes": len(fasta), "lines_bytes": len(lines),
               "fasta": stats(times["fasta"]), "lines": stats(times["lines"])}
        for key, nbytes in (("fasta", len(fasta)), ("lines", len(lines))):
            res[key]["ns_per_text_byte"] = round(res[key]["median"] * 1e3 / nbytes, 5)
            res[key]["Gbases_per_s"] = round(n * L / res[key]["median"] / 1e3, 1)
        res["slower_per_byte_us"] = round(res["fasta"]["median"] - res["lines"]["median"] * len(fasta) / len(lines), 1)
        res["yardstick_spread_us"] = round(res["lines"]["max"] - res["lines"]["min"], 1)
        del d_fasta, d_lines, outs, starts, tmp_f, tmp_l
        torch.cuda.empty_cache()
        print(f"# {name}: device times done", file=sys.stderr, flush=True)
        if with_wall:
            strings = [row.tobytes().decode("ascii") for row in ascii_reads]

            def wall(fn, reps):
                ts = []
                for _ in range(reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    r = fn()
                    torch.cuda.synchronize()
                    ts.append((time.perf_counter() - t0) * 1e3)
                    total = int(r[0][-1].item())
                    del r
                return ts, total

            wall(lambda: sm.find_smems_text(fasta, "fasta"), 2)     # warm-up: the allocator's pools
            t_text, total_text = wall(lambda: sm.find_smems_text(fasta, "fasta"), a.reps)
            wall(lambda: sm.find_smems_long(strings, 1, split_breaks=True), 1)
            t_list, total_list = wall(lambda: sm.find_smems_long(strings, 1, split_breaks=True), a.list_reps)
            assert total_text == total_list
            res["wall"] = {"smems": total_text, "find_smems_text_fasta": stats(t_text, 2), "find_smems_long_list": stats(t_list, 2)}
            res["wall"]["speedup"] = round(res["wall"]["find_smems_long_list"]["median"] / res["wall"]["find_smems_text_fasta"]["median"], 2)
            del strings
        out[name] = res
        print(f"# {name}: {json.dumps(res)}", file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
