"""Cost of reading a batch from text on the device (genie_reads_from_text), on reads drawn from the 100 kb synthetic
reference (create_query_from_ref distribution):
  lines_1Mx150   10^6 x 150-base reads, one per line
  fastq_1Mx150   the same reads as four-line FASTQ records (a 32-byte header line, 150 quality symbols)
  lines_1kx100k  10^3 x 10^5-base reads, one per line
Per batch:
  (a) ingest   genie_reads_from_text alone (the full call on preallocated buffers; its one synchronisation included), and its
               bytes per second against the compulsory traffic: the text read once, total_bases and 8 (N + 1) bytes written;
  (b) search   genie_find_smems_long_ex (BWA, GENIE_READS_SPLIT_BREAKS) on the reads (a) produced, and the ratio (a) / (b);
  (c) wall     SMEM.find_smems_text(bytes), upload included, against SMEM.find_smems_long(list of the same strings,
               split_breaks=True), whose path this tool's commit leaves as its parent has it: host wall-clock, device idle
               before and after.
(a) and (b) are timed with HIP events (torch.cuda.Event) after warm-up runs, interleaved round by round: the median and the
spread of --reps repeats in us.  (c): the median of --reps runs of the text path and --list-reps runs of the list path (each
of those spends seconds encoding on the host), in ms.  One JSON line.
Usage: python tools/time_text_reads.py [--reps 20] [--list-reps 5] [--scale 1.0] [--out profiles/text_reads_time.json]"""
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

HEADER = b"@SIM:1:FCX:1:1101:0000000:00000\n"
assert len(HEADER) == 32


def as_lines(ascii_reads):
    n, L = ascii_reads.shape
    out = np.full((n, L + 1), 0x0A, np.uint8)
    out[:, :L] = ascii_reads
    return out.tobytes()


def as_fastq(ascii_reads):
    n, L = ascii_reads.shape
    rec = np.empty((n, 32 + L + 1 + 2 + L + 1), np.uint8)
    rec[:, :32] = np.frombuffer(HEADER, np.uint8)
    rec[:, 32:32 + L] = ascii_reads
    rec[:, 32 + L:32 + L + 3] = np.frombuffer(b"\n+\n", np.uint8)
    rec[:, 32 + L + 3:-1] = ord("I")
    rec[:, -1] = 0x0A
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
    ix = m.index(15)
    table = m.byte_codes()
    letters = np.frombuffer(b"ACGT", np.uint8)
    short = letters[synth.reads_from_ref_fast(codes, max(1, int(1_000_000 * a.scale)), 150, 1)]
    long_ = letters[synth.reads_from_ref_fast(codes, max(1, int(1_000 * a.scale)), 100_000, 2)]
    batches = [("lines_1Mx150", "lines", as_lines(short), short), ("fastq_1Mx150", "fastq", as_fastq(short), short),
               ("lines_1kx100k", "lines", as_lines(long_), long_)]
    out = {"reps": a.reps, "list_reps": a.list_reps, "scale": a.scale, "device": torch.cuda.get_device_name(0),
           "units": {"ingest": "us", "search": "us", "wall": "ms"}}
    for name, fmt, text, ascii_reads in batches:
        n, L = ascii_reads.shape
        nbytes = len(text)
        d_text = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).cuda()
        bases = torch.empty(n * L, dtype=torch.uint8, device="cuda")
        roff = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        tmp_bytes = int(L_.genie_reads_from_text_tmp_bytes(nbytes, n))
        tmp = torch.empty(tmp_bytes, dtype=torch.uint8, device="cuda")
        out5 = (C.c_int64 * 5)()
        flags = g._native.READS_SPLIT_BREAKS
        ws_bytes = int(L_.genie_find_smems_long_ex_workspace_bytes(n, n * L, L, flags))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
        cap = 2 * n * L // 3
        rows = torch.empty((cap, 4), dtype=torch.int32, device="cuda")
        off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        st = torch.empty(n, dtype=torch.int32, device="cuda")

        def ingest():
            rc = L_.genie_reads_from_text(_ptr(d_text), nbytes, g._native.TEXT_FORMATS[fmt], 0, table.ctypes.data_as(C.c_void_p),
                                          _ptr(bases), n * L, _ptr(roff), n, out5, _ptr(tmp), tmp_bytes, sp)
            g._native.check(rc, "genie_reads_from_text")

        def search():
            rc = L_.genie_find_smems_long_ex(ix._h, 0, flags, _ptr(bases), _ptr(roff), n, n * L, L, 1, _ptr(off), _ptr(rows), cap,
                                             _ptr(st), _ptr(ws), ws_bytes, sp)
            g._native.check(rc, "genie_find_smems_long_ex")

        times = {"ingest": [], "search": []}
        for fn in (ingest, search, ingest, search):                 # warm-up
            fn()
        torch.cuda.synchronize()
        assert list(out5)[:3] == [n, n * L, L]
        smems = int(off[n].item())
        for _ in range(a.reps):
            for key, fn in (("ingest", ingest), ("search", search)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                times[key].append(e0.elapsed_time(e1) * 1e3)
        res = {"reads": n, "read_len": L, "text_bytes": nbytes, "smems": smems, "ingest": stats(times["ingest"]),
               "search": stats(times["search"])}
        traffic = nbytes + n * L + 8 * (n + 1)
        res["ingest"]["compulsory_bytes"] = traffic
        res["ingest"]["GB_per_s"] = round(traffic / res["ingest"]["median"] / 1e3, 1)
        res["ingest"]["Gbases_per_s"] = round(n * L / res["ingest"]["median"] / 1e3, 1)
        res["search"]["Gbases_per_s"] = round(n * L / res["search"]["median"] / 1e3, 1)
        res["ingest_over_search"] = round(res["ingest"]["median"] / res["search"]["median"], 4)
        del d_text, bases, roff, tmp, ws, rows, off, st
        torch.cuda.empty_cache()
        print(f"# {name}: device times done", file=sys.stderr, flush=True)

        # (c) end to end on the host clock
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

        wall(lambda: sm.find_smems_text(text, fmt), 2)               # warm-up: the allocator's pools
        t_text, total_text = wall(lambda: sm.find_smems_text(text, fmt), a.reps)
        print(f"# {name}: text path done", file=sys.stderr, flush=True)
        wall(lambda: sm.find_smems_long(strings, 1, split_breaks=True), 1)
        t_list, total_list = wall(lambda: sm.find_smems_long(strings, 1, split_breaks=True), a.list_reps)
        assert total_text == total_list == smems
        res["wall"] = {"find_smems_text": stats(t_text, 2), "find_smems_long_list": stats(t_list, 2)}
        res["wall"]["speedup"] = round(res["wall"]["find_smems_long_list"]["median"] / res["wall"]["find_smems_text"]["median"], 2)
        out[name] = res
        print(f"# {name}: {json.dumps(res)}", file=sys.stderr, flush=True)
        del strings
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
