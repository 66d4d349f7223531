"""Cost of genie_insert_size_stats (the insert-size distribution of a paired batch) next to
genie_pair_alignments, the call it feeds, and next to a bare device copy of as many bytes as the head rows it must read (48 per
read), taken in the same run on the same batches:
  cfg1_500kx2x150   the two batches of tools/time_pair.py as they are: reads drawn from the forward strand
  tandem7_10kx2x150 and taken two by two as mates, so every sample is of type "same" and the spans are as wide as a contig
  narrow_500kx2     5 x 10^5 synthetic pairs, one record per read, every head unique (mapq 60), FR, spans from a normal
                    distribution (mean 450, deviation 40): nearly all samples in a few hundred neighbouring bins, the contended
                    case the histogram in LDS exists for
with the wrapper's defaults (min_mapq 20, max_span 10000, min_samples 25).  Calls on preallocated buffers, each with its
synchronisation included, timed with HIP events (torch.cuda.Event) after warm-up runs and interleaved round by round:
  isize      genie_insert_size_stats with every output
  pair       genie_pair_alignments with every output
  copy       a device-to-device copy of 48 bytes per read
  isize_no_lds   narrow_500kx2 only, with --no-lds-lib: the same call from a library built with -DGENIE_ISIZE_NO_LDS
                 (make -C genie-smem_amd/csrc EXTRA=-DGENIE_ISIZE_NO_LDS BUILD=<dir> OUT=<path>), every span counted in the global
                 histogram at once; its statistics must equal the other build's
The median and the spread (min, max) of --reps repeats in us, the statistics, the totals, and the ratios of the medians.  The
statistics of the synthetic batch are checked once against numpy.  One JSON line.
Usage: python tools/time_isize.py [--reps 10] [--scale 1.0] [--no-lds-lib PATH] [--skip-mapped] [--out profiles/isize_time.json]"""
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
from tools.time_chains import DEFAULTS  # noqa: E402
from tools.time_mems import stats, tandem_batch  # noqa: E402
from tools.time_pair import PAIR, SELECT  # noqa: E402

ISIZE = dict(min_mapq=20, max_span=10000, min_samples=25)
COLS = "n ok q25 q50 q75 lo_b hi_b n_in mean std isize_min isize_max".split()


def mapped_batch(ix, rs, bases, offs, m, cprm, sprm):
    """select_alignments' (sel_offsets, records, klass) of a batch of reads."""
    row_off, rows, _, _ = ix.find_mems_contigs(rs, bases, offs, m)
    chained = ix.chain_mems(row_off, rows, rs, **cprm)
    aln, _ = ix.align_chains((bases, offs), row_off, rows, chained, rs, **ALIGN)
    res = ix.select_alignments(offs, chained[0], chained[1], aln, rs, False, **sprm)
    return res[0].contiguous(), res[2].contiguous(), res[3].contiguous()


def narrow_batch(pairs, seed=7):
    """One record per read: mate 0 forward at a random place of one contig, mate 1 reverse, the span normal(450, 40)."""
    rng = np.random.default_rng(seed)
    span = np.clip(np.rint(rng.normal(450, 40, pairs)), 101, 5000).astype(np.int64)
    at = rng.integers(1, 10**8, pairs)
    rec = np.zeros((2 * pairs, 12), np.int32)
    rec[:, 0] = np.arange(2 * pairs)
    rec[:, 1] = np.arange(2 * pairs)
    rec[1::2, 3] = 1
    rec[0::2, 5], rec[1::2, 5] = at, at + span - 100
    rec[:, 6], rec[:, 8], rec[:, 9], rec[:, 11] = 100, 100, 100, 60
    klass = np.zeros((2 * pairs, 4), np.int32)
    klass[:, 1], klass[:, 3] = np.arange(2 * pairs), 60
    return np.arange(2 * pairs + 1, dtype=np.int64), rec, klass, span


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the batch sizes (a quick look)")
    ap.add_argument("--no-lds-lib", default="", help="a library built with -DGENIE_ISIZE_NO_LDS")
    ap.add_argument("--skip-mapped", action="store_true", help="the synthetic batch alone")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L_ = g._native.lib()
    other = None
    if a.no_lds_lib:
        other = C.CDLL(os.path.abspath(a.no_lds_lib))
        other.genie_insert_size_stats.restype = L_.genie_insert_size_stats.restype
        other.genie_insert_size_stats.argtypes = L_.genie_insert_size_stats.argtypes
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = {"reps": a.reps, "scale": a.scale, "device": torch.cuda.get_device_name(0), "units": "us", "isize": ISIZE, "pair": PAIR,
           "lds_bins": g._native.ISIZE_LDS_BINS}
    codes = synth.synth_ref(100_000, 100_000)
    n1, n3, n4 = (2 * max(1, int(k * a.scale)) for k in (500_000, 10_000, 500_000))
    batches = []
    if not a.skip_mapped:
        tref, treads = tandem_batch(n3, 150, 3)
        batches += [("cfg1_500kx2x150", codes, 25, synth.reads_from_ref_fast(codes, n1, 150, 1), 19, DEFAULTS, SELECT),
                    ("tandem7_10kx2x150", tref, 1, treads, 19, dict(DEFAULTS, max_pred=64, bandwidth=64), dict(SELECT, max_secondary=16))]
    batches.append(("narrow_500kx2", codes[:4096], 1, None, 0, None, None))
    for name, ref, n_contigs, reads, m, cprm, sprm in batches:
        ix = g.GenieIndex.build(ref, 0).to("cuda")
        want = None
        if reads is None:
            so, rec, klass, span = narrow_batch(n4 // 2)
            s_off, rec, klass = (torch.from_numpy(x).cuda() for x in (so, rec, klass))
            n = n4
        else:
            if isinstance(reads, np.ndarray):
                n, lens, flat = reads.shape[0], np.full(reads.shape[0], reads.shape[1], np.int64), reads.reshape(-1)
            else:
                n, lens, flat = len(reads), np.asarray([len(r) for r in reads], np.int64), np.concatenate(reads)
            bases = torch.from_numpy(np.ascontiguousarray(flat)).cuda()
            offs = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).cuda()
            rs = g.ReferenceSet([str(i) for i in range(n_contigs)], np.linspace(0, ref.size, n_contigs + 1).astype(np.int64), ref)
            s_off, rec, klass = mapped_batch(ix, rs, bases, offs, m, cprm, sprm)
            del bases, offs
        cap, kept = rec.shape[0], klass.shape[0]
        p3 = [ISIZE[k] for k in ("min_mapq", "max_span", "min_samples")]
        p8 = [PAIR[k] for k in ("orient", "isize_min", "isize_max", "isize_mean", "pen_slope", "pen_max", "pen_unpaired", "mapq_boost")]
        ws_i = torch.empty(max(256, int(L_.genie_insert_size_stats_workspace_bytes(n, ISIZE["max_span"]))), dtype=torch.uint8, device="cuda")
        st, st2 = (torch.empty((3, 12), dtype=torch.int64, device="cuda") for _ in range(2))
        smp = torch.empty((n // 2, 2), dtype=torch.int32, device="cuda")
        it = torch.empty(4, dtype=torch.int64, device="cuda")

        def isize(lib=L_, stats_=st):
            g._native.check(lib.genie_insert_size_stats(ix._h, n, _ptr(s_off), _ptr(rec), cap, *p3, _ptr(stats_), _ptr(smp), _ptr(it),
                                                        _ptr(ws_i), ws_i.numel(), sp), "genie_insert_size_stats")

        ws_p = torch.empty(max(256, int(L_.genie_pair_alignments_workspace_bytes(n, cap))), dtype=torch.uint8, device="cuda")
        pairs = torch.empty((n // 2, 8), dtype=torch.int32, device="cuda")
        sam = torch.empty((max(cap, 1), 4), dtype=torch.int32, device="cuda")
        pt = torch.empty(4, dtype=torch.int64, device="cuda")

        def pair():
            g._native.check(L_.genie_pair_alignments(ix._h, n, _ptr(s_off), _ptr(rec), cap, _ptr(klass), kept, *p8, _ptr(pairs), _ptr(sam),
                                                     _ptr(pt), _ptr(ws_p), ws_p.numel(), sp), "genie_pair_alignments")

        src = torch.empty(48 * n, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)

        def copy():
            dst.copy_(src)
            torch.cuda.synchronize()

        fns = [("isize", isize), ("pair", pair), ("copy", copy)]
        if other is not None and reads is None:
            fns.append(("isize_no_lds", lambda: isize(other, st2)))
        for _, fn in fns:
            fn()
        torch.cuda.synchronize()
        got = st.cpu().numpy()
        if reads is None:
            v = np.sort(span)
            k = v.size
            q = [int(v[min(k - 1, (k + 1) // 4)]), int(v[k // 2]), int(v[min(k - 1, (3 * k + 1) // 4)])]
            if got[0, :5].tolist() != [k, 1] + q or got[1:, 0].any() or it.tolist() != [k, k, 0, 0]:
                raise SystemExit(f"{name}: the statistics {got[0].tolist()} are not those of the planted spans {[k, 1] + q}")
            if other is not None and not torch.equal(st, st2):
                raise SystemExit(f"{name}: the build without the LDS histogram gives other statistics")
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
        res = {"reads": n, "pairs": n // 2, "records": cap, "head_row_bytes": 48 * n, "workspace_bytes": ws_i.numel(),
               "stats": {t: dict(zip(COLS, (int(x) for x in got[i]))) for i, t in enumerate(("fr", "rf", "same"))},
               "totals": dict(zip(("both_mapped", "sampled", "mapq_alone", "contig_type_span"), (int(x) for x in it.tolist())))}
        for key, _ in fns:
            res[key] = stats(times[key])
        res["isize"]["ratio_to_pair_alignments"] = round(res["isize"]["median"] / res["pair"]["median"], 3)
        res["isize"]["ratio_to_copy"] = round(res["isize"]["median"] / res["copy"]["median"], 3)
        if "isize_no_lds" in res:
            res["isize_no_lds"]["ratio_to_isize"] = round(res["isize_no_lds"]["median"] / res["isize"]["median"], 3)
        out[name] = res
        print(f"# {name}: {json.dumps(res)}", file=sys.stderr, flush=True)
        del s_off, rec, klass, ws_i, ws_p, pairs, sam, smp, src, dst
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
