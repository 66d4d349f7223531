"""Wall time of the two ways to get a queryable index image on the GPU, for synthetic references:
host build (genie_index_create_ex) + serialize + upload, against the device build (genie_index_create_device).
One JSON line per size.  Usage: python tools/time_device_build.py 1000000 17000000 [--skip-host-above N]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sizes", type=int, nargs="+")
    ap.add_argument("--K", type=int, default=15)
    ap.add_argument("--skip-host-above", type=int, default=1 << 62)
    a = ap.parse_args()
    for n in a.sizes:
        ref = synth.synth_ref(n, n)
        d_ref = torch.as_tensor(ref).cuda()
        g.GenieIndex.build_on_device(d_ref[:100_000], a.K)              # warm-up: module load, allocator
        torch.cuda.synchronize()
        row = {"n": n, "K": a.K}
        t0 = time.perf_counter()
        dev = g.GenieIndex.build_on_device(d_ref, a.K)
        torch.cuda.synchronize()
        row["device_build_s"] = round(time.perf_counter() - t0, 4)
        row["image_bytes"] = int(dev.blob.numel())
        if n <= a.skip_host_above:
            t0 = time.perf_counter()
            host = g.GenieIndex.build(ref, a.K)
            t1 = time.perf_counter()
            img = host.serialize()
            t2 = time.perf_counter()
            d_img = img.cuda()
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            row.update(host_build_s=round(t1 - t0, 4), serialize_s=round(t2 - t1, 4), upload_s=round(t3 - t2, 4),
                       host_path_s=round(t3 - t0, 4), identical=bool(torch.equal(d_img, dev.blob)))
        print(json.dumps(row), flush=True)
        del dev


if __name__ == "__main__":
    main()
