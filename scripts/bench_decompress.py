#!/usr/bin/env python3
""".rec files -> pixels, the list path against the device path, on one box in one process.  Writes profiles/decompress/bench.json
(or --out), one row per batch size, rewritten after every row; the file names the box (--box), the device, and under `not_measured`
every size of the list that the run was not asked for.  Diagnostic; needs a GPU.

The 24-block model of scripts/config3_harness.py on 32 x 32 images (8192-dim latents: 9 blocks of 1000 per residual block).  The files
are written once per size by model.compress_rec.  Per size, [median, min, max] in milliseconds of --reps calls after --warmup calls
(host clock around a call that ends synchronised):
  list_path     what the parent commit offers: irec.io.read_compressed_code per file, then model.decompress on the nested lists
                (24 host round trips, a Python loop over every block)
  device_path   harness.decompress_images: the files read and their headers parsed on the host, the bytes uploaded once, the
                arithmetic decoder, the row checks and the generative pass on the device, one read-back
  device_rec    model.decompress_rec alone on bytes that are on the device already (no file reads)
N = 1 also through GraphedDecompress (one HIP graph replay per call) against eager decompress_rec.
Before anything is timed the two paths' pixels are compared (torch.equal) at every size."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "relative-entropy-coding_amd"), os.path.join(ROOT, "scripts")]

SIZES = (1, 38, 300, 4096)
SEED = 42


def spread_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return [round(statistics.median(ts), 3), round(min(ts), 3), round(max(ts), 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decompress", "bench.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default=",".join(str(n) for n in SIZES))
    ap.add_argument("--blocks", type=int, default=24)
    ap.add_argument("--box", default="", help="the machine this runs on, in words (written into the file)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_decompress.py measures a GPU: none here")
    from config3_harness import build_model
    from irec import harness
    from irec.io import read_compressed_code, rec_files_max_K
    from irec.models import GraphedDecompress
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    model = build_model(device, args.blocks)
    g = torch.Generator().manual_seed(7)
    out_dir = tempfile.mkdtemp(prefix="irec_decompress_bench_")
    sizes_run = [int(v) for v in args.sizes.split(",")]
    result = {"box": args.box, "device": torch.cuda.get_device_name(0), "arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", ""),
              "host_cpus_available": len(os.sched_getaffinity(0)), "torch": torch.__version__,
              "model": f"{args.blocks}-block RVAE shim, 32x32 images, B=20 Omega=3 eps=0.2, block_size 1000", "reps": args.reps,
              "warmup": args.warmup, "unit": "ms per call: [median, min, max]",
              "not_measured": [f"n_images {n}: not among --sizes of this run" for n in SIZES if n not in sizes_run], "rows": []}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")

    for n in sizes_run:
        images = (torch.rand(n, 3, 32, 32, generator=g) - 0.5).to(device)
        shape = tuple(images.shape)
        paths, blobs, sizes = [], [], []
        for lo in range(0, n, 512):                                   # the files, written once
            blob, off, _ = model.compress_rec(images[lo:lo + 512], seed=SEED)
            host, o = blob.cpu().numpy(), off.cpu().numpy()
            for i in range(len(o) - 1):
                paths.append(os.path.join(out_dir, f"n{n}_{lo + i:05d}.rec"))
                with open(paths[-1], "wb") as fh:
                    fh.write(host[o[i]:o[i + 1]].tobytes())
                sizes.append(int(o[i + 1] - o[i]))
            blobs.append(host)
        host = np.concatenate(blobs)
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        blob_dev = torch.from_numpy(host).to(device)
        max_K = rec_files_max_K(host, off)

        def list_path():
            codes = [read_compressed_code(p)[3] for p in paths]
            return model.decompress(codes[0] if n == 1 else codes, seed=SEED, image_shape=shape)

        def device_path():
            return harness.decompress_images(model, paths)[0]

        def device_rec():
            return model.decompress_rec(blob_dev, off, SEED, shape, max_K=max_K)

        ref = list_path()
        equal = bool(torch.equal(device_path(), ref)) and bool(torch.equal(device_rec(), ref))
        row = {"n_images": n, "file_bytes": int(off[-1]), "max_K": int(max_K), "device_pixels_equal_list_pixels": equal}
        row["list_path"] = spread_ms(list_path, args.reps, args.warmup)
        row["device_path"] = spread_ms(device_path, args.reps, args.warmup)
        row["device_rec"] = spread_ms(device_rec, args.reps, args.warmup)
        row["list_over_device"] = round(row["list_path"][0] / row["device_path"][0], 3)
        if n == 1:
            gd = GraphedDecompress(model, shape, SEED, R=args.blocks, bpt=model.blocks_per_tensor(shape), max_K=max_K, blob_bytes=int(off[-1]))
            row["graph_pixels_equal_list_pixels"] = bool(torch.equal(gd(blob_dev, off), ref))
            row["graphed_rec"] = spread_ms(lambda: gd(blob_dev, off), args.reps, args.warmup)
            row["graph_captures"] = gd.captures
        result["rows"].append(row)
        print(json.dumps(row), flush=True)
        save()
        del images, blob_dev, ref
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
