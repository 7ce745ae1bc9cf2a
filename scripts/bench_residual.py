#!/usr/bin/env python3
"""The .res coder, device against host, and what exactness costs on top of decompress_rec, on one box in one process.  Writes
profiles/residual/bench.json (or --out), rewritten after every row; the file names the box (--box), the device, and under
`not_measured` every size of the list that the run was not asked for.  Diagnostic; needs a GPU.

The 24-block model of scripts/config3_harness.py on 32 x 32 images.  No trained model or dataset exists, so the images are made to
sit around the model's output the way a trained model's do: the reconstruction of a noise image, quantised, plus logistic noise of
--levels grey levels, coded at likelihood_log_scale = log(levels / 256) (about log2(levels) + 2 bits per pixel).  Per size, [median,
min, max] in milliseconds of --reps calls after --warmup calls (host clock around a call that ends synchronised):
  res_encode_device / res_decode_device    irec.io.encode_residuals_device / decode_residuals_device at the default stream_len, tensors on
                                           the device, the call's one read-back included
  res_encode_host16 / _host1, res_decode_* the host twins on 16 threads and on 1, with the copies they need: pixels and loc (or the
                                           bytes and loc) to the host, the result back to the device
  decompress_rec / decompress_lossless     the model's two read paths on the same files, max_K and stream_len passed
and at --size-at images, for every stream_len of STREAM_LENS: the files' bits against residual_model_bits, and the device times.
Before anything is timed the round trip is checked (torch.equal) at every size."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "relative-entropy-coding_amd"), os.path.join(ROOT, "scripts")]

SIZES = (1, 38, 300, 4096)
STREAM_LENS = (32, 64, 128, 256, 1024)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "residual", "bench.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default=",".join(str(n) for n in SIZES))
    ap.add_argument("--size-at", type=int, default=300, help="the batch at which the stream_len rows are taken")
    ap.add_argument("--blocks", type=int, default=24)
    ap.add_argument("--levels", type=float, default=4.0)
    ap.add_argument("--box", default="", help="the machine this runs on, in words (written into the file)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_residual.py measures a GPU: none here")
    from config3_harness import build_model
    from irec.io import rec_files_max_K
    from irec.io import residual as R
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    model = build_model(device, args.blocks)
    with torch.no_grad():
        model.likelihood_log_scale.fill_(float(np.log(args.levels / 256.0)))
    scale = model.likelihood_scale()
    g = torch.Generator().manual_seed(7)
    sizes_run = [int(v) for v in args.sizes.split(",")]
    L0 = R.DEFAULT_STREAM_LEN
    result = {"box": args.box, "device": torch.cuda.get_device_name(0), "arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", ""),
              "host_cpus_available": len(os.sched_getaffinity(0)), "torch": torch.__version__,
              "model": f"{args.blocks}-block RVAE shim, 32x32 images, B=20 Omega=3 eps=0.2, block_size 1000", "reps": args.reps,
              "warmup": args.warmup, "unit": "ms per call: [median, min, max]", "likelihood_scale": scale, "default_stream_len": L0,
              "images": f"reconstruction of a noise image, quantised, plus logistic noise of {args.levels} grey levels",
              "not_measured": [f"n_images {n}: not among --sizes of this run" for n in SIZES if n not in sizes_run], "rows": [], "stream_len_rows": []}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")

    def make_images(n):
        """uint8 images around the model's own output, and their coded form, in chunks of 512."""
        parts = []
        for lo in range(0, n, 512):
            m = min(512, n - lo)
            noise = torch.randint(0, 256, (m, 3, 32, 32), generator=g, dtype=torch.uint8).to(device)
            recon = model.compress_lossless(noise, SEED)[4]
            u = torch.rand(recon.shape, generator=g).clamp_(1e-6, 1 - 1e-6).to(device)
            x = torch.floor((recon + 0.5) * 256) + torch.round(args.levels * (torch.log(u) - torch.log1p(-u)))
            parts.append(x.clamp_(0, 255).to(torch.uint8))
        return torch.cat(parts)

    def code(images):
        recs, ress, locs = [], [], []
        for lo in range(0, images.shape[0], 512):
            rb, ro, sb, so, loc = model.compress_lossless(images[lo:lo + 512], SEED)
            recs.append((rb.cpu().numpy(), np.diff(ro.cpu().numpy())))
            ress.append((sb.cpu().numpy(), np.diff(so.cpu().numpy())))
            locs.append(loc)
        def join(parts):
            return np.concatenate([p[0] for p in parts]), np.concatenate([[0], np.cumsum(np.concatenate([p[1] for p in parts]))]).astype(np.int64)
        return join(recs), join(ress), torch.cat(locs)

    for n in sizes_run:
        images = make_images(n)
        shape = tuple(images.shape)
        (rec_host, rec_off), (res_host, res_off), loc = code(images)
        rec_dev, res_dev = torch.from_numpy(rec_host).to(device), torch.from_numpy(res_host).to(device)
        max_K = rec_files_max_K(rec_host, rec_off)
        ideal = R.residual_model_bits(images, loc, scale)

        def enc_dev():
            return R.encode_residuals_device(images, loc, scale, stream_len=L0)

        def dec_dev():
            return R.decode_residuals_device(res_dev, res_off, loc, scale, stream_len=L0)

        def enc_host(threads):
            blob, off = R.encode_residuals(images.cpu().numpy(), loc.cpu().numpy(), scale, stream_len=L0, n_threads=threads)
            return torch.from_numpy(blob).to(device), off

        def dec_host(threads):
            return torch.from_numpy(R.decode_residuals(res_dev.cpu().numpy(), res_off, loc.cpu().numpy(), scale, stream_len=L0, n_threads=threads)).to(device)

        def rec_only():
            return model.decompress_rec(rec_dev, rec_off, SEED, shape, max_K=max_K)

        def lossless():
            return model.decompress_lossless(rec_dev, rec_off, res_dev, res_off, SEED, shape, max_K=max_K, stream_len=L0)

        blob_d, off_d = enc_dev()
        equal = bool(torch.equal(lossless(), images)) and bool(torch.equal(dec_dev(), images)) and bool(torch.equal(dec_host(16), images)) and \
            np.array_equal(blob_d.cpu().numpy(), res_host) and np.array_equal(enc_host(16)[0].cpu().numpy(), res_host)
        row = {"n_images": n, "stream_len": L0, "rec_bytes": int(rec_off[-1]), "res_bytes": int(res_off[-1]), "max_K": int(max_K),
               "residual_model_bits": float(ideal.sum()), "res_bits_over_model_bits": round(int(res_off[-1]) * 8 / float(ideal.sum()), 5),
               "res_bits_per_dim": round(int(res_off[-1]) * 8 / (n * 3072), 4), "round_trips_exact_and_bytes_equal": equal}
        row["res_encode_device"] = spread_ms(enc_dev, args.reps, args.warmup)
        row["res_decode_device"] = spread_ms(dec_dev, args.reps, args.warmup)
        for threads in (16, 1):
            row[f"res_encode_host{threads}"] = spread_ms(lambda: enc_host(threads), args.reps, args.warmup)
            row[f"res_decode_host{threads}"] = spread_ms(lambda: dec_host(threads), args.reps, args.warmup)
        row["decompress_rec"] = spread_ms(rec_only, args.reps, args.warmup)
        row["decompress_lossless"] = spread_ms(lossless, args.reps, args.warmup)
        row["lossless_over_rec"] = round(row["decompress_lossless"][0] / row["decompress_rec"][0], 3)
        result["rows"].append(row)
        print(json.dumps(row), flush=True)
        save()
        if n == args.size_at:
            for L in STREAM_LENS:
                blob, off = R.encode_residuals_device(images, loc, scale, stream_len=L)
                ok = bool(torch.equal(R.decode_residuals_device(blob, off, loc, scale, stream_len=L), images))
                bits = int(off[-1]) * 8
                srow = {"n_images": n, "stream_len": L, "res_bits": bits, "residual_model_bits": float(ideal.sum()),
                        "overhead_bits_per_image": round((bits - float(ideal.sum())) / n, 1), "res_bits_over_model_bits": round(bits / float(ideal.sum()), 5),
                        "round_trip_exact": ok,
                        "res_encode_device": spread_ms(lambda: R.encode_residuals_device(images, loc, scale, stream_len=L), args.reps, args.warmup),
                        "res_decode_device": spread_ms(lambda: R.decode_residuals_device(blob, off, loc, scale, stream_len=L), args.reps, args.warmup)}
                result["stream_len_rows"].append(srow)
                print(json.dumps(srow), flush=True)
                save()
        del images, loc, rec_dev, res_dev
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
