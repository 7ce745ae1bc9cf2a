#!/usr/bin/env python3
"""Per-channel likelihood scales and their fitter on one box in one process.  Writes profiles/residual_scales/bench.json (or --out),
rewritten after every row; the file names the box (--box), the device, and under `not_measured` what the run was not asked for or
cut short.  Diagnostic; needs a GPU.

The 24-block model of scripts/config3_harness.py on 32 x 32 images, made as scripts/bench_residual.py makes them (the reconstruction of
a noise image, quantised, plus logistic noise) but with another noise width per colour channel (--levels grey levels), so that one
scale cannot fit all three.  Per size, [median, min, max] in milliseconds of --reps calls after --warmup calls (host clock around a
call that ends synchronised); the legs of a comparison ALTERNATE inside every repetition, so that drift hits both alike.  A leg whose
repetitions would take more than --budget seconds stops early (at least 3) and its row says how many it ran (`reps_run_<first leg>`).
  (a) v1_encode / v2_encode, v1_decode / v2_decode    encode_residuals_device / decode_residuals_device on the same tensors with the
      scalar scale and with three equal-cost channel scales, the call's one read-back included
  (b) scale_bits_device_1 / _64                         one scale_bits_device call at 1 and 64 candidates (no read-back: synchronised;
                                                        one untimed call before each timed one, the host legs leave the GPU idle),
      scale_bits_host16_* / host1_*                     the host twin on 16 threads and on 1 with the copies it needs
  (c) fit_single / fit_per_channel                      one model.fit_likelihood_scale call (the model's two passes included),
      fit_search_only_*                                 irec.io.residual.fit_scales alone on reconstructions already made
  (d) res_bytes and residual_model_bits per image at log_scale = 0, fitted single, fitted per channel
and one Kodak-size row (24 images of 3 x 512 x 768, synthetic loc and logistic pixels: no model pass) for (b) and the search of (c)."""
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

SIZES = (1, 38, 300, 4096)            # (1: the row where a host twin may win)
SEED = 42
CHUNK = 512


def alternate_ms(legs, reps, warmup, budget, rewarm=()):
    """{name: [median, min, max]} of the legs' calls, one call of every leg per repetition in turn; `reps_run_<first leg>` if the
    budget cut it.  rewarm: legs that get one untimed call before every timed one (a device leg that follows seconds of host work
    otherwise pays for a GPU that has gone idle: 12.6 ms median against 0.58 ms minimum in a first run of the Kodak-size row)."""
    for _ in range(warmup):
        for fn in legs.values():
            fn()
    ts = {name: [] for name in legs}
    t_start = time.perf_counter()
    for rep in range(reps):
        for name, fn in legs.items():
            if name in rewarm:
                fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[name].append((time.perf_counter() - t0) * 1e3)
        if rep + 1 >= 3 and time.perf_counter() - t_start > budget:
            break
    out = {name: [round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)] for name, v in ts.items()}
    n_run = len(next(iter(ts.values())))
    if n_run < reps:
        out["reps_run_" + next(iter(legs))] = n_run         # (the group is named by its first leg)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "residual_scales", "bench.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--budget", type=float, default=20.0, help="seconds after which a group of alternated legs stops repeating")
    ap.add_argument("--sizes", default=",".join(str(n) for n in SIZES))
    ap.add_argument("--blocks", type=int, default=24)
    ap.add_argument("--levels", default="2,4,8", help="logistic noise width per channel, in grey levels")
    ap.add_argument("--kodak", type=int, default=24, help="images of the Kodak-size row (0: none)")
    ap.add_argument("--host-limit", type=float, default=4e8, help="pixels x candidates above which a host leg is not run")
    ap.add_argument("--box", default="", help="the machine this runs on, in words (written into the file)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_residual_scales.py measures a GPU: none here")
    from config3_harness import build_model
    from irec.io import residual as R
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    model = build_model(device, args.blocks)
    levels = torch.tensor([float(v) for v in args.levels.split(",")], device=device).reshape(1, 3, 1, 1)
    g = torch.Generator().manual_seed(7)
    sizes_run = [int(v) for v in args.sizes.split(",")]
    result = {"box": args.box, "device": torch.cuda.get_device_name(0), "arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", ""),
              "host_cpus_available": len(os.sched_getaffinity(0)), "torch": torch.__version__,
              "model": f"{args.blocks}-block RVAE shim, 32x32 images, B=20 Omega=3 eps=0.2, block_size 1000", "reps": args.reps,
              "warmup": args.warmup, "budget_s": args.budget, "unit": "ms per call: [median, min, max]", "stream_len": R.DEFAULT_STREAM_LEN,
              "images": f"reconstruction of a noise image, quantised, plus logistic noise of {args.levels} grey levels per channel",
              "not_measured": [f"n_images {n}: not among --sizes of this run" for n in SIZES if n not in sizes_run], "rows": [], "kodak_row": None}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")

    def make_images(n):
        parts = []
        for lo in range(0, n, CHUNK):
            m = min(CHUNK, n - lo)
            noise = torch.randint(0, 256, (m, 3, 32, 32), generator=g, dtype=torch.uint8).to(device)
            recon = model.compress_lossless(noise, SEED)[4]
            u = torch.rand(recon.shape, generator=g).clamp_(1e-6, 1 - 1e-6).to(device)
            x = torch.floor((recon + 0.5) * 256) + torch.round(levels * (torch.log(u) - torch.log1p(-u)))
            parts.append(x.clamp_(0, 255).to(torch.uint8))
        return torch.cat(parts)

    def scale_bits_legs(pixels, loc, row, who):
        """leg (b) on CUDA (pixels, loc)."""
        n_px = pixels.numel()
        px_h, loc_h = pixels.cpu().numpy(), loc.cpu().numpy()
        for n_cand in (1, 64):
            cand = np.exp(np.linspace(-9.0, 1.0, n_cand)).astype(np.float32) if n_cand > 1 else np.float32([0.05])
            cand_d = torch.from_numpy(np.broadcast_to(cand, (3, n_cand)).copy()).to(device)
            legs = {f"scale_bits_device_{n_cand}": lambda: R.scale_bits_device(pixels, loc, cand_d)}
            want = R.scale_bits_device(pixels, loc, cand_d)[0].cpu().numpy()
            for threads in (16, 1):
                name = f"scale_bits_host{threads}_{n_cand}"
                if n_px * n_cand / threads > args.host_limit:
                    result["not_measured"].append(f"{who}: {name} ({n_px} pixels x {n_cand} candidates on {threads} thread(s): above --host-limit)")
                    continue
                legs[name] = lambda threads=threads: R.scale_bits(pixels.cpu().numpy(), loc.cpu().numpy(), cand, n_threads=threads)
                row.setdefault("device_equals_host", True)
                row["device_equals_host"] &= bool(np.array_equal(R.scale_bits(px_h, loc_h, cand, n_threads=threads)[0], want))
            row.update(alternate_ms(legs, args.reps, args.warmup, args.budget, rewarm=(f"scale_bits_device_{n_cand}",)))

    for n in sizes_run:
        images = make_images(n)
        model.set_likelihood_scales(None)
        with torch.no_grad():
            model.likelihood_log_scale.fill_(0.0)
        locs = torch.cat([model._lossless_rec(images[lo:lo + CHUNK], SEED)[2] for lo in range(0, n, CHUNK)])
        row = {"n_images": n}

        def sizes_at(tag):
            scale = model.residual_scale()
            blob, off = R.encode_residuals_device(images, locs, scale)
            assert torch.equal(R.decode_residuals_device(blob, off, locs, scale), images)
            row[f"res_bytes_per_image_{tag}"] = round(int(off[-1]) / n, 2)
            row[f"model_bits_per_image_{tag}"] = round(float(R.residual_model_bits_device(images, locs, scale).sum()) / n, 2)
            return blob, off

        # (d), and the fits whose result (a) codes with
        sizes_at("log_scale_0")
        pairs = [(images[lo:lo + CHUNK], locs[lo:lo + CHUNK]) for lo in range(0, n, CHUNK)]
        single = R.fit_scales(pairs, start=0.0)[0]
        channels = R.fit_scales(pairs, per_channel=True, start=0.0)[0]
        row["fitted_log_scale"], row["fitted_log_scales"] = round(single, 5), [round(float(v), 5) for v in channels]
        with torch.no_grad():
            model.likelihood_log_scale.fill_(single)
        s1 = model.likelihood_scale()
        blob1, off1 = sizes_at("fitted_single")
        model.set_likelihood_scales(channels)
        s3 = model.likelihood_scales()
        blob3, off3 = sizes_at("fitted_per_channel")
        # (a) version 2 against version 1 on the same tensors
        row.update(alternate_ms({"v1_encode": lambda: R.encode_residuals_device(images, locs, s1),
                                 "v2_encode": lambda: R.encode_residuals_device(images, locs, s3),
                                 "v1_decode": lambda: R.decode_residuals_device(blob1, off1, locs, s1, stream_len=R.DEFAULT_STREAM_LEN),
                                 "v2_decode": lambda: R.decode_residuals_device(blob3, off3, locs, s3, stream_len=R.DEFAULT_STREAM_LEN)},
                                args.reps, args.warmup, args.budget))
        for k in ("encode", "decode"):
            row[f"v2_over_v1_{k}"] = round(row[f"v2_{k}"][0] / row[f"v1_{k}"][0], 3)
        scale_bits_legs(images, locs, row, f"n_images {n}")
        # (c)
        fits = alternate_ms({"fit_single": lambda: model.fit_likelihood_scale(images, SEED, batch=CHUNK),
                             "fit_per_channel": lambda: model.fit_likelihood_scale(images, SEED, per_channel=True, batch=CHUNK),
                             "fit_search_only_single": lambda: R.fit_scales(pairs, start=0.0),
                             "fit_search_only_per_channel": lambda: R.fit_scales(pairs, per_channel=True, start=0.0)},
                            args.reps, args.warmup, args.budget)
        row.update(fits)
        result["rows"].append(row)
        print(json.dumps(row), flush=True)
        save()
        del images, locs, pairs
        torch.cuda.empty_cache()

    if args.kodak:
        n, h, w = args.kodak, 512, 768
        loc = (torch.rand((n, 3, h, w), generator=g) * 0.9 - 0.45).to(device)
        u = torch.rand(loc.shape, generator=g).clamp_(1e-6, 1 - 1e-6).to(device)
        pixels = torch.floor((loc + 0.5) * 256 + levels * (torch.log(u) - torch.log1p(-u))).clamp_(0, 255).to(torch.uint8)
        del u
        row = {"n_images": n, "shape": [3, h, w], "images": "loc uniform in [-0.45, 0.45], pixels = loc + logistic noise of --levels; no model pass"}
        scale_bits_legs(pixels, loc, row, "kodak")
        pairs = [(pixels[lo:lo + 8], loc[lo:lo + 8]) for lo in range(0, n, 8)]
        row.update(alternate_ms({"fit_search_only_single": lambda: R.fit_scales(pairs, start=0.0),
                                 "fit_search_only_per_channel": lambda: R.fit_scales(pairs, per_channel=True, start=0.0)},
                                args.reps, args.warmup, args.budget))
        fitted = R.fit_scales(pairs, per_channel=True, start=0.0)[0]
        row["fitted_log_scales"] = [round(float(v), 5) for v in fitted]
        row["log_of_levels_over_256"] = [round(float(np.log(float(v) / 256.0)), 5) for v in args.levels.split(",")]
        result["not_measured"].append("kodak: fit_likelihood_scale with the model's passes (the 24-block model was not run at 512 x 768)")
        result["kodak_row"] = row
        print(json.dumps(row), flush=True)
        save()


if __name__ == "__main__":
    main()
