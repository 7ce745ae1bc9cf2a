#!/usr/bin/env python3
"""The two-level lossy shim (Large2LevelVAE, BASELINE configs[3]: B = 10, Omega = 3, S = 20, block_size 1000) end to end, images to .rec
files on disk and back, on three paths timed in ONE run on one box.  Writes profiles/lossy/bench.json (or --out).  Needs a GPU.

  list           the reference's surface, one image per call: compress(file_path, ...) -- nested Python lists, write_compressed_code --
                 and decompress(file_path, sampler)
  packed_host    compress_rec(images) -- one read-back of packed rows, irec_rec_encode_files_ragged on host threads -- the N files
                 written; the N files read, decompress_rec (irec_rec_decode_files_ragged on host threads, one upload of the rows)
  packed_device  the same with rec_on_device=True: the arithmetic coder runs on the device, one lane per stream

Per leg the median of --reps calls after --warmup calls, milliseconds for the whole batch of N images (host clock around a
synchronise).  Each at --scale 0.2 on the random-init head weights (K = 1 per block) and at --high-scale (default: searched, the first
scale at which a level-1 block takes 100 partitions or more -- the regime of a trained model at 0.2-1 bpp); the measured K range and
indices per image are reported.
Shapes: Kodak size (768 x 512: 13 + 302 blocks per image) at N = 1, 8, 24 and 64 x 64 crops (1 + 4 blocks) at N = 300.  Before anything
is timed the packed paths' files are compared byte for byte, and at N = 1 with the list path's.

--model 1: the same three paths for the one-level model (Large1LevelVAE, the lossy driver's default: one level of 48 x 32 x 192 latents,
295 blocks, on a Kodak-size image) on the Kodak-size shapes, written to profiles/lossy/bench_one_level.json; the search then looks at
the one level, and the rows' K_level_2 is null."""
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
sys.path[:0] = [ROOT, os.path.join(ROOT, "relative-entropy-coding_amd")]

SHAPES = [("kodak_1", 1, 512, 768), ("kodak_8", 8, 512, 768), ("kodak_24", 24, 512, 768), ("crops64_300", 300, 64, 64)]
SEED, BLOCK = 42, 1000
HIGH_LADDER = (1.5, 2., 2.5, 3., 3.5, 4., 5., 6., 8., 10., 12., 16.)


def median_ms(fn, reps, warmup):
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


def model_at(scale, levels=2):
    from irec.models import Large1LevelVAE, Large2LevelVAE
    torch.manual_seed(3)
    m = (Large2LevelVAE() if levels == 2 else Large1LevelVAE()).cuda().eval()
    heads = (m.analysis_transform[-1], m.hyper_analysis_transform[-1], m.hyper_synthesis_transform[-1], m._prior_loc_head,
             m._prior_log_scale_head, m._level_1_posterior_loc_combiner, m._level_1_posterior_log_scale_combiner) if levels == 2 else \
        (m.analysis_transform[-1], m._prior_loc_head, m._prior_log_scale_head)
    with torch.no_grad():
        for mod in heads:
            mod.weight.mul_(scale)
    return m


def write_files(blob, off, paths):
    if hasattr(blob, "cpu"):
        blob, off = blob.cpu().numpy(), off.cpu().numpy()
    mv = memoryview(blob)
    for i, path in enumerate(paths):
        with open(path, "wb") as fh:
            fh.write(mv[off[i]:off[i + 1]])


def read_files(paths):
    datas = [open(p, "rb").read() for p in paths]
    return np.frombuffer(b"".join(datas), dtype=np.uint8), np.concatenate([[0], np.cumsum([len(d) for d in datas])]).astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", type=int, choices=(1, 2), default=2, help="the levels of the model: Large2LevelVAE, or Large1LevelVAE")
    ap.add_argument("--out", default=None, help="default: profiles/lossy/bench.json, bench_one_level.json with --model 1")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=0.2)
    ap.add_argument("--high-scale", type=float, default=None,
                    help="default: the first scale of HIGH_LADDER at which a level-1 block of one Kodak-size image takes >= 100 partitions")
    ap.add_argument("--only", default=None, help="one shape by name")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lossy.py measures a GPU: none here")
    import irec
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "lossy", "bench.json" if args.model == 2 else "bench_one_level.json")
    shapes = SHAPES if args.model == 2 else SHAPES[:3]
    rows, search = [], []
    if args.high_scale is None:                  # the random-init weights have no natural scale: find the one that gives a trained model's K
        g = torch.Generator().manual_seed(11)
        probe = (torch.rand(1, 3, 512, 768, generator=g) - 0.5).cuda()
        for scale in HIGH_LADDER:
            K, _, bpr, _ = model_at(scale, args.model).compress_packed(probe, SEED, irec.BeamSearchCoder(kl_per_partition=3., n_beams=10, extra_samples=1.,
                                                                                            block_size=BLOCK))
            K_1 = K[:, sum(bpr[:-1]):]                                 # (level 1: the last residual block of the file)
            search.append({"head_weight_scale": scale, "K_level_1": [int(K_1.min()), int(np.median(K_1)), int(K_1.max())]})
            print(json.dumps(search[-1]), flush=True)
            if K_1.max() >= 100:
                args.high_scale = scale
                break
        if args.high_scale is None:
            raise SystemExit("no scale of HIGH_LADDER gave a level-1 block 100 partitions: pass --high-scale")
    out_dir = tempfile.mkdtemp(prefix="irec_lossy_")
    for setting, scale in (("low_K", args.scale), ("high_K", args.high_scale)):
        m = model_at(scale, args.model)
        sampler = irec.BeamSearchCoder(kl_per_partition=3., n_beams=10, extra_samples=1., block_size=BLOCK)
        S = m._max_index(sampler)
        for name, n, h, w in shapes:
            if args.only and args.only != name:
                continue
            g = torch.Generator().manual_seed(11)
            images = (torch.rand(n, 3, h, w, generator=g) - 0.5).cuda()
            hwc = [images[i].permute(1, 2, 0).contiguous() for i in range(n)]
            shape = (n, 3, h, w)
            paths = {leg: [os.path.join(out_dir, f"{leg}_{i}.rec") for i in range(n)] for leg in ("list", "packed_host", "packed_device")}

            def list_compress():
                for i in range(n):
                    m.compress(paths["list"][i], hwc[i], seed=SEED, sampler=sampler, block_size=BLOCK, max_index=S)

            def list_decompress():
                for i in range(n):
                    m.decompress(paths["list"][i], sampler)

            def packed_compress(leg, on_device):
                blob, off, _ = m.compress_rec(images, SEED, sampler, block_size=BLOCK, rec_on_device=on_device)
                write_files(blob, off, paths[leg])

            def packed_decompress(leg, on_device, max_K):
                blob, off = read_files(paths[leg])
                if on_device:
                    blob = torch.from_numpy(blob.copy()).cuda()
                m.decompress_rec(blob, off, SEED, shape, sampler, max_K=max_K, rec_on_device=on_device)

            # the three paths' files, compared before anything is timed
            K, idx, bpr, _ = m.compress_packed(images, SEED, sampler)
            packed_compress("packed_host", False)
            packed_compress("packed_device", True)
            m.compress(paths["list"][0], hwc[0], seed=SEED, sampler=sampler, block_size=BLOCK, max_index=S)
            if n == 1:                                   # (a batch may change convolution bits: the list path's file is compared at N = 1)
                assert open(paths["packed_host"][0], "rb").read() == open(paths["list"][0], "rb").read(), name
            assert all(open(a, "rb").read() == open(b, "rb").read() for a, b in zip(paths["packed_host"], paths["packed_device"])), name
            max_K = max(int(K.max()), 1)
            first_rows = [0, sum(bpr[:-1])]                                  # (level 1 is the last residual block of the file; one level: all of it)
            row = {"model": type(m).__name__, "setting": setting, "head_weight_scale": scale, "shape": name, "n_images": n, "height": h, "width": w, "blocks_per_res": bpr,
                   "K_level_2": [int(K[:, :first_rows[1]].min()), int(K[:, :first_rows[1]].max())] if args.model == 2 else None,
                   "K_level_1": [int(K[:, first_rows[1]:].min()), int(K[:, first_rows[1]:].max())], "K_level_1_median": int(np.median(K[:, first_rows[1]:])),
                   "indices_per_image": int(K.sum()) // n, "file_bytes_per_image": sum(os.path.getsize(p) for p in paths["packed_host"]) // n,
                   "reps": args.reps, "unit": "ms per batch: [median, min, max]"}
            row["list_compress"] = median_ms(list_compress, args.reps, args.warmup)
            row["list_decompress"] = median_ms(list_decompress, args.reps, args.warmup)
            for leg, on_device in (("packed_host", False), ("packed_device", True)):
                row[f"{leg}_compress"] = median_ms(lambda: packed_compress(leg, on_device), args.reps, args.warmup)
                row[f"{leg}_decompress"] = median_ms(lambda: packed_decompress(leg, on_device, max_K), args.reps, args.warmup)
            rows.append(row)
            print(json.dumps(row), flush=True)
            for ps in paths.values():
                for p in ps:
                    if os.path.exists(p):
                        os.remove(p)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "host_threads_available": len(os.sched_getaffinity(0)), "high_scale_search": search, "rows": rows}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
