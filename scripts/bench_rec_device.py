#!/usr/bin/env python3
"""The .rec leg of a batch, host against device: what it costs to turn a batch's indices (on the device) into its files' bytes, and
back.  Writes profiles/rec_device/bench.json (or --out).  Diagnostic; needs a GPU.

Per shape, medians over --reps runs after --warmup runs, milliseconds:
  host    the path of irec.io.encode_files: ONE device-to-host copy of the joined K / idx rows, then irec_rec_encode_files on
          n_threads = 1 and 16 host threads (host clock; the copy ends in a synchronise); back: irec_rec_decode_files, then K / idx copied up
  device  irec.io.encode_files_device / decode_files_device as a caller sees them (host clock, their one read-back of offsets and
          status included), and their launches alone between two device events
  blob    the files' bytes copied to the host (after a device encode) / to the device (before a device decode)
The device's bytes are compared with the host's at every shape before anything is timed.

Shapes: one GPU's share of config 3 (38 images x 24 residual blocks x 9 blocks, K uniform in 6..10 as the shim's random-init model
gives, max_K 16, max_index 36), 300 and 4096 such images, and one Kodak-like image (R = 2, 302 blocks of 180..236 indices at
max_index 20: one lane walks ~60 000 symbols)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "relative-entropy-coding_amd")]

SHAPES = [("config3_share_38", 38, 24, 9, 6, 10, 16, 36), ("images_300", 300, 24, 9, 6, 10, 16, 36),
          ("images_4096", 4096, 24, 9, 6, 10, 16, 36), ("kodak_like_1", 1, 2, 302, 180, 236, 240, 20)]


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
    return round(statistics.median(ts), 4), round(min(ts), 4), round(max(ts), 4)


def event_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return round(statistics.median(ts), 4), round(min(ts), 4), round(max(ts), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rec_device", "bench.json"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default=None, help="one shape by name")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rec_device.py measures a GPU: none here")
    from irec.io import utils as U
    rows = []
    for name, n, R, bpt, k_lo, k_hi, mk, S in SHAPES:
        if args.only and args.only != name:
            continue
        rng = np.random.default_rng(3)
        K = rng.integers(k_lo, k_hi + 1, (n, R, bpt)).astype(np.int32)
        idx = rng.integers(0, S, (n, R, bpt, mk)).astype(np.int32)
        both = torch.from_numpy(np.concatenate([K[..., None], idx], axis=3)).cuda()        # the joined rows, as gather_packed has them
        Kd, idxd = both[..., 0], both[..., 1:]
        reps = args.reps if n <= 300 else max(3, args.reps // 3)
        meta = (42, (32, 32, 3), 1000)
        blob_h, off_h = U.encode_files(*meta, K, idx, S)
        blob_d, off_d = U.encode_files_device(*meta, Kd, idxd, S)
        assert np.array_equal(blob_d.cpu().numpy(), blob_h) and np.array_equal(off_d.cpu().numpy(), off_h), name
        hdr_d, K_d, idx_d = U.decode_files_device(blob_d, off_h, R, bpt, mk)
        live = np.arange(mk)[None, None, None, :] < K[..., None]
        assert np.array_equal(K_d.cpu().numpy(), K) and np.array_equal(idx_d.cpu().numpy(), np.where(live, idx, 0)), name
        row = {"shape": name, "n_images": n, "n_res_blocks": R, "blocks_per_res": bpt, "max_K": mk, "max_index": S,
               "indices": int(K.sum()), "file_bytes": int(off_h[-1]), "reps": reps, "unit": "ms: [median, min, max]"}

        def host_encode(threads):
            h = both.cpu().numpy()
            U.encode_files(*meta, h[..., 0], h[..., 1:], S, n_threads=threads)

        def host_decode(threads):
            _, K2, i2 = U.decode_files(blob_h, off_h, R, bpt, mk, n_threads=threads)
            torch.from_numpy(K2).cuda(), torch.from_numpy(np.ascontiguousarray(i2)).cuda()

        row["host_index_copy_d2h"] = median_ms(lambda: both.cpu(), reps, args.warmup)
        for t in (1, 16):
            row[f"host_encode_copy_plus_{t}_threads"] = median_ms(lambda: host_encode(t), reps, args.warmup)
            row[f"host_decode_{t}_threads_plus_copy_up"] = median_ms(lambda: host_decode(t), reps, args.warmup)
        out = torch.empty(int(off_h[-1]), dtype=torch.uint8, device="cuda")
        row["device_encode_call"] = median_ms(lambda: U.encode_files_device(*meta, Kd, idxd, S, out=out), reps, args.warmup)
        row["device_encode_launches"] = event_ms(lambda: U._encode_files_device_launch(*meta, Kd, idxd, S, out), reps, args.warmup)
        row["device_decode_call"] = median_ms(lambda: U.decode_files_device(blob_d, off_h, R, bpt, mk), reps, args.warmup)
        row["device_decode_launches"] = event_ms(lambda: U._decode_files_device_launch(blob_d, off_h, R, bpt, mk), reps, args.warmup)
        row["blob_copy_d2h"] = median_ms(lambda: blob_d.cpu(), reps, args.warmup)
        blob_t = torch.from_numpy(blob_h)
        row["blob_copy_h2d"] = median_ms(lambda: blob_t.cuda(), reps, args.warmup)
        rows.append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "host_threads_available": len(os.sched_getaffinity(0)), "rows": rows}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
