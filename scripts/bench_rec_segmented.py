#!/usr/bin/env python3
"""The segmented .rec container (NAME.recs) against the plain one, writing and reading, in ONE run on one box.
Writes profiles/rec_segmented/bench.json (or --out), a line per finished row to stdout.  Needs a GPU.

Part 1, the coders alone, over rows that one compress pass of the two-level lossy model left (scripts/bench_lossy.py's model, shapes and
head-weight scales: kodak_1 / 8 / 24 and crops64_300 at low and at high K), plus one GPU's share of config 3 (38 images x 24 residual
blocks x 9 blocks, K in [6, 10], max_index 36: scripts/bench_rec_device.py's synthetic rows).  Legs, each writing and reading:
  plain_host_1 / plain_host_16    irec.io.encode_files_ragged / decode_files_ragged on 1 and on 16 host threads (host rows, host clock)
  plain_device                    irec_rec_encode_files_device_ragged / decode: the launches alone, device rows, device events
  seg_host_16_g{4,16,64}          irec.io.encode_files_segmented / decode_files_segmented on 16 host threads
  seg_device_g{4,16,64}           irec_rec_encode_files_device_segmented / decode: the launches alone, device events
The legs are alternated: every repetition runs each leg once, in order; a leg's figure is the median of --reps after --warmup rounds.
Bytes per image are reported for the plain file and for every g.  Before anything is timed every segmented device file is compared
with the host's, and every reader's rows with the rows that went in.

Part 2, end to end: harness.compress_images_lossy / decompress_images_lossy (files on disk, read back and checked) with each of the four
coders -- plain host, plain device, segmented host, segmented device (--g-end-to-end, default 16) -- host clock around a synchronise."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "relative-entropy-coding_amd"), os.path.join(ROOT, "scripts")]

from bench_lossy import BLOCK, SEED, SHAPES, model_at  # noqa: E402

SEGMENT_BLOCKS = (4, 16, 64)


def alternated(legs, reps, warmup):
    """legs: {name: (fn, on_device)}.  Every round runs each leg once; {name: [median, min, max] ms} over the rounds after the warm-ups.
    A device leg is timed by a pair of events around its launches, a host leg by the host clock."""
    times = {name: [] for name in legs}
    for r in range(warmup + reps):
        for name, (fn, on_device) in legs.items():
            if on_device:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                ms = a.elapsed_time(b)
            else:
                t0 = time.perf_counter()
                fn()
                ms = (time.perf_counter() - t0) * 1e3
            if r >= warmup:
                times[name].append(ms)
    return {name: [round(statistics.median(ts), 4), round(min(ts), 4), round(max(ts), 4)] for name, ts in times.items()}


def coder_row(name, K, idx, bpr, S, shape_hw, reps, warmup):
    """Part 1 for rows K [N, T], idx [N, T, max_K] (numpy)."""
    from irec.io import segmented as SG
    from irec.io import utils as U
    n, mk = K.shape[0], idx.shape[2]
    h, w = shape_hw
    Kd, Id = torch.from_numpy(K).cuda(), torch.from_numpy(idx).cuda()
    zeroed = np.where(np.arange(mk)[None, None, :] < K[..., None], idx, 0)
    row = {"shape": name, "n_images": n, "blocks_per_res": [int(b) for b in bpr], "max_K": mk, "max_index": int(S), "indices_per_image": int(K.sum()) // n,
           "K_range": [int(K.min()), int(np.median(K)), int(K.max())], "reps": reps, "unit": "ms per call: [median, min, max]"}
    write, read = {}, {}
    plain, poff = U.encode_files_ragged(SEED, (h, w, 3), BLOCK, K, idx, S, bpr)
    row["plain_bytes_per_image"] = int(poff[-1]) // n
    plain_d, poff_d = torch.from_numpy(plain.copy()).cuda(), torch.from_numpy(poff.copy()).cuda()
    out = torch.empty(int(poff[-1]) + 64, dtype=torch.uint8, device="cuda")
    blob_d, off_d = U.encode_files_device_ragged(SEED, (h, w, 3), BLOCK, Kd, Id, S, bpr)
    assert np.array_equal(blob_d.cpu().numpy(), plain) and np.array_equal(U.decode_files_device_ragged(plain_d, poff, bpr, mk)[1].cpu().numpy(), K)
    for threads in (1, 16):
        write[f"plain_host_{threads}"] = (lambda t=threads: U.encode_files_ragged(SEED, (h, w, 3), BLOCK, K, idx, S, bpr, n_threads=t), False)
        read[f"plain_host_{threads}"] = (lambda t=threads: U.decode_files_ragged(plain, poff, bpr, mk, n_threads=t), False)
    write["plain_device"] = (lambda: U._encode_files_device_ragged_launch(SEED, (h, w, 3), BLOCK, Kd, Id, S, bpr, out), True)
    read["plain_device"] = (lambda: U._decode_files_device_ragged_launch(plain_d, poff_d, bpr, mk, on_device=True), True)
    keep = []
    for g in SEGMENT_BLOCKS:
        blob, off = SG.encode_files_segmented(SEED, (h, w, 3), BLOCK, K, idx, S, bpr, g, n_threads=16)
        row[f"seg_g{g}_bytes_per_image"] = int(off[-1]) // n
        row[f"seg_g{g}_segments_per_image"] = int(sum(-(-int(b) // g) for b in bpr))
        bd, od = SG.encode_files_device_segmented(SEED, (h, w, 3), BLOCK, Kd, Id, S, bpr, g)
        assert np.array_equal(bd.cpu().numpy(), blob) and np.array_equal(od.cpu().numpy(), off), (name, g)
        _, K2, idx2 = SG.decode_files_device_segmented(bd, od, bpr, mk, g)
        _, K3, idx3 = SG.decode_files_segmented(blob, off, bpr, mk, g)
        assert np.array_equal(K2.cpu().numpy(), K) and np.array_equal(idx2.cpu().numpy(), zeroed) and np.array_equal(K3, K) and np.array_equal(idx3, zeroed)
        out_g = torch.empty(int(off[-1]) + 64, dtype=torch.uint8, device="cuda")
        keep.append((blob, off, bd, od, out_g))
        write[f"seg_host_16_g{g}"] = (lambda g=g: SG.encode_files_segmented(SEED, (h, w, 3), BLOCK, K, idx, S, bpr, g, n_threads=16), False)
        read[f"seg_host_16_g{g}"] = (lambda g=g, b=blob, o=off: SG.decode_files_segmented(b, o, bpr, mk, g, n_threads=16), False)
        write[f"seg_device_g{g}"] = (lambda g=g, o=out_g: SG._encode_files_device_segmented_launch(SEED, (h, w, 3), BLOCK, Kd, Id, S, bpr, g, o), True)
        read[f"seg_device_g{g}"] = (lambda g=g, b=bd, o=od: SG._decode_files_device_segmented_launch(b, o, bpr, g, mk, on_device=True), True)
    row["write"] = alternated(write, reps, warmup)
    row["read"] = alternated(read, reps, warmup)
    return row


def end_to_end_row(m, sampler, images, g, reps, warmup, out_dir):
    """Part 2: compress_images_lossy / decompress_images_lossy with the four coders, the legs alternated."""
    from irec import harness
    n = images.shape[0]
    coders = {"plain_host": (False, None), "plain_device": (True, None), f"seg_host_g{g}": (False, g), f"seg_device_g{g}": (True, g)}
    dirs = {c: os.path.join(out_dir, c) for c in coders}
    names = [f"im{i}" for i in range(n)]

    def compress(c):
        on_device, seg = coders[c]
        rows = harness.compress_images_lossy(m, sampler, images, names, SEED, BLOCK, dirs[c], rec_on_device=on_device, segment_blocks=seg)
        torch.cuda.synchronize()
        return rows

    def decompress(c):
        on_device, seg = coders[c]
        ext = "rec" if seg is None else "recs"
        out = harness.decompress_images_lossy(m, sampler, [os.path.join(dirs[c], f"{nm}.{ext}") for nm in names], rec_on_device=on_device)
        torch.cuda.synchronize()
        return out
    back = {}
    for c in coders:                                     # checked before anything is timed
        assert all(r["indices_recovered"] for r in compress(c)), c
        back[c] = decompress(c)[0]
    assert all(torch.equal(back[c], back["plain_host"]) for c in coders)
    return {"compress_images_lossy": alternated({c: (lambda c=c: compress(c), False) for c in coders}, reps, warmup),
            "decompress_images_lossy": alternated({c: (lambda c=c: decompress(c), False) for c in coders}, reps, warmup)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rec_segmented", "bench.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=0.2)
    ap.add_argument("--high-scale", type=float, default=5.0, help="the scale scripts/bench_lossy.py's search found (profiles/lossy/bench.json): a level-1 block of >= 100 partitions")
    ap.add_argument("--g-end-to-end", type=int, default=16)
    ap.add_argument("--only", default=None, help="one shape by name")
    ap.add_argument("--skip-end-to-end", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rec_segmented.py measures a GPU: none here")
    import irec
    result = {"device": torch.cuda.get_device_name(0), "host_threads_available": len(os.sched_getaffinity(0)), "segment_blocks": list(SEGMENT_BLOCKS),
              "coders": [], "end_to_end": []}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")
    out_dir = tempfile.mkdtemp(prefix="irec_recs_")
    if not args.only or args.only == "config3_share_38":
        rng = np.random.default_rng(3)
        K = rng.integers(6, 11, (38, 24 * 9)).astype(np.int32)
        idx = rng.integers(0, 36, (38, 24 * 9, 16)).astype(np.int32)
        row = coder_row("config3_share_38", K, idx, [9] * 24, 36, (32, 32), args.reps, args.warmup)
        row["setting"] = "synthetic rows"
        result["coders"].append(row)
        print(json.dumps(row), flush=True)
        save()
    for setting, scale in (("low_K", args.scale), ("high_K", args.high_scale)):
        m = model_at(scale)
        sampler = irec.BeamSearchCoder(kl_per_partition=3., n_beams=10, extra_samples=1., block_size=BLOCK)
        S = m._max_index(sampler)
        for name, n, h, w in SHAPES:
            if args.only and args.only != name:
                continue
            g = torch.Generator().manual_seed(11)
            images = (torch.rand(n, 3, h, w, generator=g) - 0.5).cuda()
            K, idx, bpr, _ = m.compress_packed(images, SEED, sampler)
            row = coder_row(name, np.ascontiguousarray(K), np.ascontiguousarray(idx), bpr, S, (h, w), args.reps, args.warmup)
            row.update({"setting": setting, "head_weight_scale": scale, "height": h, "width": w})
            result["coders"].append(row)
            print(json.dumps(row), flush=True)
            save()
            if not args.skip_end_to_end:
                e2e = {"setting": setting, "shape": name, "n_images": n, "segment_blocks": args.g_end_to_end, "reps": args.reps,
                       "unit": "ms per batch, files written, read back and checked: [median, min, max]"}
                e2e.update(end_to_end_row(m, sampler, images, args.g_end_to_end, args.reps, args.warmup, out_dir))
                result["end_to_end"].append(e2e)
                print(json.dumps(e2e), flush=True)
                save()
    shutil.rmtree(out_dir, ignore_errors=True)


if __name__ == "__main__":
    main()
