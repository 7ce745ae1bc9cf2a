#!/usr/bin/env python3
"""Empirical symbol tables against the default models: what the .rec files weigh and what the coder costs.  Writes
profiles/rec_tables/bench.json (or --out).  Diagnostic; needs a GPU.  Nothing here is promised in advance.

Per workload the model codes two disjoint image sets (different generator seeds): tables are fitted on the first
(irec.io.hist_rows on the device, irec.io.tables_from_histograms) and applied to the second.
  bytes   per image of the second set, split into header (28 + 16 R), count streams and index streams, under the default models, an
          index table alone, count tables alone, and both; the files under tables are read back and their rows compared first
  ms      medians of --reps runs after --warmup, [median, min, max], default models against both tables in the same run:
          device  irec.io.encode_files_device_ragged / decode_files_device_ragged as a caller sees them (their one read-back included)
          host    irec.io.encode_files_ragged / decode_files_ragged on 16 threads and on 1, from rows already on the host

Workloads: the 24-block RVAE shim of scripts/config3_harness.py, 300 images of 32 x 32; the two-level model of scripts/bench_lossy.py on
8 Kodak-size images at both of that script's head-weight scales (0.2: K = 1 per block; --high-scale, default 5.0, the scale its
search settled on in profiles/lossy/bench.json: a level-1 block takes 100 partitions or more)."""
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

SEED = 42


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


def split_bytes(blob, off, R):
    """Mean bytes per image: header, count streams, index streams (the header's own length words)."""
    n = len(off) - 1
    words = np.stack([np.frombuffer(blob[off[i] + 28:off[i] + 28 + 16 * R].tobytes(), dtype="<u4").reshape(4, R) for i in range(n)])
    header, counts, index = 28 + 16 * R, words[:, 1].sum(axis=1), words[:, 2].sum(axis=1)
    assert (header + counts + index == np.diff(off)).all()
    return {"total": round(float(np.diff(off).mean()), 2), "header": header, "count_streams": round(float(counts.mean()), 2),
            "index_streams": round(float(index.mean()), 2)}


def measure(name, fit_rows, apply_rows, shape, block_size, S, reps, warmup):
    from irec.io import SymbolTables, hist_rows, tables_from_histograms, utils as U
    (Kf, idxf, bpr), (K, idx, bpr2) = fit_rows, apply_rows
    assert list(bpr) == list(bpr2)
    R, n = len(bpr), K.shape[0]
    ncv = 2 * max(idxf.shape[2], idx.shape[2]) + 1
    hist = hist_rows(Kf, idxf, bpr, S, ncv)
    both = tables_from_histograms(hist)
    assert int(hist.numpy().rejected[0]) == 0
    variants = {"default": None, "index_table": SymbolTables(both.index_counts, None), "count_tables": SymbolTables(None, both.num_aux_var_counts),
                "both": both}
    K_h, idx_h = K.cpu().numpy(), idx.cpu().numpy()
    live = np.arange(idx_h.shape[2])[None, None, :] < K_h[..., None]
    row = {"workload": name, "n_images_fit": int(Kf.shape[0]), "n_images_applied": n, "blocks_per_res": [int(b) for b in bpr], "max_index": S,
           "K_applied": [int(K_h.min()), float(np.median(K_h)), int(K_h.max())], "count_symbols_per_image": int(K_h.shape[1]),
           "index_symbols_per_image": round(float(K_h.sum(axis=1).mean()), 1), "bytes_per_image": {}, "ms": {}}
    blobs = {}
    for v, t in variants.items():
        blob, off = U.encode_files_device_ragged(SEED, shape, block_size, K, idx, S, bpr, tables=t)
        hdr, K2, idx2 = U.decode_files_device_ragged(blob, off, bpr, idx.shape[2], tables=t)
        assert np.array_equal(K2.cpu().numpy(), K_h) and np.array_equal(np.where(live, idx2.cpu().numpy(), 0), np.where(live, idx_h, 0)), v
        blobs[v] = (blob, off, blob.cpu().numpy(), off.cpu().numpy())
        row["bytes_per_image"][v] = split_bytes(blobs[v][2], blobs[v][3], R)
        host_blob, host_off = U.encode_files_ragged(SEED, shape, block_size, K_h, idx_h, S, bpr, tables=t)
        assert np.array_equal(host_blob, blobs[v][2]) and np.array_equal(host_off, blobs[v][3]), v
    for v in ("default", "both"):
        t = variants[v]
        blob, off, blob_h, off_h = blobs[v]
        out = torch.empty(blob.numel() + 64, dtype=torch.uint8, device=blob.device)
        ms = {"device_encode": median_ms(lambda: U.encode_files_device_ragged(SEED, shape, block_size, K, idx, S, bpr, out=out, tables=t), reps, warmup),
              "device_decode": median_ms(lambda: U.decode_files_device_ragged(blob, off_h, bpr, idx.shape[2], tables=t), reps, warmup)}
        for threads in (16, 1):
            ms[f"host_encode_{threads}"] = median_ms(lambda: U.encode_files_ragged(SEED, shape, block_size, K_h, idx_h, S, bpr, threads, tables=t),
                                                     reps, warmup)
            ms[f"host_decode_{threads}"] = median_ms(lambda: U.decode_files_ragged(blob_h, off_h, bpr, idx.shape[2], threads, tables=t), reps, warmup)
        row["ms"][v] = ms
    d, b = row["bytes_per_image"]["default"], row["bytes_per_image"]["both"]
    row["saved_bytes_per_image"] = {v: round(d["total"] - row["bytes_per_image"][v]["total"], 2) for v in ("index_table", "count_tables", "both")}
    row["saved_fraction_both"] = round(1 - b["total"] / d["total"], 4)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rec_tables", "bench.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--images", type=int, default=300)
    ap.add_argument("--kodak", type=int, default=8)
    ap.add_argument("--scale", type=float, default=0.2)
    ap.add_argument("--high-scale", type=float, default=5.0)
    ap.add_argument("--only", default=None, help="rvae or lossy")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rec_tables.py measures a GPU: none here")
    import irec
    from irec.coding.beam_search_coder import PendingCode
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    result = {"device": torch.cuda.get_device_name(0), "host_cpus_available": len(os.sched_getaffinity(0)), "torch": torch.__version__,
              "reps": args.reps, "warmup": args.warmup, "unit": "bytes per image (means); ms per call: [median, min, max]", "rows": []}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")

    if args.only in (None, "rvae"):
        from config3_harness import build_model
        model = build_model(device, 24)
        coder = model.residual_blocks[0].coder
        rows = []
        for gen_seed in (7, 8):                                       # two disjoint image sets
            g = torch.Generator().manual_seed(gen_seed)
            images = (torch.rand(args.images, 3, 32, 32, generator=g) - 0.5).to(device)
            _, (K, idx) = model.compress_rec(images, seed=SEED, return_pendings=True)
            m, R, bpt = K.shape
            rows.append((K.reshape(m, R * bpt).contiguous(), idx.reshape(m, R * bpt, -1).contiguous(), [bpt] * R))
        result["rows"].append(measure("rvae24_32x32", rows[0], rows[1], (32, 32, 3), coder.block_size, coder.n_samples, args.reps, args.warmup))
        save()
        del model
    if args.only in (None, "lossy"):
        from bench_lossy import model_at
        for setting, scale in (("low_K", args.scale), ("high_K", args.high_scale)):
            model = model_at(scale)
            sampler = irec.BeamSearchCoder(kl_per_partition=3., n_beams=10, extra_samples=1., block_size=1000)
            rows = []
            for gen_seed in (7, 8):
                g = torch.Generator().manual_seed(gen_seed)
                images = (torch.rand(args.kodak, 3, 512, 768, generator=g) - 0.5).to(device)
                with torch.no_grad():
                    (K, idx, bpr), _ = model._compress_gather(images, SEED, sampler, PendingCode.gather_packed_ragged_device)
                rows.append((K.contiguous(), idx.contiguous(), bpr))
            row = measure(f"two_level_kodak_{setting}", rows[0], rows[1], (512, 768, 3), 1000, model._max_index(sampler), args.reps, args.warmup)
            row["head_weight_scale"] = scale
            result["rows"].append(row)
            save()
            del model
    save()


if __name__ == "__main__":
    main()
