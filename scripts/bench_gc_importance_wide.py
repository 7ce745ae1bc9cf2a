"""Timing of the sequential importance coder on blocks of MORE than 1024 dims (gc_importance_encode_wide_kernel, csrc/irec_gc.hip):
the `GaussianCoder.encode` call on GPU tensors, synchronised, wall clock, median over --runs calls after a warm-up.

Shapes (RVAE-shaped latents of 8192 dims, Omega = 3, S = 21 unless named):
  tensor_bsNone        one block of 8192 dims (block_size=None, the reference's default for Coder)
  batch64_bsNone       64 such tensors in one batched call
  tensor_bs3000        one tensor cut at block_size=3000 (blocks of 3000, 3000 and 2192 dims)
  tensor_bs3000_S256   the same at S = 256 (for the tile form against the plain walk)
Warm: the same seed every call -- the normal tables are cached, the reference drivers' case.  Cold: a new seed per call -- the host
builds and uploads the tables; `table_build_ms` times exactly that on its own (Engine.normal_tables with a fresh seed, synchronised) and
`table_share_of_cold` is its share of the cold call.

One process measures one build, named by --label:
  (default)            the product library of this checkout
  --lib NAME           a diagnostic build, csrc/variants/NAME.so (`make -C csrc variant_gc NAME=gc_plain DEFS=-DIREC_GC_WIDE_TILE=0`:
                       the plain lane-per-sample walk at every S)
  --tree PATH          ANOTHER checkout, built (the parent commit, where these calls take the host loop: the baseline)
Each writes --out; `--merge A.json B.json ...` joins them into one file with the warm speed-ups over the rows labelled `baseline`.
A cell stops early after --cell-seconds (never before 3 calls): the host loop codes a batch of 64 in most of a minute; `runs` says how
many calls a median is over.

Usage: python scripts/bench_gc_importance_wide.py --label tile --out profiles/gc_importance/bench_wide_tile.json"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

HERE_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OMEGA, SEED, N = 3.0, 42, 8192
SHAPES = [("tensor_bsNone", 1, None, 21), ("batch64_bsNone", 64, None, 21), ("tensor_bs3000", 1, 3000, 21),
          ("tensor_bs3000_S256", 1, 3000, 256)]


class Dist:
    def __init__(self, loc, scale):
        self.loc, self.scale = loc, scale


def median_ms(fn, runs, cell_seconds):
    out, t_start = [], time.perf_counter()
    while len(out) < runs and (len(out) < 3 or time.perf_counter() - t_start < cell_seconds):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), len(out)


def merge(paths, out_path):
    rows, meta = [], {}
    for p in paths:
        with open(p) as fh:
            part = json.load(fh)
        meta = {k: v for k, v in part.items() if k != "rows"}
        rows += part["rows"]
    base = {r["shape"]: r for r in rows if r["label"] == "baseline"}
    for r in rows:
        b = base.get(r["shape"])
        if b is not None and r["label"] != "baseline":
            r["warm_speedup_over_baseline"] = round(b["warm_ms"] / r["warm_ms"], 2)
            if r.get("cold_ms") and b.get("cold_ms"):
                r["cold_speedup_over_baseline"] = round(b["cold_ms"] / r["cold_ms"], 2)
    meta["rows"] = rows
    with open(out_path, "w") as fh:
        json.dump(meta, fh, indent=1)
    print("wrote", out_path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE_ROOT, "profiles", "gc_importance", "bench_wide.json"))
    ap.add_argument("--label", default="tile")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--tree", default=None)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--cell-seconds", type=float, default=60.0)
    ap.add_argument("--only", default=None)
    ap.add_argument("--no-cold", action="store_true")
    ap.add_argument("--merge", nargs="+", default=None)
    a = ap.parse_args()
    if a.merge:
        return merge(a.merge, a.out)
    root = os.path.abspath(a.tree) if a.tree else HERE_ROOT
    sys.path[:0] = [root, os.path.join(root, "relative-entropy-coding_amd")]
    import irec
    from oracle import oracle as O
    if a.lib:
        irec._lib.load(a.lib if os.path.sep in a.lib else os.path.join(root, "relative-entropy-coding_amd", "csrc", "variants", a.lib + ".so"))
    assert os.path.abspath(irec.__file__).startswith(root), irec.__file__
    eng = irec.get_engine()
    rows = []
    for name, n_tensors, bs, S in SHAPES:
        if a.only and name not in a.only.split(","):
            continue
        stats = [O.synthetic_latent(9000 + i, N) for i in range(n_tensors)]
        dev = [torch.from_numpy(np.stack([s[j] for s in stats]).reshape(n_tensors, 16, 16, 32)).cuda() for j in range(4)]
        coder = irec.GaussianCoder(kl_per_partition=OMEGA, sampler=irec.ImportanceSampler(coding_bits=float(np.log2(S - 0.5))), block_size=bs)
        assert coder.sampler.n_samples() == S

        def call(seed):
            return coder.encode(Dist(dev[0], dev[1]), Dist(dev[2], dev[3]), seed, batched=True)

        idx, _ = call(SEED)                           # warm-up: raises the coder's window to the blocks' K, builds the tables
        path = coder.last_path
        if path == "device":
            call(SEED)
        torch.cuda.synchronize()
        K = [len(ix) for b in idx for ix in (b if bs is not None else [b])]
        warm_ms, warm_runs = median_ms(lambda: call(SEED), a.runs, a.cell_seconds)
        row = {"label": a.label, "shape": name, "tensors": n_tensors, "block_size": bs, "n_samples": S, "path": path,
               "blocks": len(K), "K_max": max(K), "indices": sum(K), "warm_ms": round(warm_ms, 3), "warm_runs": warm_runs}
        if not a.no_cold:
            seeds = iter(range(1000, 1000000, 97))
            cold_ms, cold_runs = median_ms(lambda: call(next(seeds)), a.runs, a.cell_seconds)
            row.update({"cold_ms": round(cold_ms, 3), "cold_runs": cold_runs})
            if path == "device":
                lay = eng.layout(n_tensors, N, bs, SEED)
                steps = max(coder.table_window(), coder._max_K_hint)
                tab_ms, _ = median_ms(lambda: eng.normal_tables(next(seeds), S, lay.distinct_dims, steps), 5, a.cell_seconds)
                row.update({"table_steps": steps, "table_build_ms": round(tab_ms, 3), "table_share_of_cold": round(tab_ms / cold_ms, 3)})
        print(json.dumps(row), flush=True)
        rows.append(row)
    out = {"what": "GaussianCoder.encode on GPU tensors, blocks of more than 1024 dims: wall clock of the synchronised call, median",
           "device": torch.cuda.get_device_name(0), "omega": OMEGA, "tensor_dims": N, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
