"""Timing of the sequential importance coder -- GaussianCoder(sampler=ImportanceSampler(coding_bits, alpha)) -- on RVAE-shaped
latents ([16, 16, 32] tensors cut at block_size = 1000: eight blocks of 1000 dims and one of 192 per tensor).

Shapes: a batch of 64 tensors (576 blocks) at S = 21 and S = 404; one tensor (9 blocks, latency) at S = 21 and S = 1024; the decoder
on the same.  Device figures: HIP events around the whole device call (block KL, ordering by K, encode launch; tables cached, as in a
run over many images with one seed), every shape warmed first, at least --seconds timed per shape.  Before a shape is timed its
indices and sample are compared with the numpy referee (tests/gc_referee.py) at the timed size.
The yardstick is the HOST PATH on the same inputs on the same box: the reference's loop over ImportanceSampler.coded_sample on CPU
tensors (what the reference itself does), timed in this script -- on the first --host-tensors tensors of a shape where the whole
shape would take minutes (the figure is then scaled by blocks; `host_blocks_timed` says so).

--alpha A [A ...]: the sampler's alpha (default inf: the arg-max of the weights; finite: the Gumbel-max branch, whose yardstick is
the host loop at the same alpha).  Every shape is run once per alpha, in the order given; the rows say which.  With a finite alpha
among them the default output is profiles/gc_importance/bench_alpha.json: `--alpha 1 inf` times the alpha = inf rows in the same run
on the same box, to lie beside bench.json.

Usage: python scripts/bench_gc_importance.py [--alpha 1 inf] [--out FILE] [--seconds 0.5] [--only NAME] [--no-host]
`--only NAME --no-host --no-check` is the form to run under a kernel profiler (one shape, device work only)."""
import argparse
import functools
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "relative-entropy-coding_amd"), os.path.join(ROOT, "tests")]
import irec  # noqa: E402
from oracle import oracle as O  # noqa: E402
import gc_referee as R  # noqa: E402
import gc_referee_alpha as RA  # noqa: E402

OMEGA, SEED, BLOCK_SIZE, N = 3.0, 42, 1000, 8192
SHAPES = [("batch64_S21", 64, 21), ("batch64_S404", 64, 404), ("tensor_S21", 1, 21), ("tensor_S1024", 1, 1024)]


class Dist:
    def __init__(self, loc, scale):
        self.loc, self.scale = loc, scale


class CachedOracle:
    def __init__(self):
        self.tf_random_normal = functools.lru_cache(maxsize=64)(O.tf_random_normal)

    def __getattr__(self, name):
        return getattr(O, name)


def latents(n_tensors):
    stats = [O.synthetic_latent(9000 + i, N) for i in range(n_tensors)]
    return [np.stack([s[j] for s in stats]).reshape(n_tensors, 16, 16, 32) for j in range(4)]


def timed(fn, seconds):
    """Mean milliseconds of fn() by device events: runs of 1, 2, 4, ... calls until one run lasts `seconds`."""
    reps = 1
    while True:
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(reps):
            fn()
        stop.record()
        stop.synchronize()
        ms = start.elapsed_time(stop)
        if ms >= seconds * 1e3:
            return ms / reps, reps
        reps *= 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--alpha", type=float, nargs="+", default=[float("inf")])
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--only", default=None)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--host-tensors", type=int, default=2)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "gc_importance", "bench_alpha.json" if np.isfinite(a.alpha).any() else "bench.json")
    eng = irec.get_engine()
    plan = eng.plan(eng.params(3.0, 36, 20), eng.layout(1, 192, 192, 42), 8)
    n_cu, clock_mhz = plan["n_cu"], plan["clock_mhz"]
    rows = []
    for alpha, (name, n_tensors, S) in ((al, sh) for al in a.alpha for sh in SHAPES):
        if a.only and name != a.only:
            continue
        bits = float(np.log2(S - 0.5))
        coder = irec.GaussianCoder(kl_per_partition=OMEGA, sampler=irec.ImportanceSampler(coding_bits=bits, alpha=alpha),
                                   block_size=BLOCK_SIZE)
        coder.table_steps = coder._max_K_hint = 16
        assert coder.sampler.n_samples() == S
        host = latents(n_tensors)
        dev = [torch.from_numpy(h).cuda() for h in host]
        t0 = time.perf_counter()
        idx, z = coder.encode(Dist(dev[0], dev[1]), Dist(dev[2], dev[3]), SEED, batched=True)     # warm-up: builds the tables
        torch.cuda.synchronize()
        first_call_s = time.perf_counter() - t0
        lay = eng.layout(n_tensors, N, BLOCK_SIZE, SEED)
        dims = lay.block_dim.cpu().numpy()[lay.natural].reshape(n_tensors, -1)
        elements = int(sum(len(ix) * S * int(dims[i, j]) for i, b in enumerate(idx) for j, ix in enumerate(b)))
        checked = 0
        if not a.no_check:
            orc, zh = CachedOracle(), z.cpu().numpy()
            for i in range(n_tensors):
                if np.isfinite(alpha):
                    ridx, rz = RA.encode_tensor(*(h[i] for h in host), SEED, S, OMEGA, BLOCK_SIZE, orc, alpha)
                else:
                    ridx, rz = R.encode_tensor(*(h[i] for h in host), SEED, S, OMEGA, BLOCK_SIZE, orc)
                assert [[int(v) for v in ix] for ix in idx[i]] == ridx, (name, i)
                assert np.array_equal(zh[i], rz), (name, i)
                checked += len(ridx)
        enc_ms, enc_reps = timed(lambda: coder.encode_tensors_device(dev[0], dev[1], dev[2], dev[3], SEED, BLOCK_SIZE), a.seconds)
        dec = coder.decode(Dist(dev[2], dev[3]), idx, SEED, batched=True)
        assert torch.equal(dec, z)
        ql, qs, pl, ps = (t.reshape(n_tensors, -1).contiguous() for t in dev)
        K, ix_dev, _ = eng.gc_encode_blocks(lay, ql, qs, pl, ps, SEED, OMEGA, S, 16, alpha=alpha)
        dec_ms, dec_reps = timed(lambda: eng.gc_decode_blocks(lay, pl, ps, SEED, S, K, ix_dev), a.seconds)
        row = {"shape": name, "alpha": alpha if np.isfinite(alpha) else "inf", "tensors": n_tensors, "blocks": int(lay.n_blocks), "n_samples": S, "indices": int(sum(len(ix) for b in idx for ix in b)),
               "elements_K_S_D": elements, "blocks_checked_against_referee": checked, "first_call_with_table_build_s": round(first_call_s, 4),
               "device_encode_ms": round(enc_ms, 4), "device_encode_calls_timed": enc_reps,
               "device_decode_ms": round(dec_ms, 4), "device_decode_calls_timed": dec_reps,
               "encode_elements_per_cu_per_clock": round(elements / (enc_ms * 1e-3) / n_cu / (clock_mhz * 1e6), 4)}
        if not a.no_host:
            n_host = min(n_tensors, a.host_tensors if (S > 21 and n_tensors > 1) else n_tensors)
            cpu = [torch.from_numpy(h[:n_host]) for h in host]
            t0 = time.perf_counter()
            hidx, hz = coder.encode(Dist(cpu[0], cpu[1]), Dist(cpu[2], cpu[3]), SEED, batched=True)
            host_enc_s = time.perf_counter() - t0
            t0 = time.perf_counter()
            hdec = coder.decode(Dist(cpu[2], cpu[3]), hidx, SEED, batched=True)
            host_dec_s = time.perf_counter() - t0
            assert [[int(v) for v in ix] for b in hidx for ix in b] == [[int(v) for v in ix] for b in idx[:n_host] for ix in b], name
            assert torch.equal(hz, z[:n_host].cpu()) and torch.equal(hdec, hz)
            scale = n_tensors / n_host
            row.update({"host_blocks_timed": n_host * 9, "host_encode_ms": round(host_enc_s * 1e3 * scale, 2),
                        "host_decode_ms": round(host_dec_s * 1e3 * scale, 2),
                        "host_scaled_from_subset": scale != 1.0,
                        "encode_speedup_over_host": round(host_enc_s * 1e3 * scale / enc_ms, 1),
                        "decode_speedup_over_host": round(host_dec_s * 1e3 * scale / dec_ms, 1)})
        print(json.dumps(row), flush=True)
        rows.append(row)
    out = {"what": "sequential importance coder (irec_gc_importance_encode[_gumbel] / _decode) vs the host path on the same inputs at the "
                   "same alpha, same box",
           "device": torch.cuda.get_device_name(0), "n_cu": n_cu, "clock_mhz": clock_mhz, "omega": OMEGA, "block_size": BLOCK_SIZE,
           "tensor_dims": N, "seconds_per_shape": a.seconds, "rows": rows}
    if not a.only:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
