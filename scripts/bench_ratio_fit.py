"""Timing of the auxiliary-variance ratio fit (GaussianCoder.update_auxiliary_variance_ratios, csrc/irec_fit.hip) on the
SURVEY §8d synthetic latents: one fit of 16 x 1000 and one of 512 x 1000 rows x dims at Omega = 3, three ways on the same box:

  device   irec_fit_aux_ratios: one launch per SGD iteration, `done` read every 64 launches
  host     irec_fit_aux_ratios_host at 16 threads (the same bits as the device path: asserted)
  eager    the loop a user could have written without the kernels: PyTorch on the GPU, float64, autograd, the reference's
           literal formulas (tests/ratio_fit_referee.py restated on device tensors), loss read back every iteration for the
           stop test.  Its ratios must agree with the device path's to 1e-5 (asserted; its hand-over is float64 where the contract's is float32); it is a
           yardstick, not a referee.

Wall-clock seconds per fit (time.perf_counter around the call, the device idle before and after; the device path's table of
normal draws is built and uploaded inside the call and is part of its figure, reported separately as well), best of --repeats.
Also: iterations per fit step, microseconds per iteration, and -- with --fold-stats DIR -- the per-kernel summary of a
`rocprofv3 --kernel-trace --stats` run of `--only device --size N` (a run of its own).

Usage: python scripts/bench_ratio_fit.py [--out profiles/ratio_fit/bench.json] [--repeats 3] [--only device|host|eager] [--size N]
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "relative-entropy-coding_amd"), os.path.join(ROOT, "tests")]
import irec  # noqa: E402
from irec.engine import build_normal_table, fit_aux_ratios_host  # noqa: E402
from oracle import oracle as O  # noqa: E402

OMEGA, SEED, DIM = 3.0, 42, 1000
SIZES = (16, 512)
TOL, LR, MAX_ITERS = 1e-4, 1e-3, 10000


def rows(n):
    lat = [O.synthetic_latent(20000 + i, DIM) for i in range(n)]
    return [np.ascontiguousarray(np.stack([r[j] for r in lat])) for j in range(4)]


def kl_normal(la, sa, lb, sb):
    d = torch.log(sa) - torch.log(sb)
    return 0.5 * (la / sb - lb / sb) ** 2 + 0.5 * torch.expm1(2. * d) - d


def eager_fit(stats, table):
    """coder.py:266-410 in eager PyTorch on the device, float64.  -> (ratios float32, iterations per step)."""
    tl, ts, cl, cs = (t.double() for t in stats)
    num = 1 + torch.floor(kl_normal(tl, ts, cl, cs).sum(1).float() / np.float32(OMEGA)).long()
    M = int(num.max())
    ratios, counts, iters = np.zeros(M, np.float32), np.zeros(M, np.float32), []
    ratios[0] = counts[0] = 1.
    for ratio in range(M, 1, -1):
        sel = torch.nonzero(num >= ratio)[:, 0]
        t_loc, t_scale, c_loc, c_scale = tl[sel], ts[sel], cl[sel], cs[sel]
        total = kl_normal(t_loc, t_scale, c_loc, c_scale).sum(1)
        init = ratios[ratio - 1] if ratios[ratio - 1] > 0 else ratios[ratio] if ratio < M else np.float32(1. / ratio)
        x0 = min(max(float(init), 1e-10), 1 - 1e-10)
        theta = torch.tensor(np.log(x0) - np.log(1 - x0), dtype=torch.float64, device=tl.device, requires_grad=True)
        c_var, t_var, rest, prev = c_scale ** 2, t_scale ** 2, OMEGA * (ratio - 1), float("inf")
        for it in range(MAX_ITERS):
            rho = torch.sigmoid(theta)
            aux_var = rho * c_var
            at_loc = (t_loc - c_loc) * aux_var / c_var
            at_var = t_var * aux_var ** 2 / c_var ** 2 + aux_var * (c_var - aux_var) / c_var
            aux_kl = kl_normal(at_loc, torch.sqrt(at_var), torch.zeros_like(c_loc), torch.sqrt(aux_var)).sum(1)
            loss = torch.mean(torch.where(aux_kl > OMEGA, (aux_kl - OMEGA) ** 2, torch.zeros_like(aux_kl)) +
                              torch.where(total - aux_kl > rest, ((total - aux_kl) - rest) ** 2, torch.zeros_like(aux_kl)))
            grad, = torch.autograd.grad(loss, theta)
            rho_eval = rho.detach()
            with torch.no_grad():
                theta -= LR * grad
            L = float(loss)
            if abs(prev - L) < TOL:
                break
            prev = L
        iters.append(it + 1)
        r_last = np.float32(float(rho_eval))
        n_el = np.float32(sel.numel())
        ratios[ratio - 1] = (ratios[ratio - 1] * counts[ratio - 1] + r_last * n_el) / (counts[ratio - 1] + n_el)
        counts[ratio - 1] += n_el
        a_last, a = float(r_last) * c_var, float(ratios[ratio - 1]) * c_var
        A = table[M - ratio][:, sel].T.double() * torch.sqrt(t_var * a_last ** 2 / c_var ** 2 + a_last * (c_var - a_last) / c_var) \
            + (t_loc - c_loc) * a_last / c_var
        den = t_var * a + c_var * (c_var - a)
        tl[sel] = c_loc + (A * t_var * c_var + (t_loc - c_loc) * (c_var - a) * c_var) / den
        ts[sel] = torch.sqrt(t_var * c_var * (c_var - a) / den)
        cl[sel] = c_loc + A
        cs[sel] = torch.sqrt(c_var - a)
    return ratios, iters


def best_of(fn, repeats):
    best, out = float("inf"), None
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best, out


def fold_stats(directory):
    """Rows of the fit kernels from a rocprofv3 --kernel-trace --stats run."""
    out = []
    for path in sorted(glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)):
        with open(path) as fh:
            for row in csv.DictReader(fh):
                if "fit_" in row.get("Name", ""):
                    out.append({k: row[k] for k in ("Name", "Calls", "TotalDurationNs", "AverageNs", "MinNs", "MaxNs", "Percentage") if k in row})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ratio_fit", "bench.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", default=None, choices=[None, "device", "host", "eager"])
    ap.add_argument("--size", type=int, default=None)
    ap.add_argument("--fold-stats", action="append", default=[], metavar="SIZE=DIR")
    a = ap.parse_args()
    eng = irec.get_engine()
    ones = np.ones(1, np.float32)
    result = {"what": "ratio fit (irec_fit_aux_ratios) vs its host twin at 16 threads vs an eager float64 PyTorch-on-GPU restatement",
              "device": torch.cuda.get_device_name(0), "omega": OMEGA, "dim": DIM, "relative_tolerance": TOL, "learning_rate": LR,
              "launch_chunk": 64, "rows": []}
    for n in SIZES:
        if a.size and n != a.size:
            continue
        host = rows(n)
        dev = [torch.from_numpy(h).cuda() for h in host]
        row = {"rows": n, "elements": n * DIM}
        dev_out = None
        if a.only in (None, "device"):
            eng.fit_aux_ratios(*dev, SEED, OMEGA, ones, ones, TOL, MAX_ITERS, LR)            # warm-up
            s, dev_out = best_of(lambda: eng.fit_aux_ratios(*dev, SEED, OMEGA, ones, ones, TOL, MAX_ITERS, LR), a.repeats)
            M = dev_out[0].size
            t_s, table = best_of(lambda: torch.from_numpy(build_normal_table(SEED, n, DIM, M - 1)).cuda(), 1)
            its = int(dev_out[2].sum())
            row.update({"partitions": int(M), "iterations_per_step": dev_out[2].tolist(), "iterations": its,
                        "device_fit_s": round(s, 5), "of_which_normal_table_build_and_upload_s": round(t_s, 5),
                        "device_us_per_iteration": round((s - t_s) / its * 1e6, 3)})
        if a.only in (None, "host"):
            s, host_out = best_of(lambda: fit_aux_ratios_host(*host, SEED, OMEGA, ones, ones, TOL, MAX_ITERS, LR, n_threads=16), 1)
            row.update({"host_16_threads_fit_s": round(s, 4)})
            if dev_out is not None:
                assert all(x.tobytes() == y.tobytes() for x, y in zip(dev_out, host_out)), "device and host twin disagree"
                row["device_equals_host_bits"] = True
                row["device_speedup_over_host"] = round(s / row["device_fit_s"], 1)
        if a.only in (None, "eager") and dev_out is not None:
            table = torch.from_numpy(build_normal_table(SEED, n, DIM, dev_out[0].size - 1)).cuda()
            eager_fit(dev, table)                                                          # warm-up
            s, (er, ei) = best_of(lambda: eager_fit(dev, table), max(1, a.repeats - 1))
            delta = float(np.max(np.abs(er.astype(np.float64) - dev_out[0].astype(np.float64))))
            assert delta <= 1e-5, (delta, ei)
            row.update({"eager_gpu_fit_s": round(s, 4), "eager_us_per_iteration": round(s / sum(ei) * 1e6, 2),
                        "eager_iterations": int(sum(ei)), "eager_max_abs_ratio_delta": delta, "device_speedup_over_eager": round(s / row["device_fit_s"], 1)})
            assert row["device_fit_s"] < s, "the device path must beat the eager restatement"
        print(json.dumps(row), flush=True)
        result["rows"].append(row)
    for spec in a.fold_stats:
        size, directory = spec.split("=", 1)
        result.setdefault("rocprofv3_kernel_stats", {})[size] = fold_stats(directory)
    if not a.only:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
