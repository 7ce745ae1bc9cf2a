#!/usr/bin/env python3
"""The ideal half of a results row (irec.ideal: seeded posterior draws with their KL, the log-likelihood of a batch) measured in ONE run
on one box.  Writes profiles/ideal/bench.json (or --out).  Needs a GPU.  Medians of --reps after --warmup, device events, the legs
alternating inside every repetition, milliseconds.

draw      posterior_draw for the 24 tensors [N, 16, 16, 32] of the 24-block model at N = 1, 38 and 300, against
            torch_device   torch.randn on the device, the draw in torch ops, and harness._gaussian_kl_per_image's float64 KL expression
            cpu_copy       the form update_coders has: torch.randn from a CPU generator, copied to the device, the draw in torch ops (no KL)
          The draw's algorithmic bytes (16 B in, 4 B out per element) over its time are reported as a share of HBM peak.
loglik    log_likelihood of N Kodak-size images against the same formula in float64 torch ops.
harness   harness.compress_images with and without ideal=True on a 24-block model, host clock around a synchronise: the ideal pass as a
          share of a batch."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "relative-entropy-coding_amd"), os.path.join(ROOT, "tests")]

HBM_PEAK_BYTES_PER_S = 8.0e12          # MI355X: 8 TB/s
N_TENSORS, LATENT = 24, (16, 16, 32)


def alternate(fns, reps, warmup):
    """{name: [median, min, max] ms} of the callables, each repetition running every one of them once, device events."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts[name].append(e0.elapsed_time(e1))
    return {name: [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)] for name, v in ts.items()}


def torch_loglik(x, loc, log_scale, binsize=1.0 / 256.0):
    xd, ld = x.to(torch.float64), loc.to(torch.float64)
    scale = torch.exp(torch.as_tensor(log_scale, dtype=torch.float64, device=x.device))
    a = (torch.floor(xd / binsize) * binsize - ld) / scale
    return torch.log(torch.sigmoid(a + binsize / scale) - torch.sigmoid(a) + 1e-7).sum(dim=(1, 2, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ideal", "bench.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-harness", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ideal.py measures a GPU: none here")
    from irec import harness, ideal
    N = types.SimpleNamespace

    draw = []
    for n in (1, 38, 300):
        g = torch.Generator().manual_seed(5)
        tensors = []
        for _ in range(N_TENSORS):
            mp, sp = torch.randn(n, *LATENT, generator=g).cuda(), torch.rand(n, *LATENT, generator=g).cuda() + 0.5
            tensors.append((N(loc=mp + 0.3 * sp, scale=0.7 * sp), N(loc=mp, scale=sp)))
        cpu_gen = torch.Generator().manual_seed(42)

        def ours():
            return [ideal.posterior_draw(q, p, 42, r) for r, (q, p) in enumerate(tensors)]

        def torch_device():
            return [(q.loc + q.scale * torch.randn(q.loc.shape, device="cuda"), harness._gaussian_kl_per_image(q, p)) for q, p in tensors]

        def cpu_copy():
            return [q.loc + q.scale * torch.randn(q.loc.shape, generator=cpu_gen, dtype=torch.float32).to("cuda") for q, _ in tensors]
        kl_ours, kl_torch = torch.stack([k for _, k in ours()]), torch.stack([k for _, k in torch_device()])
        t = alternate({"irec": ours, "torch_device": torch_device, "cpu_copy": cpu_copy}, args.reps, args.warmup)
        elements = N_TENSORS * n * LATENT[0] * LATENT[1] * LATENT[2]
        row = {"n_images": n, "tensors": N_TENSORS, "latent": list(LATENT), "reps": args.reps, "unit": "ms for the 24 tensors: [median, min, max], device events",
               **t, "kl_differs_from_torch_by_relative": float(((kl_ours - kl_torch).abs() / kl_torch.abs()).max()),
               "algorithmic_bytes": 20 * elements,
               "algorithmic_bytes_over_irec_time_share_of_hbm_peak": round(20 * elements / (t["irec"][0] * 1e-3) / HBM_PEAK_BYTES_PER_S, 4),
               "torch_device_over_irec": round(t["torch_device"][0] / t["irec"][0], 2), "cpu_copy_over_irec": round(t["cpu_copy"][0] / t["irec"][0], 2)}
        draw.append(row)
        print(json.dumps(row), flush=True)
        del tensors

    loglik = []
    for n in (1, 8, 24):
        g = torch.Generator().manual_seed(11)
        x = (torch.randint(0, 256, (n, 3, 512, 768), generator=g) / 256.0 - 0.5).cuda()
        loc = (x + 0.03 * torch.randn(x.shape, generator=g).cuda()).clamp(-0.5 + 1 / 512, 0.5 - 1 / 512)
        agree = float(((ideal.log_likelihood(x, loc, -3.5) - torch_loglik(x, loc, -3.5)).abs() / torch_loglik(x, loc, -3.5).abs()).max())
        t = alternate({"irec": lambda: ideal.log_likelihood(x, loc, -3.5), "torch_float64": lambda: torch_loglik(x, loc, -3.5)}, args.reps, args.warmup)
        row = {"n_images": n, "height": 512, "width": 768, "reps": args.reps, "unit": "ms: [median, min, max], device events", **t,
               "differs_from_torch_by_relative": agree, "torch_float64_over_irec": round(t["torch_float64"][0] / t["irec"][0], 2)}
        loglik.append(row)
        print(json.dumps(row), flush=True)

    rows_harness = []
    if not args.skip_harness:
        from irec.models import BidirectionalResNetVAE
        torch.manual_seed(0)
        m = BidirectionalResNetVAE(num_res_blocks=24, sampler="beam_search", sampler_args={"n_beams": 20, "extra_samples": 1.2},
                                   coder_args={"block_size": 1000}, deterministic_filters=160, stochastic_filters=32, kl_per_partition=3.)
        with torch.no_grad():                        # random-init weights: keep the posteriors close to the priors so that K stays small
            for b in m.residual_blocks:
                for head in (b.infer_posterior_loc_head, b.infer_posterior_log_scale_head, b.gen_posterior_loc_head, b.gen_posterior_log_scale_head):
                    head.weight.mul_(0.05)
                    head.bias.zero_()
        m = m.cuda().eval()
        out_dir = tempfile.mkdtemp(prefix="irec_ideal_")
        for n in (1, 8):
            images = (torch.rand(n, 3, 32, 32, generator=torch.Generator().manual_seed(7)) - 0.5).cuda()
            names = [f"img{i}" for i in range(n)]
            ts = {False: [], True: []}
            for rep in range(args.warmup + max(3, args.reps // 4)):
                for flag in (False, True):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    rows = harness.compress_images(m, images, names, 42, 1000, out_dir, rec_on_device=True, ideal=flag)
                    torch.cuda.synchronize()
                    if rep >= args.warmup:
                        ts[flag].append((time.perf_counter() - t0) * 1e3)
            med = {flag: statistics.median(v) for flag, v in ts.items()}
            row = {"n_images": n, "height": 32, "width": 32, "res_blocks": 24, "reps": len(ts[True]), "unit": "ms per batch: [median, min, max], host clock",
                   "plain": [round(med[False], 3), round(min(ts[False]), 3), round(max(ts[False]), 3)],
                   "ideal": [round(med[True], 3), round(min(ts[True]), 3), round(max(ts[True]), 3)],
                   "ideal_pass_share_of_batch": round((med[True] - med[False]) / med[True], 4),
                   "last_row": {k: rows[0][k] for k in ("residual", "kl", "bpd", "comp_kl", "comp_codelength", "overhead_bits")}}
            rows_harness.append(row)
            print(json.dumps(row), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S, "posterior_draw": draw,
                   "log_likelihood": loglik, "compress_images": rows_harness}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
