#!/usr/bin/env python3
"""The quality metrics (irec.metrics: PSNR and MS-SSIM of a batch on the device) measured in ONE run on one box.  Writes
profiles/quality/bench.json (or --out).  Needs a GPU.

accuracy  per fixture of tests/quality_cases.py and per kind of value (psnr, ms_ssim, per-scale): the worst error of the device result
          and of the host twin against the float64 referee, and e_ref32, the error of the literal float32 restatement of TF's op order
          (direct 121-tap filter, uncentred) against the same referee.
time      metrics.quality eager and as a graph replay, against a torch-ops restatement on the same GPU (one depthwise F.conv2d with
          the 11 x 11 kernel over the four quantities, F.avg_pool2d; eager and as a graph replay), the alternatives alternating inside
          every repetition: medians of --reps after --warmup, device events, milliseconds.  The library call alone (metrics.moments) as
          a graph replay gives the kernels' time; the algorithmic bytes (two planes read per scale, two quarter-planes written) over
          it are reported as a share of HBM peak under that name -- not a measured traffic figure.
lossy     harness.compress_images_lossy with and without quality=True, 1 and 8 Kodak-size images, host clock around a synchronise."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "relative-entropy-coding_amd"), os.path.join(ROOT, "tests")]

SHAPES = [("kodak_1", 1, 512, 768), ("kodak_8", 8, 512, 768), ("kodak_24", 24, 512, 768), ("square256_64", 64, 256, 256)]
HBM_PEAK_BYTES_PER_S = 8.0e12          # MI355X: 8 TB/s
PF = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def torch_quality(a, b, kernel, pf=PF):
    """The definition in torch ops, float32: (psnr, ms_ssim) of clip(a) * 255 against b * 255."""
    x, y = a.clamp(0.0, 1.0) * 255.0, b * 255.0
    c = x.shape[1]
    psnr = 20.0 * np.log10(255.0) - 10.0 * torch.log10(((x - y) ** 2).mean(dim=(1, 2, 3)))
    c1, c2 = (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2
    terms = []
    for k in range(len(pf)):
        if k:
            ph, pw = x.shape[2] % 2, x.shape[3] % 2
            if ph or pw:
                x, y = (F.pad(t, (0, pw, 0, ph), mode="replicate") for t in (x, y))      # (one row or column: replicate is symmetric)
            x, y = F.avg_pool2d(x, 2), F.avg_pool2d(y, 2)
        f = F.conv2d(torch.cat([x, y, x * y, x * x + y * y], dim=1), kernel, groups=4 * c)
        m0, m1, xy, sq = f[:, :c], f[:, c:2 * c], f[:, 2 * c:3 * c], f[:, 3 * c:]
        num0, den0 = 2.0 * m0 * m1, m0 * m0 + m1 * m1
        cs = (2.0 * xy - num0 + c2) / (sq - den0 + c2)
        terms.append((((num0 + c1) / (den0 + c1)) * cs if k == len(pf) - 1 else cs).mean(dim=(2, 3)).clamp_min(0.0) ** pf[k])
    return psnr, torch.stack(terms).prod(dim=0).mean(dim=1)


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


def captured(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn()
    return graph, out


def algorithmic_bytes(n, c, h, w, n_scales):
    total = 0
    for k in range(n_scales):
        total += 2 * n * c * h * w * 4
        h, w = (h + 1) // 2, (w + 1) // 2
        if k + 1 < n_scales:
            total += 2 * n * c * h * w * 4
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quality", "bench.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-lossy", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_quality.py measures a GPU: none here")
    import irec
    import quality_cases as Q
    from irec import harness, metrics

    accuracy = []
    for shape_name, family in Q.CASES:
        a, b = Q.fixture(shape_name, family)
        y = Q.yardstick(shape_name, family)
        row = {"shape": shape_name, "family": family, "e_ref32": y.e_ref32}
        for leg, dev in (("device", "cuda"), ("host_twin", "cpu")):
            got = metrics.quality(torch.from_numpy(np.array(a)).to(dev), torch.from_numpy(np.array(b)).to(dev), y.power_factors, **Q.UNIT)
            row[leg] = {}
            for kind, g in zip(("psnr", "ms_ssim", "per_scale"), got):
                want = getattr(y, kind)
                finite = np.isfinite(want)
                row[leg][kind] = float(np.max(np.abs(g.cpu().numpy().astype(np.float64)[finite] - want[finite]), initial=0.0))
        accuracy.append(row)
        print(json.dumps(row), flush=True)

    times = []
    for name, n, h, w in SHAPES:
        g = torch.Generator().manual_seed(11)
        b = torch.rand(n, 3, h, w, generator=g).cuda()
        a = (b + 0.05 * torch.randn(n, 3, h, w, generator=g).cuda()).contiguous()
        k1d = torch.exp(-(torch.arange(11, dtype=torch.float64) - 5) ** 2 / 4.5)
        k2d = torch.outer(k1d, k1d)
        kernel = (k2d / k2d.sum()).to(torch.float32).cuda().expand(12, 1, 11, 11).contiguous()
        ours, theirs = metrics.quality(a, b), torch_quality(a, b, kernel)
        agree = {"psnr": float((ours[0] - theirs[0]).abs().max()), "ms_ssim": float((ours[1] - theirs[1]).abs().max())}
        g_ours, _ = captured(lambda: metrics.quality(a, b))
        g_theirs, _ = captured(lambda: torch_quality(a, b, kernel))
        g_moments, _ = captured(lambda: metrics.moments(a, b, 5))
        t = alternate({"irec_eager": lambda: metrics.quality(a, b), "torch_eager": lambda: torch_quality(a, b, kernel),
                       "irec_graph": g_ours.replay, "torch_graph": g_theirs.replay, "irec_moments_graph": g_moments.replay}, args.reps, args.warmup)
        nbytes = algorithmic_bytes(n, 3, h, w, 5)
        row = {"shape": name, "n_images": n, "height": h, "width": w, "reps": args.reps, "unit": "ms: [median, min, max], device events", **t,
               "irec_and_torch_differ_by": agree, "algorithmic_bytes": nbytes,
               "algorithmic_bytes_over_moments_graph_time_share_of_hbm_peak": round(nbytes / (t["irec_moments_graph"][0] * 1e-3) / HBM_PEAK_BYTES_PER_S, 4),
               "torch_eager_over_irec_eager": round(t["torch_eager"][0] / t["irec_eager"][0], 2),
               "torch_graph_over_irec_graph": round(t["torch_graph"][0] / t["irec_graph"][0], 2)}
        times.append(row)
        print(json.dumps(row), flush=True)
        del g_ours, g_theirs, g_moments

    lossy = []
    if not args.skip_lossy:
        from irec.models import Large2LevelVAE
        torch.manual_seed(3)
        m = Large2LevelVAE().cuda().eval()
        with torch.no_grad():                        # scripts/bench_lossy.py's low_K setting
            for mod in (m.analysis_transform[-1], m.hyper_analysis_transform[-1], m.hyper_synthesis_transform[-1], m._prior_loc_head,
                        m._prior_log_scale_head, m._level_1_posterior_loc_combiner, m._level_1_posterior_log_scale_combiner):
                mod.weight.mul_(0.2)
        sampler = irec.BeamSearchCoder(kl_per_partition=3., n_beams=10, extra_samples=1., block_size=1000)
        out_dir = tempfile.mkdtemp(prefix="irec_quality_")
        for n in (1, 8):
            g = torch.Generator().manual_seed(11)
            images = (torch.rand(n, 3, 512, 768, generator=g) - 0.5).cuda()
            names = [f"img{i}" for i in range(n)]
            ts = {False: [], True: []}
            for rep in range(args.warmup + args.reps):
                for quality in (False, True):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    rows = harness.compress_images_lossy(m, sampler, images, names, 42, 1000, out_dir, quality=quality, image_range=(-0.5, 0.5))
                    torch.cuda.synchronize()
                    if rep >= args.warmup:
                        ts[quality].append((time.perf_counter() - t0) * 1e3)
            row = {"n_images": n, "height": 512, "width": 768, "reps": args.reps, "unit": "ms per batch: [median, min, max], host clock",
                   "plain": [round(statistics.median(ts[False]), 3), round(min(ts[False]), 3), round(max(ts[False]), 3)],
                   "quality": [round(statistics.median(ts[True]), 3), round(min(ts[True]), 3), round(max(ts[True]), 3)],
                   "last_row": {k: rows[0][k] for k in ("psnr", "ms_ssim", "kld", "lossy_bpp", "comp_lossy_bpp")}}
            lossy.append(row)
            print(json.dumps(row), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S, "accuracy": accuracy, "time": times,
                   "compress_images_lossy": lossy}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
