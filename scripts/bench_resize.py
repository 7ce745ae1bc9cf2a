#!/usr/bin/env python3
"""The driver's resize (irec.image.resize_bilinear: tf.image.resize, bilinear, shrink only, as one gfx950 kernel) measured in ONE run on
one box.  Writes profiles/resize/bench.json (or --out).  Needs a GPU.

time      per shape the legs alternate inside every repetition: medians of --reps after --warmup, device events, milliseconds.
            irec_f32 / torch_f32      image.resize_bilinear against F.interpolate(mode="bilinear", align_corners=False) on float32 NCHW
            irec_u8 / torch_u8        the same from uint8 images: one launch that converts, against x.float() / 255 then interpolate
            irec_f32_nhwc             the library's call on [N, H, W, C] (the reference's layout; torch has no such form)
            *_graph                   the same calls as graph replays: the kernels' time without the launch path of an eager call
            irec_f32_staged, irec_u8_staged   with --variant NAME: the same entry of the diagnostic build csrc/variants/NAME.so
                                      (make -C relative-entropy-coding_amd/csrc variant_image NAME=image_stage DEFS=-DIREC_IMAGE_STAGE=1: a
                                      tile's source rectangle copied into LDS first), its output compared with the product's bit for bit
          The algorithmic bytes (the input read once, the output written once) over the graph-replay time are reported against the HBM
          peak of bench.py's roofline (8 TB/s) under that name -- not a measured traffic figure.
          Shapes: 1 / 8 / 24 photographs of 500 x 375 to 448 x 320, 24 Kodak images to their own size (the copy), 300 crops of 70 x 70
          to 64 x 64.
grouping  harness.compress_images_lossy over the tests' list of five sizes with resize=True, against the same images resized by the
          caller with torch and passed one group (a 4-D tensor) per call: host clock around a synchronise, medians, Large1LevelVAE with
          its default 192 filters."""
import argparse
import ctypes
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "relative-entropy-coding_amd")]

# (name, n, in_h, in_w, out_h, out_w)
SHAPES = [("photo_1", 1, 375, 500, 320, 448), ("photo_8", 8, 375, 500, 320, 448), ("photo_24", 24, 375, 500, 320, 448),
          ("kodak_24_copy", 24, 512, 768, 512, 768), ("crops70_300", 300, 70, 70, 64, 64)]
HBM_PEAK_BYTES_PER_S = 8.0e12          # MI355X: 8 TB/s (bench.py: HBM_PEAK_GBS)
FIVE_SIZES = [(65, 67), (64, 64), (130, 201), (127, 64), (64, 64)]


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


def variant_resize(path):
    """image.resize_bilinear's NCHW device call over another build of the library (loaded beside the product, not instead of it)."""
    from irec import _lib
    lib = ctypes.CDLL(path)
    lib.irec_resize_bilinear_device.restype, lib.irec_resize_bilinear_device.argtypes = _lib.SIGNATURES["irec_resize_bilinear_device"]

    def resize(src, size):
        n, c, h, w = src.shape
        dst = torch.empty((n, c, *size), dtype=torch.float32, device=src.device)
        st = lib.irec_resize_bilinear_device(src.data_ptr(), 1 if src.dtype == torch.uint8 else 0, n, c, h, w, size[0], size[1], 0, dst.data_ptr(),
                                             torch.cuda.current_stream().cuda_stream)
        assert st == 0, st
        return dst
    return resize


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resize", "bench.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-grouping", action="store_true")
    ap.add_argument("--variant", default=None, help="a diagnostic build csrc/variants/NAME.so to time beside the product (the staged form)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_resize.py measures a GPU: none here")
    import irec
    from irec import harness, image
    from irec.models import Large1LevelVAE

    staged = variant_resize(os.path.join(ROOT, "relative-entropy-coding_amd", "csrc", "variants", args.variant + ".so")) if args.variant else None
    times = []
    for name, n, ih, iw, oh, ow in SHAPES:
        g = torch.Generator().manual_seed(11)
        u8 = torch.randint(0, 256, (n, 3, ih, iw), generator=g, dtype=torch.uint8).cuda()
        f32 = (u8.float() / 255.0).contiguous()
        nhwc = f32.permute(0, 2, 3, 1).contiguous()
        size = (oh, ow)
        legs = {"irec_f32": lambda: image.resize_bilinear(f32, size),
                "torch_f32": lambda: F.interpolate(f32, size=size, mode="bilinear", align_corners=False),
                "irec_u8": lambda: image.resize_bilinear(u8, size),
                "torch_u8": lambda: F.interpolate(u8.float() / 255.0, size=size, mode="bilinear", align_corners=False),
                "irec_f32_nhwc": lambda: image.resize_bilinear(nhwc, size, layout="nhwc")}
        if staged is not None:
            legs["irec_f32_staged"], legs["irec_u8_staged"] = (lambda: staged(f32, size)), (lambda: staged(u8, size))
            assert torch.equal(legs["irec_f32_staged"](), legs["irec_f32"]()) and torch.equal(legs["irec_u8_staged"](), legs["irec_u8"]())
        differ = float((legs["irec_f32"]() - legs["torch_f32"]()).abs().max())
        assert torch.equal(legs["irec_f32_nhwc"]().permute(0, 3, 1, 2), legs["irec_f32"]())
        differ_u8 = float((legs["irec_u8"]() - legs["torch_u8"]()).abs().max())
        graphs = {leg: captured(fn)[0] for leg, fn in legs.items()}
        t = alternate({**legs, **{f"{leg}_graph": gr.replay for leg, gr in graphs.items()}}, args.reps, args.warmup)
        out_bytes = n * 3 * oh * ow * 4
        nbytes = {"f32": n * 3 * ih * iw * 4 + out_bytes, "u8": n * 3 * ih * iw + out_bytes}
        row = {"shape": name, "n_images": n, "in": [ih, iw], "out": [oh, ow], "reps": args.reps, "unit": "ms: [median, min, max], device events", **t,
               "irec_and_torch_differ_by": {"f32": differ, "u8": differ_u8}, "algorithmic_bytes": nbytes}
        more = (("irec_f32_staged", "f32"), ("irec_u8_staged", "u8")) if staged is not None else ()
        for leg, kind in (("irec_f32", "f32"), ("torch_f32", "f32"), ("irec_u8", "u8"), ("torch_u8", "u8"), ("irec_f32_nhwc", "f32")) + more:
            rate = nbytes[kind] / (t[f"{leg}_graph"][0] * 1e-3)
            row[f"{leg}_graph_bytes_per_s"] = round(rate, -6)
            row[f"{leg}_graph_share_of_hbm_peak"] = round(rate / HBM_PEAK_BYTES_PER_S, 4)
        row["torch_over_irec"] = {k: round(t[f"torch_{k}"][0] / t[f"irec_{k}"][0], 2) for k in ("f32", "u8", "f32_graph", "u8_graph")}
        times.append(row)
        print(json.dumps(row), flush=True)
        del graphs

    grouping = None
    if not args.skip_grouping:
        torch.manual_seed(3)
        m = Large1LevelVAE().cuda().eval()
        with torch.no_grad():
            for mod in (m.analysis_transform[-1], m._prior_loc_head, m._prior_log_scale_head):
                mod.weight.mul_(0.2)
        sampler = irec.BeamSearchCoder(kl_per_partition=3., n_beams=10, extra_samples=1., block_size=1000)
        g = torch.Generator().manual_seed(11)
        images = [torch.rand(3, h, w, generator=g).cuda() for h, w in FIVE_SIZES]
        names = [f"im{i}" for i in range(len(images))]
        out_dir = tempfile.mkdtemp(prefix="irec_resize_")

        def library():
            return harness.compress_images_lossy(m, sampler, images, names, 42, 1000, out_dir, resize=True)

        def caller():
            resized = [F.interpolate(x[None], size=image.driver_size(*x.shape[1:]), mode="bilinear", align_corners=False) for x in images]
            groups = {}
            for i, r in enumerate(resized):
                groups.setdefault(tuple(r.shape[2:]), []).append(i)
            rows = []
            for members in groups.values():
                rows += harness.compress_images_lossy(m, sampler, torch.cat([resized[i] for i in members]), [names[i] for i in members], 42, 1000, out_dir)
            return rows
        assert len(library()) == len(caller()) == len(images)
        ts = {"library_list_resize_true": [], "caller_resizes_and_groups": []}
        for _ in range(args.warmup):
            library(), caller()
        for _ in range(args.reps):
            for leg, fn in (("library_list_resize_true", library), ("caller_resizes_and_groups", caller)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts[leg].append((time.perf_counter() - t0) * 1e3)
        grouping = {"sizes": FIVE_SIZES, "model": "Large1LevelVAE()", "reps": args.reps, "unit": "ms per call of five images: [median, min, max], host clock",
                    **{leg: [round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)] for leg, v in ts.items()}}
        print(json.dumps(grouping), flush=True)
        shutil.rmtree(out_dir, ignore_errors=True)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S, "variant": args.variant, "time": times, "grouping": grouping}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
