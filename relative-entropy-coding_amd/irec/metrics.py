"""Distortion of a batch: PSNR and MS-SSIM of reconstructions `a` against originals `b`, float32 [N, C, H, W] each (the last two
columns of the reference's lossy results row, examples/lossy/compress_with_lossy_model.py:192-270: tf.image.psnr and
tf.image.ssim_multiscale of `clip(reconstruction, 0, 1) * 255` against `image * 255`, max_val = 255).

CUDA tensors go through irec_quality_device (csrc/irec_quality.hip: one launch per scale and one for the sums, nothing else), CPU
tensors through irec_quality_host, the same core over host memory; both leave the per-(image, channel, scale) means and the sum of
squared errors, and the last step here -- clamp at 0, powers, product, channel mean, log10 -- is a handful of float64 torch ops on the
inputs' device.  Nothing synchronises: `quality` on CUDA tensors can be captured by torch.cuda.graph on one stream.

A pixel is `v * mul + add`, clamped to [0, max_val] where the image's clip flag is set.  The defaults are the reference's lossy
convention (images in [0, 1]: mul 255, add 0, the reconstruction clipped); `transform_for(image_range)` gives the arguments for images
in another range, e.g. the model shim's [-0.5, 0.5].  Parity with a real TensorFlow run is not pinned (DESIGN.md §3 "quality")."""
import ctypes
import math

import torch

from . import _lib

POWER_FACTORS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)      # tf.image.ssim_multiscale's default
FILTER_SIZE = 11
MAX_SCALES = 5


def transform_for(image_range=(0., 1.), max_val=255., clip_a=True, clip_b=False):
    """The keyword arguments of psnr / ms_ssim / quality for images whose values lie in image_range = (lo, hi): lo maps to 0 and hi to
    max_val; the reconstruction `a` clamped to that range, the original `b` not (the reference's convention)."""
    lo, hi = float(image_range[0]), float(image_range[1])
    if not hi > lo:
        raise ValueError(f"image_range {image_range!r}: the upper end must exceed the lower")
    mul = float(max_val) / (hi - lo)
    return {"mul": mul, "add": -lo * mul, "clip": (bool(clip_a), bool(clip_b)), "max_val": float(max_val)}


def min_side(n_scales):
    """The smallest height or width that n_scales scales allow: the last scale is still 11 pixels."""
    side = FILTER_SIZE
    for _ in range(int(n_scales) - 1):
        side = 2 * side - 1
    return side


def _params(mul, add, clip, max_val, k1, k2):
    mul_a, mul_b = (mul if isinstance(mul, (tuple, list)) else (mul, mul))
    add_a, add_b = (add if isinstance(add, (tuple, list)) else (add, add))
    clip_a, clip_b = (clip if isinstance(clip, (tuple, list)) else (clip, clip))
    return _lib.IrecQualityParams(float(mul_a), float(add_a), float(mul_b), float(add_b), int(bool(clip_a)), int(bool(clip_b)),
                                  float(max_val), float(k1), float(k2))


def moments(a, b, n_scales, mul=255., add=0., clip=(True, False), max_val=255., k1=0.01, k2=0.03, n_threads=0):
    """What the library leaves (include/irec.h: irec_quality_*): (per_scale float32 [N, C, n_scales, 2], sse float32 [N]) on the
    inputs' device.  per_scale[..., 0] is the mean of lum * cs and [..., 1] the mean of cs over the VALID filter outputs of the scale,
    not clamped; sse the sum of squared pixel differences of the image.  mul / add / clip: one value for both images, or (a's, b's)."""
    lib = _lib.load()
    if a.shape != b.shape or a.dim() != 4:
        raise ValueError(f"irec.metrics: a {tuple(a.shape)} and b {tuple(b.shape)} are not one [N, C, H, W] shape")
    if a.device != b.device:
        raise ValueError(f"irec.metrics: a on {a.device}, b on {b.device}")
    a, b = a.to(torch.float32).contiguous(), b.to(torch.float32).contiguous()
    n, c, h, w = (int(v) for v in a.shape)
    n_scales = int(n_scales)
    if not 1 <= n_scales <= MAX_SCALES:
        raise ValueError(f"irec.metrics: n_scales must be 1 .. 5, not {n_scales}")
    params = _params(mul, add, clip, max_val, k1, k2)
    per_scale = torch.empty((n, c, max(n_scales, 0), 2), dtype=torch.float32, device=a.device)
    sse = torch.empty((n,), dtype=torch.float32, device=a.device)
    if a.is_cuda:
        nbytes = lib.irec_quality_workspace_bytes(n, c, h, w, n_scales)
        workspace = torch.empty((max(nbytes, 8) + 7) // 8, dtype=torch.float64, device=a.device)
        with torch.cuda.device(a.device):
            st = lib.irec_quality_device(a.data_ptr(), b.data_ptr(), n, c, h, w, n_scales, ctypes.byref(params), per_scale.data_ptr(),
                                         sse.data_ptr(), workspace.data_ptr(), workspace.numel() * 8,
                                         torch.cuda.current_stream(a.device).cuda_stream)
    else:
        st = lib.irec_quality_host(a.data_ptr(), b.data_ptr(), n, c, h, w, n_scales, ctypes.byref(params), per_scale.data_ptr(),
                                   sse.data_ptr(), int(n_threads))
    if st != 0:
        raise ValueError(lib.irec_last_error().decode("utf-8", "replace"))
    return per_scale, sse


def _psnr_of(sse, pixels, max_val):
    mse = sse.to(torch.float64) / float(pixels)
    return 20.0 * math.log10(float(max_val)) - 10.0 * torch.log10(mse)            # (identical images: mse 0, +inf)


def _ms_ssim_of(per_scale, power_factors):
    v = per_scale.to(torch.float64).clamp_min(0.0)
    last = len(power_factors) - 1
    out = v[:, :, last, 0].pow(float(power_factors[last]))                          # ssim of the last scale, cs of the others
    for k in range(last - 1, -1, -1):                                               # (scalar exponents: no upload, capturable)
        out = v[:, :, k, 1].pow(float(power_factors[k])) * out
    return out.mean(dim=1)


def quality(a, b, power_factors=POWER_FACTORS, mul=255., add=0., clip=(True, False), max_val=255., k1=0.01, k2=0.03, n_threads=0):
    """(psnr float64 [N], ms_ssim float64 [N], per_scale float32 [N, C, len(power_factors), 2]) of reconstructions a against
    originals b.  psnr = 20 log10(max_val) - 10 log10(mse), +inf for identical images; ms_ssim is tf.image.ssim_multiscale with its
    defaults and len(power_factors) (1 .. 5) scales.  An image below 11 x 11 at one of its scales is a ValueError, as TF asserts."""
    power_factors = tuple(power_factors)
    per_scale, sse = moments(a, b, len(power_factors), mul, add, clip, max_val, k1, k2, n_threads)
    pixels = a.shape[1] * a.shape[2] * a.shape[3]
    return _psnr_of(sse, pixels, max_val), _ms_ssim_of(per_scale, power_factors), per_scale


def psnr(a, b, mul=255., add=0., clip=(True, False), max_val=255., n_threads=0):
    """tf.image.psnr of the transformed pixels: float64 [N].  (One scale of the moments is computed with it: images of at least
    11 x 11.)"""
    return quality(a, b, POWER_FACTORS[:1], mul, add, clip, max_val, n_threads=n_threads)[0]


def ms_ssim(a, b, power_factors=POWER_FACTORS, mul=255., add=0., clip=(True, False), max_val=255., k1=0.01, k2=0.03, n_threads=0):
    """tf.image.ssim_multiscale of the transformed pixels: float64 [N]."""
    return quality(a, b, power_factors, mul, add, clip, max_val, k1, k2, n_threads)[1]
