"""The lossy driver's resize (examples/lossy/compress_with_lossy_model.py:183-184): `tf.image.resize(image, [h - h % 64, w - w % 64])`
-- TF 2.1 ResizeBilinear with half_pixel_centers=True and antialias=False -- as the library's own arithmetic (include/irec.h and
DESIGN.md §3 "resize" have the definition), so that the image the quality columns are measured against is under the library's control.

CUDA tensors go through irec_resize_bilinear_device (csrc/irec_image.hip: one launch, no workspace) on the current stream, CPU tensors
through the host twin, the same core over host memory, which gives the device's bits.  Nothing synchronises.

SHRINK ONLY (the driver never enlarges an image), bilinear only, no antialiasing; an axis of equal sizes is not interpolated, so equal
sizes are a bit-for-bit copy.  Parity with a real TensorFlow run is not pinned: no TensorFlow is at hand to record one."""
import torch

from . import _lib

LAYOUTS = {"nchw": 0, "nhwc": 1}      # IREC_IMAGE_NCHW, IREC_IMAGE_NHWC
_DTYPES = {torch.float32: 0, torch.uint8: 1}   # IREC_IMAGE_F32, IREC_IMAGE_U8


def driver_size(h, w):
    """(h - h % 64, w - w % 64): the size the reference's driver brings an h x w image to before coding.  ValueError below 64."""
    h, w = int(h), int(w)
    if h < 64 or w < 64:
        raise ValueError(f"irec.image.driver_size: a {h} x {w} image has no multiple of 64 to be brought to (both sides at least 64)")
    return h - h % 64, w - w % 64


def resize_bilinear(images, size, layout="nchw", n_threads=0):
    """images [N, C, H, W] (layout="nchw") or [N, H, W, C] ("nhwc"), float32 or uint8 (converted as x / 255 in the same pass), to
    size = (out_h, out_w) <= (H, W): float32 in the same layout, on the images' device."""
    lib = _lib.load()
    if layout not in LAYOUTS:
        raise ValueError(f"irec.image.resize_bilinear: layout {layout!r} is neither 'nchw' nor 'nhwc'")
    if not isinstance(images, torch.Tensor) or images.dim() != 4 or images.dtype not in _DTYPES:
        raise ValueError("irec.image.resize_bilinear: images must be a 4-D float32 or uint8 tensor")
    src = images.contiguous()
    n, c, h, w = (int(v) for v in (src.shape if layout == "nchw" else (src.shape[0], src.shape[3], src.shape[1], src.shape[2])))
    out_h, out_w = (int(v) for v in size)
    if min(n, c, h, w) < 1 or out_h < 1 or out_w < 1 or out_h > h or out_w > w:
        raise ValueError(f"irec.image.resize_bilinear: {n} x {c} x {h} x {w} to {out_h} x {out_w}: every size at least 1 and no output "
                         "side above its input's (the resize only shrinks)")
    dst = torch.empty((n, c, out_h, out_w) if layout == "nchw" else (n, out_h, out_w, c), dtype=torch.float32, device=src.device)
    args = (src.data_ptr(), _DTYPES[src.dtype], n, c, h, w, out_h, out_w, LAYOUTS[layout], dst.data_ptr())
    if src.is_cuda:
        with torch.cuda.device(src.device):
            st = lib.irec_resize_bilinear_device(*args, torch.cuda.current_stream(src.device).cuda_stream)
    else:
        st = lib.irec_resize_bilinear_host(*args, int(n_threads))
    if st != 0:
        raise ValueError(lib.irec_last_error().decode("utf-8", "replace"))
    return dst
