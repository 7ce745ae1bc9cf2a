"""The `.res` container: an image's pixels, arithmetic-coded under the model's discretized-logistic likelihood given the
reconstruction, so that NAME.rec + NAME.res decode to exactly the uint8 image (csrc/irec_res.hip over csrc/irec_res_core.h;
INTEGRATION.md has the layout).  `.rec` files are untouched by it.

pixels [N, C, H, W] uint8, loc the same shape in float32 (the clamped reconstruction), scale one float32 per call.  The device
calls take and return CUDA tensors; the host calls run the same core over numpy arrays and give the same bytes."""
import math

import numpy as np

from .. import _lib
from . import _files

# Symbols per stream where a call does not say.  A device call's time is its longest lane's, about 0.26 ms + 4.7 us per symbol of a
# stream up to hundreds of images, and a stream costs its 16-bit length word plus about 9 bits of coder end and padding
# (scripts/bench_residual.py -> profiles/residual/bench.json, 300 images): 64 keeps one image's call level with the host twin
# (0.45 ms) at 6.2 % over the model's bits; 128 gives 3.7 % for 0.97 ms, 256 2.4 % for 1.8 ms, 1024 1.5 % for 6.8 ms.
DEFAULT_STREAM_LEN = 64
MAX_STREAM_LEN = 4096
HEADER_BYTES = 28
MAX_BITS_PER_SYMBOL = 18            # csrc/irec_res_core.h: what a stream can cost at the most, per symbol (+ 2 bits per stream)

_RES_STATUS_TEXT = {
    1: "irec_res_encode_files: the likelihood scale is not finite, not positive or outside [2^-24, 2^24]",
    2: "irec_res_encode_files: a reconstruction value (loc) is not finite",
    3: "irec_res_decode_files: truncated header",
    4: "irec_res_decode_files: not a .res file of this version (magic / version)",
    5: "irec_res_decode_files: the file's shape or stream length differs from the call's",
    6: "irec_res_decode_files: the file's likelihood scale differs from the call's",
    7: "irec_res_decode_files: the streams run past the file",
    8: "irec_res_decode_files: corrupt stream",
    9: "irec_res_decode_files: checksum mismatch (the reconstruction differs from the encoder's, or the bits are damaged)",
}


def res_status_text(status):
    return _RES_STATUS_TEXT.get(int(status), f"irec_res: status {int(status)}")


def _raise_first_status(status):
    _files.raise_first_status(status, res_status_text)


def _scale32(scale):
    return float(np.float32(scale))


def _shape(pixels_shape, loc_shape, stream_len, who):
    if len(pixels_shape) != 4 or tuple(pixels_shape) != tuple(loc_shape):
        raise ValueError(f"{who}: pixels {tuple(pixels_shape)} and loc {tuple(loc_shape)} are not one [N, C, H, W] shape")
    stream_len = DEFAULT_STREAM_LEN if stream_len is None else int(stream_len)
    if not 1 <= stream_len <= MAX_STREAM_LEN:
        raise ValueError(f"{who}: stream_len {stream_len} outside [1, {MAX_STREAM_LEN}]")
    n, c, h, w = (int(v) for v in pixels_shape)
    if min(c, h, w) < 1 or max(c, h, w) > 65535 or c * h * w >= 2 ** 31:
        raise ValueError(f"{who}: image shape {(c, h, w)} out of range")
    return n, c, h, w, stream_len, -(-(c * h * w) // stream_len)


def max_file_bytes(c, h, w, stream_len):
    """What one image's .res file can take at the most (MAX_BITS_PER_SYMBOL)."""
    n_sym = c * h * w
    ns = -(-n_sym // stream_len)
    return HEADER_BYTES + 2 * ns + (MAX_BITS_PER_SYMBOL * n_sym + 2 * ns) // 8 + ns


def stream_len_of(data):
    """The stream_len word of a .res file's bytes (None for bytes too short to hold it)."""
    data = bytes(data[:12])
    return int.from_bytes(data[8:12], "little") if len(data) >= 12 else None


# ---- host ---------------------------------------------------------------------------------------------------------------------------
def encode_residuals(pixels, loc, scale, stream_len=None, n_threads=0):
    """N .res files from numpy arrays (irec_res_encode_files): (blob uint8, offsets int64 [N + 1]), file i = blob[offsets[i]:offsets[i + 1]].
    ValueError naming the first image that cannot be coded."""
    lib = _lib.load()
    pixels = np.ascontiguousarray(pixels, dtype=np.uint8)
    loc = np.ascontiguousarray(loc, dtype=np.float32)
    n, c, h, w, stream_len, _ = _shape(pixels.shape, loc.shape, stream_len, "encode_residuals")
    offsets = np.zeros(n + 1, dtype=np.int64)
    status = np.zeros(max(n, 1), dtype=np.int32)
    cap = n * (HEADER_BYTES + 2 * -(-(c * h * w) // stream_len) + c * h * w) + 64      # a first guess: a byte per pixel
    for _attempt in range(2):
        out = np.empty(max(cap, 1), dtype=np.uint8)
        st = lib.irec_res_encode_files(pixels.ctypes.data, loc.ctypes.data, _scale32(scale), n, h, w, c, stream_len, out.ctypes.data,
                                       out.size, offsets.ctypes.data, status.ctypes.data, int(n_threads))
        if st != 0:
            raise ValueError(lib.irec_last_error().decode())
        _raise_first_status(status[:n])
        if offsets[n] <= out.size:
            return out[:offsets[n]], offsets
        cap = int(offsets[n])
    raise ValueError("irec_res_encode_files: the files did not fit the size the call itself reported")


def decode_residuals(blob, offsets, loc, scale, stream_len=None, strict=True, n_threads=0):
    """The inverse (irec_res_decode_files): pixels uint8 of loc's shape; strict=False: (pixels, status int32 [N]), an image with a
    nonzero status zero.  stream_len None: the word of the first file's header."""
    lib = _lib.load()
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    loc = np.ascontiguousarray(loc, dtype=np.float32)
    if stream_len is None and offsets.size >= 2:
        stream_len = stream_len_of(blob[int(offsets[0]):int(offsets[1])])
        stream_len = stream_len if stream_len and 1 <= stream_len <= MAX_STREAM_LEN else None
    n, c, h, w, stream_len, _ = _shape(loc.shape, loc.shape, stream_len, "decode_residuals")
    offsets = _files.host_offsets(offsets, blob.size, "decode_residuals", n)
    pixels = np.zeros(loc.shape, dtype=np.uint8)
    status = np.zeros(max(n, 1), dtype=np.int32)
    keep = blob if blob.size else np.zeros(1, np.uint8)
    st = lib.irec_res_decode_files(keep.ctypes.data, offsets.ctypes.data, loc.ctypes.data, _scale32(scale), n, h, w, c, stream_len,
                                   pixels.ctypes.data, status.ctypes.data, int(n_threads))
    if st != 0:
        raise ValueError(lib.irec_last_error().decode())
    if strict:
        _raise_first_status(status[:n])
        return pixels
    return pixels, status[:n].copy()


def model_counts(m, scale):
    """The 257 cumulative counts C(0 .. 256) of one (m, scale) (irec_res_model_counts)."""
    lib = _lib.load()
    out = np.zeros(257, dtype=np.uint32)
    if lib.irec_res_model_counts(int(m), _scale32(scale), out.ctypes.data) != 0:
        raise ValueError(lib.irec_last_error().decode())
    return out


def residual_model_bits(pixels, loc, scale):
    """The ideal bits of every image under the integer model: sum over its pixels of -log2(count / 65536) (float64 [N])."""
    lib = _lib.load()
    pixels = pixels.cpu().numpy() if hasattr(pixels, "cpu") else pixels
    loc = loc.cpu().numpy() if hasattr(loc, "cpu") else loc
    pixels = np.ascontiguousarray(pixels, dtype=np.uint8)
    loc = np.ascontiguousarray(loc, dtype=np.float32)
    if pixels.shape != loc.shape or pixels.ndim < 1:
        raise ValueError("residual_model_bits: pixels and loc differ in shape")
    count = np.zeros(pixels.size, dtype=np.uint32)
    if lib.irec_res_symbol_counts(pixels.ctypes.data, loc.ctypes.data, _scale32(scale), pixels.size, count.ctypes.data) != 0:
        raise ValueError(lib.irec_last_error().decode())
    with np.errstate(divide="ignore"):
        bits = 16.0 - np.log2(count.astype(np.float64))
    return bits.reshape(pixels.shape[0], -1).sum(axis=1)


# ---- device -------------------------------------------------------------------------------------------------------------------------
def _check_device(pixels, loc, who):
    import torch
    if not (loc.is_cuda and loc.dtype == torch.float32):
        raise ValueError(f"{who}: loc must be a CUDA float32 tensor")
    if pixels is not None and not (pixels.is_cuda and pixels.dtype == torch.uint8 and pixels.device == loc.device):
        raise ValueError(f"{who}: pixels must be a CUDA uint8 tensor on loc's device")


def _encode_residuals_device_launch(pixels, loc, scale, stream_len, out):
    """One irec_res_encode_files_device call on the current stream, nothing read back: (offsets int64 [N + 1], status int32 [N], both views
    of `both`, which one copy fetches).  The bytes are in `out` only if offsets[N] <= out.numel()."""
    import torch
    lib = _lib.load()
    n, c, h, w, stream_len, ns = _shape(pixels.shape, loc.shape, stream_len, "encode_residuals_device")
    pixels, loc = pixels.contiguous(), loc.contiguous()
    dev = loc.device
    with torch.cuda.device(dev):
        ws = torch.empty(lib.irec_res_device_workspace_bytes(n, ns), dtype=torch.uint8, device=dev)
        offsets, status, both = _files.offsets_and_status(n, dev)
        st = lib.irec_res_encode_files_device(pixels.data_ptr() if n else None, loc.data_ptr() if n else None, _scale32(scale), n, h, w, c,
                                              stream_len, out.data_ptr() if out.numel() else None, out.numel(), offsets.data_ptr(),
                                              status.data_ptr() if n else None, ws.data_ptr(), ws.numel(),
                                              torch.cuda.current_stream().cuda_stream)
    _files.check_status(st, "irec_res_encode_files_device")
    return offsets, status, both


def encode_residuals_device(pixels, loc, scale, stream_len=None, out=None):
    """encode_residuals on the device (irec_res_encode_files_device): (blob uint8, offsets int64 [N + 1]) as CUDA tensors, byte for byte
    what encode_residuals gives; the only host synchronisation is ONE read-back of offsets and status.
    out: a CUDA uint8 buffer to write into (a short one costs a second run at the size the first one reports)."""
    import torch
    _check_device(pixels, loc, "encode_residuals_device")
    n, c, h, w, stream_len, ns = _shape(pixels.shape, loc.shape, stream_len, "encode_residuals_device")
    if out is None:
        out = torch.empty(max(n * (HEADER_BYTES + 2 * ns + c * h * w) + 64, 1), dtype=torch.uint8, device=loc.device)
    elif not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.device == loc.device):
        raise ValueError("encode_residuals_device: out must be a contiguous CUDA uint8 tensor on loc's device")
    return _files.encode_device(lambda o: _encode_residuals_device_launch(pixels, loc, scale, stream_len, o), n, out, res_status_text,
                                "irec_res_encode_files_device")


def _decode_residuals_device_launch(blob, offsets, loc, scale, stream_len, on_device=False):
    """One irec_res_decode_files_device call on the current stream: (pixels uint8 of loc's shape, status int32 [N]) on the device,
    nothing read back.  Host offsets are checked against the blob; on_device: offsets that are on the device stay there, clamped into
    the blob and made non-decreasing by two small device operations (_files.device_offsets)."""
    import torch
    lib = _lib.load()
    _check_device(None, loc, "decode_residuals_device")
    if not (blob.is_cuda and blob.dtype == torch.uint8):
        raise ValueError("decode_residuals_device takes a CUDA uint8 tensor")
    n, c, h, w, stream_len, ns = _shape(loc.shape, loc.shape, stream_len, "decode_residuals_device")
    blob, loc = blob.contiguous(), loc.contiguous()
    dev = loc.device
    off_dev = _files.device_offsets(offsets, blob, dev, on_device, "decode_residuals_device", n)
    with torch.cuda.device(dev):
        ws = torch.empty(lib.irec_res_device_workspace_bytes(n, ns), dtype=torch.uint8, device=dev)
        pixels = torch.empty(loc.shape, dtype=torch.uint8, device=dev)
        status = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
        st = lib.irec_res_decode_files_device(blob.data_ptr() if blob.numel() else ws.data_ptr(), off_dev.data_ptr(), loc.data_ptr() if n else None,
                                              _scale32(scale), n, h, w, c, stream_len, pixels.data_ptr() if n else None, status.data_ptr(),
                                              ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    _files.check_status(st, "irec_res_decode_files_device")
    return pixels, status[:n]


def _stream_len_device(blob, offsets):
    """The stream_len word of the first file of a device blob: a 12-byte read-back (a caller that knows it passes stream_len)."""
    first = int(offsets[0])
    return stream_len_of(blob[first:min(first + 12, int(offsets[1]))].cpu().numpy().tobytes()) if len(offsets) >= 2 else None


def decode_residuals_device(blob, offsets, loc, scale, stream_len=None, strict=True):
    """decode_residuals on the device (irec_res_decode_files_device): blob uint8 CUDA, offsets [N + 1] (CUDA, CPU or numpy), loc CUDA
    float32 [N, C, H, W].  Returns pixels uint8 CUDA; ValueError naming the first image that cannot be decoded.  strict=False:
    (pixels, status int32 numpy [N]), an image with a nonzero status zero.  ONE read-back, the status (and, with stream_len None, the
    12 header bytes that hold it)."""
    if stream_len is None:
        stream_len = _stream_len_device(blob, offsets)
        stream_len = stream_len if stream_len and 1 <= stream_len <= MAX_STREAM_LEN else None
    pixels, status = _decode_residuals_device_launch(blob, offsets, loc, scale, stream_len)
    host = status.cpu().numpy()
    if strict:
        _raise_first_status(host)
        return pixels
    return pixels, host


def scale_from_log(log_scale):
    """The call's float32 scale from a likelihood_log_scale value: exp in float64, rounded once to float32."""
    return float(np.float32(math.exp(float(log_scale))))


__all__ = ["encode_residuals", "decode_residuals", "encode_residuals_device", "decode_residuals_device", "residual_model_bits",
           "model_counts", "res_status_text", "scale_from_log", "DEFAULT_STREAM_LEN"]
