"""The `.res` container: an image's pixels, arithmetic-coded under the model's discretized-logistic likelihood given the
reconstruction, so that NAME.rec + NAME.res decode to exactly the uint8 image (csrc/irec_res.hip over csrc/irec_res_core.h;
INTEGRATION.md has the layout).  `.rec` files are untouched by it.

pixels [N, C, H, W] uint8, loc the same shape in float32 (the clamped reconstruction), scale one float32 per call: version-1 files.
A sequence or tensor of C scales, one per channel, in scale's place: version-2 files through the "_scales" entry points.  The device
calls take and return CUDA tensors; the host calls run the same core over numpy arrays and give the same bytes.

The scale is fitted where the data is: scale_bits[_device] gives the exact coded cost of a batch under up to 64 candidate scales
per channel (csrc/irec_res_fit.hip), fit_scales searches over it."""
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
HEADER_BYTES = 28                   # version 1; version 2: header_bytes(channels)
MAX_CANDIDATES = 64                 # IREC_RES_FIT_MAX_CANDIDATES
COST_ENTRIES = 65537                # IREC_RES_COST_ENTRIES
INT64_MAX = 2 ** 63 - 1             # scale_bits' column of a candidate outside the coder's range
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


def _per_channel(scale):
    """Does `scale` name one scale per channel (a sequence, an array or a tensor of one dimension) rather than the call's one?"""
    if hasattr(scale, "dim"):
        return scale.dim() >= 1
    return np.ndim(scale) >= 1


def _scales32(scales, c, who):
    """The C float32 scales of a version-2 call as a numpy array."""
    scales = scales.detach().cpu().numpy() if hasattr(scales, "detach") else scales
    scales = np.ascontiguousarray(scales, dtype=np.float32)
    if scales.shape != (c,):
        raise ValueError(f"{who}: {scales.size} scales of shape {scales.shape} for {c} channels")
    return scales


def _scales_device(scales, c, dev, who):
    """The same on the device: a CUDA float32 tensor stays where it is (no copy, no read-back)."""
    import torch
    if hasattr(scales, "is_cuda") and scales.is_cuda:
        if tuple(scales.shape) != (c,):
            raise ValueError(f"{who}: scales of shape {tuple(scales.shape)} for {c} channels")
        return scales.detach().to(device=dev, dtype=torch.float32).contiguous()
    return torch.from_numpy(_scales32(scales, c, who)).to(dev)


def header_bytes(channels, per_channel):
    """Bytes of a file before its stream length words: 28, or 24 + 4 channels with one scale word per channel (version 2)."""
    return 24 + 4 * int(channels) if per_channel else HEADER_BYTES


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


def max_file_bytes(c, h, w, stream_len, per_channel=False):
    """What one image's .res file can take at the most (MAX_BITS_PER_SYMBOL)."""
    n_sym = c * h * w
    ns = -(-n_sym // stream_len)
    return header_bytes(c, per_channel) + 2 * ns + (MAX_BITS_PER_SYMBOL * n_sym + 2 * ns) // 8 + ns


def version_of(data):
    """The version word of a .res file's bytes (None for bytes too short to hold it)."""
    data = bytes(data[:6])
    return int.from_bytes(data[4:6], "little") if len(data) >= 6 else None


def stream_len_of(data):
    """The stream_len word of a .res file's bytes (None for bytes too short to hold it)."""
    data = bytes(data[:12])
    return int.from_bytes(data[8:12], "little") if len(data) >= 12 else None


# ---- host ---------------------------------------------------------------------------------------------------------------------------
def encode_residuals(pixels, loc, scale, stream_len=None, n_threads=0):
    """N .res files from numpy arrays (irec_res_encode_files): (blob uint8, offsets int64 [N + 1]), file i = blob[offsets[i]:offsets[i + 1]].
    ValueError naming the first image that cannot be coded.  scale: one number, or C of them (irec_res_encode_files_scales, version 2)."""
    lib = _lib.load()
    pixels = np.ascontiguousarray(pixels, dtype=np.uint8)
    loc = np.ascontiguousarray(loc, dtype=np.float32)
    n, c, h, w, stream_len, _ = _shape(pixels.shape, loc.shape, stream_len, "encode_residuals")
    offsets = np.zeros(n + 1, dtype=np.int64)
    status = np.zeros(max(n, 1), dtype=np.int32)
    per_channel = _per_channel(scale)
    scales = _scales32(scale, c, "encode_residuals") if per_channel else None
    cap = n * (header_bytes(c, per_channel) + 2 * -(-(c * h * w) // stream_len) + c * h * w) + 64      # a first guess: a byte per pixel
    for _attempt in range(2):
        out = np.empty(max(cap, 1), dtype=np.uint8)
        if per_channel:
            st = lib.irec_res_encode_files_scales(pixels.ctypes.data, loc.ctypes.data, scales.ctypes.data, n, h, w, c, stream_len,
                                                  out.ctypes.data, out.size, offsets.ctypes.data, status.ctypes.data, int(n_threads))
        else:
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
    if _per_channel(scale):
        scales = _scales32(scale, c, "decode_residuals")
        st = lib.irec_res_decode_files_scales(keep.ctypes.data, offsets.ctypes.data, loc.ctypes.data, scales.ctypes.data, n, h, w, c,
                                              stream_len, pixels.ctypes.data, status.ctypes.data, int(n_threads))
    else:
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
    """The ideal bits of every image under the integer model: sum over its pixels of -log2(count / 65536) (float64 [N]).  scale: one
    number, or one per channel of [N, C, H, W] arrays."""
    lib = _lib.load()
    pixels = pixels.cpu().numpy() if hasattr(pixels, "cpu") else pixels
    loc = loc.cpu().numpy() if hasattr(loc, "cpu") else loc
    pixels = np.ascontiguousarray(pixels, dtype=np.uint8)
    loc = np.ascontiguousarray(loc, dtype=np.float32)
    if pixels.shape != loc.shape or pixels.ndim < 1:
        raise ValueError("residual_model_bits: pixels and loc differ in shape")
    count = np.zeros(pixels.size, dtype=np.uint32)
    if _per_channel(scale):                  # one scale per channel of [N, C, H, W]: the counts channel by channel
        if pixels.ndim != 4:
            raise ValueError("residual_model_bits: per-channel scales go with [N, C, H, W] arrays")
        scales = _scales32(scale, pixels.shape[1], "residual_model_bits")
        count = count.reshape(pixels.shape)
        for ch, s in enumerate(scales):
            px, lc = np.ascontiguousarray(pixels[:, ch]), np.ascontiguousarray(loc[:, ch])
            part = np.zeros(px.size, dtype=np.uint32)
            if lib.irec_res_symbol_counts(px.ctypes.data, lc.ctypes.data, float(s), px.size, part.ctypes.data) != 0:
                raise ValueError(lib.irec_last_error().decode())
            count[:, ch] = part.reshape(px.shape)
    elif lib.irec_res_symbol_counts(pixels.ctypes.data, loc.ctypes.data, _scale32(scale), pixels.size, count.ctypes.data) != 0:
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
        if _per_channel(scale):
            scales = _scales_device(scale, c, dev, "encode_residuals_device")
            st = lib.irec_res_encode_files_device_scales(pixels.data_ptr() if n else None, loc.data_ptr() if n else None, scales.data_ptr(), n,
                                                         h, w, c, stream_len, out.data_ptr() if out.numel() else None, out.numel(),
                                                         offsets.data_ptr(), status.data_ptr() if n else None, ws.data_ptr(), ws.numel(),
                                                         torch.cuda.current_stream().cuda_stream)
        else:
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
        out = torch.empty(max(n * (header_bytes(c, _per_channel(scale)) + 2 * ns + c * h * w) + 64, 1), dtype=torch.uint8, device=loc.device)
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
        if _per_channel(scale):
            scales = _scales_device(scale, c, dev, "decode_residuals_device")
            st = lib.irec_res_decode_files_device_scales(blob.data_ptr() if blob.numel() else ws.data_ptr(), off_dev.data_ptr(),
                                                         loc.data_ptr() if n else None, scales.data_ptr(), n, h, w, c, stream_len,
                                                         pixels.data_ptr() if n else None, status.data_ptr(), ws.data_ptr(), ws.numel(),
                                                         torch.cuda.current_stream().cuda_stream)
        else:
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


# ---- the cost of a batch under candidate scales, and the fit ---------------------------------------------------------------------------
_COST = {}


def cost_table(device=None):
    """cost[n] = rint((16 - log2 n) 2^16), n in 1 .. 65536, cost[0] = 0 (irec_res_cost_table): uint32 numpy [65537], built once; with
    `device` the same as an int32-typed CUDA tensor of those bits, uploaded once per device."""
    if "host" not in _COST:
        lib = _lib.load()
        table = np.zeros(COST_ENTRIES, dtype=np.uint32)
        if lib.irec_res_cost_table(table.ctypes.data) != 0:
            raise ValueError(lib.irec_last_error().decode())
        table.setflags(write=False)
        _COST["host"] = table
    if device is None:
        return _COST["host"]
    import torch
    key = str(torch.device(device))
    if key not in _COST:
        _COST[key] = torch.from_numpy(_COST["host"].view(np.int32).copy()).to(device)
    return _COST[key]


def _candidates(scales, c, who):
    """scales as float32 [C, n_cand] numpy: [n_cand] is every channel's row, [C, n_cand] its own."""
    scales = scales.detach().cpu().numpy() if hasattr(scales, "detach") else scales
    scales = np.asarray(scales, dtype=np.float32)
    if scales.ndim == 1:
        scales = np.broadcast_to(scales, (c, scales.size))
    if scales.ndim != 2 or scales.shape[0] != c or not 1 <= scales.shape[1] <= MAX_CANDIDATES:
        raise ValueError(f"{who}: scales of shape {scales.shape}: [n_cand] or [{c}, n_cand] with 1 <= n_cand <= {MAX_CANDIDATES}")
    return np.ascontiguousarray(scales)


def scale_bits(pixels, loc, scales, n_threads=0):
    """The exact coded cost of numpy images under candidate scales (irec_res_scale_bits): (bits int64 [N, C, n_cand], skipped int).
    bits[i, ch, k]: the model's code length of image i's channel ch under scales[ch, k] in units of 2^-16 bit; INT64_MAX where the
    candidate is outside the coder's range.  skipped: the pixels left out because their loc is not finite."""
    lib = _lib.load()
    pixels = np.ascontiguousarray(pixels, dtype=np.uint8)
    loc = np.ascontiguousarray(loc, dtype=np.float32)
    n, c, h, w, _, _ = _shape(pixels.shape, loc.shape, 1, "scale_bits")
    scales = _candidates(scales, c, "scale_bits")
    bits = np.zeros((n, c, scales.shape[1]), dtype=np.int64)
    skipped = np.zeros((n, c), dtype=np.int64)
    st = lib.irec_res_scale_bits(pixels.ctypes.data, loc.ctypes.data, scales.ctypes.data, cost_table().ctypes.data, n, h, w, c,
                                 scales.shape[1], bits.ctypes.data, skipped.ctypes.data, int(n_threads))
    if st != 0:
        raise ValueError(lib.irec_last_error().decode())
    return bits, int(skipped.sum())


def _scale_bits_device_launch(pixels, loc, scales):
    """One irec_res_scale_bits_device call on the current stream, nothing read back: (bits int64 [N, C, n_cand], skipped int64 [N, C]).
    scales: a CUDA float32 [C, n_cand] tensor."""
    import torch
    lib = _lib.load()
    _check_device(pixels, loc, "scale_bits_device")
    n, c, h, w, _, _ = _shape(pixels.shape, loc.shape, 1, "scale_bits_device")
    n_cand = int(scales.shape[1])
    pixels, loc, scales = pixels.contiguous(), loc.contiguous(), scales.contiguous()
    dev = loc.device
    with torch.cuda.device(dev):
        ws = torch.empty(lib.irec_res_scale_bits_workspace_bytes(n, h, w, c, n_cand), dtype=torch.uint8, device=dev)
        bits = torch.empty((n, c, n_cand), dtype=torch.int64, device=dev)
        skipped = torch.empty((n, c), dtype=torch.int64, device=dev)
        st = lib.irec_res_scale_bits_device(pixels.data_ptr() if n else None, loc.data_ptr() if n else None, scales.data_ptr(),
                                            cost_table(dev).data_ptr(), n, h, w, c, n_cand, bits.data_ptr() if n else None,
                                            skipped.data_ptr() if n else None, ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    _files.check_status(st, "irec_res_scale_bits_device")
    return bits, skipped


def _candidates_device(scales, c, dev, who):
    import torch
    if hasattr(scales, "is_cuda") and scales.is_cuda:
        scales = scales.detach().to(torch.float32)
        if scales.dim() == 1:
            scales = scales.unsqueeze(0).expand(c, -1)
        if scales.dim() != 2 or scales.shape[0] != c or not 1 <= scales.shape[1] <= MAX_CANDIDATES:
            raise ValueError(f"{who}: scales of shape {tuple(scales.shape)}: [n_cand] or [{c}, n_cand] with 1 <= n_cand <= {MAX_CANDIDATES}")
        return scales.contiguous()
    return torch.from_numpy(_candidates(scales, c, who)).to(dev)


def scale_bits_device(pixels, loc, scales):
    """scale_bits on the device (irec_res_scale_bits_device): (bits int64 CUDA [N, C, n_cand], skipped int64 CUDA [N, C]), the host
    form's numbers bit for bit; asynchronous, nothing read back."""
    _check_device(pixels, loc, "scale_bits_device")
    return _scale_bits_device_launch(pixels, loc, _candidates_device(scales, int(pixels.shape[1]), loc.device, "scale_bits_device"))


def residual_model_bits_device(pixels, loc, scale):
    """residual_model_bits from the device form of scale_bits: float64 CUDA [N] = units / 2^16, the model's bits with every pixel's
    share rounded to 2^-16 bit (within N_pixels 2^-17 of residual_model_bits).  No pixel is copied to the host and nothing is read
    back.  scale: one number, or one per channel."""
    import torch
    _check_device(pixels, loc, "residual_model_bits_device")
    c = int(pixels.shape[1])
    if _per_channel(scale):
        scales = _scales_device(scale, c, loc.device, "residual_model_bits_device").reshape(c, 1)
    else:
        scales = torch.full((c, 1), _scale32(scale), dtype=torch.float32, device=loc.device)
    bits, _ = _scale_bits_device_launch(pixels, loc, scales)
    # (a refused scale's INT64_MAX columns do not add up in int64: infinity)
    return torch.where((bits == INT64_MAX).any(dim=2).any(dim=1), torch.full((), float("inf"), dtype=torch.float64, device=loc.device),
                       bits.sum(dim=(1, 2)).to(torch.float64) / 65536.0)


FIT_ROUNDS, FIT_CANDIDATES = 3, 33


def _fit_totals(batches, scales_cn, on_device):
    """Sum over the batches of bits[:, ch, k] -> int64 numpy [C, n_cand] (INT64_MAX columns stay INT64_MAX): on the device the sum is
    kept there and read back once."""
    total = None
    refused = None
    for pixels, loc in batches:
        if on_device:
            import torch
            bits, _ = _scale_bits_device_launch(pixels, loc, scales_cn)
            bad = (bits == INT64_MAX).any(dim=0)
            part = torch.where(bits == INT64_MAX, torch.zeros_like(bits), bits).sum(dim=0)
        else:
            bits, _ = scale_bits(pixels, loc, scales_cn)
            bad = (bits == INT64_MAX).any(axis=0)
            part = np.where(bits == INT64_MAX, 0, bits).sum(axis=0)
        total = part if total is None else total + part
        refused = bad if refused is None else refused | bad
    if total is None:
        raise ValueError("fit_scales: no batches")
    if on_device:
        import torch
        total = torch.where(refused, torch.full_like(total, INT64_MAX), total).cpu().numpy()      # the round's one read-back
    else:
        total = np.where(refused, INT64_MAX, total)
    return total


def _search(evaluate, rows, first, lo, hi):
    """The rounds of fit_scales for `rows` independent rows: first [rows][n] float64 log-scales (sorted; extra candidates allowed);
    evaluate(log_scales [rows][n]) -> int64 [rows][n].  Returns (best log-scale, its bits, every (log-scale, bits) evaluated, and the
    last round's (grid, index of its best)) per row."""
    seen = [dict() for _ in range(rows)]
    grids = [np.asarray(g, dtype=np.float64) for g in first]
    last = [None] * rows
    step = (hi - lo) / (FIT_CANDIDATES - 1)
    for _round in range(FIT_ROUNDS):
        width = max(len(g) for g in grids)
        padded = np.stack([np.concatenate([g, np.full(width - len(g), g[-1])]) for g in grids])
        bits = evaluate(padded)
        centres = []
        for r in range(rows):
            n = len(grids[r])
            for v, b in zip(padded[r, :n], bits[r, :n]):
                seen[r][float(v)] = int(b)
            span = [(int(b), float(v)) for v, b in zip(padded[r, :FIT_CANDIDATES], bits[r, :FIT_CANDIDATES])]   # the round's own span
            k = min(range(len(span)), key=lambda j: span[j])
            last[r] = (padded[r, :FIT_CANDIDATES].copy(), k)
            centres.append(min((b, v) for v, b in seen[r].items())[1])               # least bits; ties: the smaller scale
        grids = [np.linspace(max(lo, cv - step), min(hi, cv + step), FIT_CANDIDATES) for cv in centres]
        step = 2.0 * step / (FIT_CANDIDATES - 1)
    out = []
    for r in range(rows):
        b, v = min((b, v) for v, b in seen[r].items())
        out.append((v, b, sorted(seen[r].items()), last[r]))
    return out


def fit_scales(batches, per_channel=False, start=None, lo=-9.0, hi=1.0):
    """The log-scale(s) of least coded cost for `batches`, an iterable of (pixels, loc) pairs -- CUDA tensors (scale_bits_device; the
    bits are summed over the batches on the device, one small read-back per round) or numpy arrays (the host twin, scale_bits).
    Coarse to fine over the log-scale in three rounds of 33 candidates: round 1 spans [lo, hi] (plus `start` if given), each later
    round one step either side of the best so far.  The answer is the candidate of least total bits among ALL evaluated, ties to the
    smaller scale; per_channel=True first fits one scale, then runs the rounds per channel with that scale among every channel's
    candidates.  Returns (log_scales, bits, evaluated): a float and an int for one scale, float64 [C] and int64 [C] per channel
    (bits in units of 2^-16 bit over all batches); evaluated: {"single": [(log_scale, bits), ...], "channels": [[...] per channel] or
    None, "last_round": per fitted row (grid float64 [33], index of its best)}.
    A candidate's float32 scale is scale_from_log(log_scale), the value a model's likelihood_log_scale gives."""
    batches = list(batches)
    if not batches:
        raise ValueError("fit_scales: no batches")
    on_device = hasattr(batches[0][0], "is_cuda")
    c = int(batches[0][0].shape[1])
    if not lo < hi:
        raise ValueError("fit_scales: lo must be below hi")

    def to_scales(log_scales):
        return np.array([[scale_from_log(v) for v in row] for row in log_scales], dtype=np.float32)

    def evaluate_single(log_scales):                        # one row: the same candidates for every channel, the channels' bits added
        scales = np.broadcast_to(to_scales(log_scales), (c, log_scales.shape[1]))
        total = _fit_totals(batches, _device_scales(scales, batches) if on_device else scales, on_device)
        refused = (total == INT64_MAX).any(axis=0)
        return np.where(refused, INT64_MAX, np.where(total == INT64_MAX, 0, total).sum(axis=0))[None, :]

    def evaluate_channels(log_scales):
        scales = to_scales(log_scales)
        return _fit_totals(batches, _device_scales(scales, batches) if on_device else scales, on_device)

    first = np.linspace(lo, hi, FIT_CANDIDATES)
    if start is not None:
        first = np.concatenate([first, [float(start)]])
    (single, single_bits, single_seen, single_last), = _search(evaluate_single, 1, [first], lo, hi)
    if not per_channel:
        return single, single_bits, {"single": single_seen, "channels": None, "last_round": [single_last]}
    first = np.concatenate([np.linspace(lo, hi, FIT_CANDIDATES), [single]])
    rows = _search(evaluate_channels, c, [first] * c, lo, hi)
    return (np.array([r[0] for r in rows], dtype=np.float64), np.array([r[1] for r in rows], dtype=np.int64),
            {"single": single_seen, "channels": [r[2] for r in rows], "last_round": [r[3] for r in rows]})


def _device_scales(scales, batches):
    import torch
    return torch.from_numpy(np.ascontiguousarray(scales, dtype=np.float32)).to(batches[0][1].device)


def scale_from_log(log_scale):
    """The call's float32 scale from a likelihood_log_scale value: exp in float64, rounded once to float32."""
    return float(np.float32(math.exp(float(log_scale))))


__all__ = ["encode_residuals", "decode_residuals", "encode_residuals_device", "decode_residuals_device", "residual_model_bits",
           "model_counts", "res_status_text", "scale_from_log", "DEFAULT_STREAM_LEN", "cost_table", "scale_bits", "scale_bits_device",
           "residual_model_bits_device", "fit_scales"]
