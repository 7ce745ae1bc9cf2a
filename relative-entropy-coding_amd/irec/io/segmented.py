"""Segmented `.rec` files (NAME.recs): an opt-in second container for few, long index streams.

A residual block's rows are cut into segments of `segment_blocks` coder blocks; every segment is a pair of ordinary streams -- what
write_compressed_code writes for those blocks alone -- and lanes (csrc/irec_rec_seg.hip) or host threads run over segments.  Little-endian:

    0   magic "IRSG" | 4  version u16 = 1, reserved u16 = 0 | 8  the 28-byte static header of .rec (both flags 0) | 36  segment_blocks u32
    40  R x u32 blocks per residual block
    40 + 4 R  directory: for r, for s < ceil(blocks[r] / segment_blocks):  max_part u32, count_bytes u32, index_bytes u32
    then the streams in directory order: each segment's count stream, then its index stream

Every call works over rows like the ragged calls of irec.io.utils: K [N, T], idx [N, T, max_K], T = sum(blocks_per_res).  Default
symbol models only."""
import struct

import numpy as np

from .. import _lib
from . import _files
from . import utils as U

MAGIC = _lib.REC_SEG_MAGIC
FIXED_BYTES = 40                                         # magic, version, reserved, static header, segment_blocks
_FIXED = struct.Struct("<4sHHIIIIIHHHHI")

_SEG_STATUS_TEXT = {
    _lib.IREC_REC_E_SEG_MAGIC: "irec_rec_decode_files_segmented: not a segmented file of version 1 (magic, version or reserved word)",
    _lib.IREC_REC_E_SEG_DIRECTORY: "irec_rec_decode_files_segmented: header, directory and the streams it lists are not the file's length",
    _lib.IREC_REC_E_SEG_BLOCKS: "irec_rec_decode_files_segmented: segment_blocks is 0 or differs from the call's",
}


def seg_status_text(status):
    """irec_rec_status -> text: the plain container's causes, and the three the segmented reader adds."""
    return _SEG_STATUS_TEXT.get(status) or U._rec_status_text(status)


def _raise_first_status(status):
    _files.raise_first_status(status, seg_status_text)


def is_segmented(data):
    """Whether a file's bytes begin with the segmented container's magic (a plain .rec begins with its seed)."""
    return bytes(memoryview(np.ascontiguousarray(data))[:4] if isinstance(data, np.ndarray) else data[:4]) == MAGIC


def segmented_header_words(data):
    """The fixed part of a segmented file from its first 40 bytes (+ 4 R for the block counts): a dict of seed, image_shape (h, w, c),
    block_size, max_index, R, segment_blocks, version and -- where the bytes hold them -- bpt (blocks per residual block, a list); None for
    bytes that are too short or do not begin with the magic."""
    data = bytes(memoryview(np.ascontiguousarray(data)) if isinstance(data, np.ndarray) else data)
    if len(data) < FIXED_BYTES or data[:4] != MAGIC:
        return None
    _, version, _reserved, seed, block_size, max_index, h, w, c, _f0, _f1, r, g = _FIXED.unpack(data[:FIXED_BYTES])
    bpt = list(struct.unpack(f"<{r}I", data[FIXED_BYTES:FIXED_BYTES + 4 * r])) if len(data) >= FIXED_BYTES + 4 * r else None
    return {"seed": seed, "image_shape": (h, w, c), "block_size": block_size, "max_index": max_index, "R": r, "segment_blocks": g,
            "version": version, "bpt": bpt}


def segment_blocks_of(data):
    """The segment_blocks word of a segmented file's bytes (None for bytes too short to hold it or of another container)."""
    words = segmented_header_words(data[:FIXED_BYTES])
    return None if words is None else words["segment_blocks"]


def segmented_files_max_K(blob, offsets):
    """Index slots per block that decode the segmented files blob[offsets[i]:offsets[i + 1]] (host bytes): the largest max_part word of
    their directories, at least 1.  A word above IREC_MAX_PARTITIONS does not count (the reader refuses that file whatever max_K is), and
    a directory that leaves its file is read as far as the file goes."""
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    need = 1
    for i in range(len(offsets) - 1):
        raw = blob[int(offsets[i]):int(offsets[i + 1])]
        words = segmented_header_words(raw[:FIXED_BYTES + 4 * _lib.REC_RAGGED_MAX_RES])
        if words is None or not words["bpt"] or words["segment_blocks"] < 1:
            continue
        g = words["segment_blocks"]
        n_seg = min(sum(-(-b // g) for b in words["bpt"]), (raw.size - FIXED_BYTES - 4 * words["R"]) // 12)
        if n_seg > 0:
            at = FIXED_BYTES + 4 * words["R"]
            mp = np.frombuffer(raw[at:at + 12 * n_seg].tobytes(), dtype="<u4")[::3]
            mp = mp[mp <= _lib.MAX_PARTITIONS]
            need = max(need, int(mp.max()) if mp.size else 1)
    return need


def segmented_files_max_K_device(blob, offsets, blocks_per_res, segment_blocks):
    """segmented_files_max_K for a blob on the device: only the fixed part and the directory of every file (40 + 4 R + 12 S bytes, by
    the call's layout) are gathered and copied to the host."""
    import torch
    layout, g, n_seg = _layout(blocks_per_res, segment_blocks, "segmented_files_max_K_device")
    dev, hb = blob.device, FIXED_BYTES + 4 * layout.R + 12 * n_seg
    off = offsets.to(dev) if hasattr(offsets, "is_cuda") else torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.int64)).to(dev)
    n = off.numel() - 1
    if n < 1 or blob.numel() < 1:
        return 1
    at = (off[:-1, None] + torch.arange(hb, device=dev)).clamp_(0, blob.numel() - 1)
    whole = (off[1:] - off[:-1] >= hb) & (off[:-1] >= 0) & (off[1:] <= blob.numel())              # a shorter file: a zero header, no words
    head = blob.reshape(-1)[at] * whole[:, None].to(torch.uint8)
    return segmented_files_max_K(head.cpu().numpy().reshape(-1), np.arange(n + 1, dtype=np.int64) * hb)


def _layout(blocks_per_res, segment_blocks, who):
    layout = U._Layout.ragged(blocks_per_res, who)
    g = int(segment_blocks)
    if g < 1 or g > _lib.INT32_MAX:
        raise ValueError(f"{who}: segment_blocks must be at least 1 (got {segment_blocks})")
    return layout, g, int(sum(-(-int(b) // g) for b in layout.bpr))


def _first_cap(n, layout, g, n_seg, max_K):
    """A first allowance: the fixed parts, and 64 + 40 bits per symbol and terminator of every stream (irec_io.cpp's own)."""
    blocks = int(layout.bpr.astype(np.int64).sum())
    return n * (FIXED_BYTES + 4 * layout.R + n_seg * (12 + 2 * 9 + 2 * 5) + 5 * blocks * (1 + max_K))


# ---- host -----------------------------------------------------------------------------------------------------------------------------------
def encode_files_segmented(seed, image_shape, block_size, K, idx, max_index, blocks_per_res, segment_blocks, n_threads=0):
    """N segmented files at once on host threads (irec_rec_encode_files_segmented), parallel over (image, segment): K [N, T] int32,
    idx [N, T, max_K] int32.  Returns (blob uint8, offsets int64 [N + 1]); ValueError naming the first image that cannot be coded."""
    lib = _lib.load()
    layout, g, n_seg = _layout(blocks_per_res, segment_blocks, "encode_files_segmented")
    K = np.ascontiguousarray(K, dtype=np.int32)
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    if K.ndim != 2 or K.shape[1] != layout.T or idx.ndim != 3 or idx.shape[:2] != K.shape:
        raise ValueError(f"encode_files_segmented: K {K.shape} and idx {idx.shape} are not [N, {layout.T}] and [N, {layout.T}, max_K]")
    n, max_K = K.shape[0], idx.shape[2]
    h, w, c = (int(v) for v in image_shape)
    offsets = np.zeros(n + 1, dtype=np.int64)
    status = np.zeros(max(n, 1), dtype=np.int32)

    def call(out):
        total = lib.irec_rec_encode_files_segmented(int(seed), int(block_size), int(max_index), h, w, c, n, layout.R, layout.bpr.ctypes.data, g,
                                                    max_K, K.ctypes.data, idx.ctypes.data if idx.size else None, out.ctypes.data, out.size,
                                                    offsets.ctypes.data, status.ctypes.data, int(n_threads))
        if total < 0:
            raise ValueError(lib.irec_last_error().decode())
        _raise_first_status(status[:n])
        return total
    return _files.encode_host(call, max(_first_cap(n, layout, g, n_seg, max_K), 1)), offsets


def _decode_files_segmented_status(blob, offsets, blocks_per_res, segment_blocks, max_K, n_threads=0):
    """irec_rec_decode_files_segmented: (headers [N, 9] uint32, K [N, T], idx [N, T, max_K], status int32 [N]) -- a verdict per file, the
    outputs of a refused one zero."""
    lib = _lib.load()
    layout, g, _ = _layout(blocks_per_res, segment_blocks, "decode_files_segmented")
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    offsets = _files.host_offsets(offsets, blob.size, "decode_files_segmented")
    n = offsets.size - 1
    hdr = np.zeros((max(n, 1), 9), dtype=np.uint32)
    K = np.zeros((n, layout.T), dtype=np.int32)
    idx = np.zeros((n, layout.T, int(max_K)), dtype=np.int32)
    status = np.zeros(max(n, 1), dtype=np.int32)
    pad = np.zeros(1, dtype=np.uint8)
    st = lib.irec_rec_decode_files_segmented(blob.ctypes.data if blob.size else pad.ctypes.data, offsets.ctypes.data, n, layout.R,
                                             layout.bpr.ctypes.data, g, int(max_K), hdr.ctypes.data, K.ctypes.data if K.size else pad.ctypes.data,
                                             idx.ctypes.data if idx.size else None, status.ctypes.data, int(n_threads))
    if st != 0:
        raise ValueError(lib.irec_last_error().decode())
    return hdr[:n], K, idx, status[:n]


def decode_files_segmented(blob, offsets, blocks_per_res, max_K, segment_blocks=None, n_threads=0):
    """The inverse of encode_files_segmented (irec_rec_decode_files_segmented): (headers [N, 9] uint32, K [N, T], idx [N, T, max_K] with
    rows zero-filled past K); ValueError naming the first file that is damaged, of another structure or of another segment size.
    segment_blocks None: the word of the first file's header."""
    if segment_blocks is None:
        offsets = np.asarray(offsets.cpu() if hasattr(offsets, "cpu") else offsets)
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        segment_blocks = segment_blocks_of(blob[int(offsets[0]):int(offsets[1])][:FIXED_BYTES]) if len(offsets) >= 2 else 1
        if not segment_blocks:
            raise ValueError("decode_files_segmented: the first file is not a segmented file (no magic, or segment_blocks 0)")
    hdr, K, idx, status = _decode_files_segmented_status(blob, offsets, blocks_per_res, segment_blocks, max_K, n_threads)
    _raise_first_status(status)
    return hdr, K, idx


# ---- device: CUDA tensors in and out, the launches on the current stream ------------------------------------------------------------------
def _encode_files_device_segmented_launch(seed, image_shape, block_size, K, idx, max_index, blocks_per_res, segment_blocks, out):
    """One irec_rec_encode_files_device_segmented call on the current stream over rows K [N, T], idx [N, T, max_K], nothing read back:
    (offsets int64 [N + 1], status int32 [N], both views of `both`, which one copy fetches).  The bytes are in `out` only if
    offsets[N] <= out.numel()."""
    import torch
    lib = _lib.load()
    who = "encode_files_device_segmented"
    layout, g, _ = _layout(blocks_per_res, segment_blocks, who)
    if not (K.is_cuda and idx.is_cuda and K.dtype == torch.int32 and idx.dtype == torch.int32):
        raise ValueError(f"{who} takes CUDA int32 tensors")
    if K.dim() != 2 or K.shape[1] != layout.T or idx.dim() != 3 or tuple(idx.shape[:2]) != tuple(K.shape):
        raise ValueError(f"{who}: K {tuple(K.shape)} and idx {tuple(idx.shape)} are not [N, {layout.T}] and [N, {layout.T}, max_K]")
    n, max_K = K.shape[0], idx.shape[2]
    h, w, c = (int(v) for v in image_shape)
    K, ks, idx, ist = U._row_strides(K, idx)
    dev = K.device
    with torch.cuda.device(dev):
        ws = torch.empty(max(lib.irec_rec_seg_workspace_bytes(n, layout.R, layout.bpr.ctypes.data, g), 8), dtype=torch.uint8, device=dev)
        offsets, status, both = _files.offsets_and_status(n, dev)
        st = lib.irec_rec_encode_files_device_segmented(
            int(seed), int(block_size), int(max_index), h, w, c, n, layout.R, layout.bpr.ctypes.data, g, max_K, K.data_ptr(), ks,
            idx.data_ptr() if idx.numel() else None, ist, out.data_ptr() if out.numel() else None, out.numel(), offsets.data_ptr(),
            status.data_ptr() if n else None, ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    _files.check_status(st, "irec_rec_encode_files_device_segmented")
    return offsets, status, both


def _decode_files_device_segmented_launch(blob, offsets, blocks_per_res, segment_blocks, max_K, on_device=False):
    """One irec_rec_decode_files_device_segmented call on the current stream: (headers int32 [N, 9] holding the uint32 words, K [N, T],
    idx [N, T, max_K], status int32 [N]) on the device.  Nothing is read back (U._decode_rows_device_launch's rules for the offsets)."""
    import torch
    lib = _lib.load()
    who = "decode_files_device_segmented"
    layout, g, _ = _layout(blocks_per_res, segment_blocks, who)
    if not (blob.is_cuda and blob.dtype == torch.uint8):
        raise ValueError(f"{who} takes a CUDA uint8 tensor")
    blob = blob.contiguous()
    dev = blob.device
    max_K = int(max_K)
    offsets = _files.device_offsets(offsets, blob, dev, on_device, who)
    n = offsets.numel() - 1
    with torch.cuda.device(dev):
        ws = torch.empty(max(lib.irec_rec_seg_workspace_bytes(n, layout.R, layout.bpr.ctypes.data, g), 8), dtype=torch.uint8, device=dev)
        hdr = torch.zeros((n, 9), dtype=torch.int32, device=dev)
        K = torch.empty((n, layout.T), dtype=torch.int32, device=dev)
        idx = torch.empty((n, layout.T, max_K), dtype=torch.int32, device=dev)
        status = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
        st = lib.irec_rec_decode_files_device_segmented(
            blob.data_ptr() if blob.numel() else ws.data_ptr(), offsets.data_ptr(), n, layout.R, layout.bpr.ctypes.data, g, max_K,
            hdr.data_ptr(), K.data_ptr(), idx.data_ptr() if idx.numel() else None, status.data_ptr(), ws.data_ptr(), ws.numel(),
            torch.cuda.current_stream().cuda_stream)
    _files.check_status(st, "irec_rec_decode_files_device_segmented")
    return hdr, K, idx, status[:n]


def encode_files_device_segmented(seed, image_shape, block_size, K, idx, max_index, blocks_per_res, segment_blocks, out=None):
    """encode_files_segmented on the device (irec_rec_encode_files_device_segmented): K [N, T], idx [N, T, max_K] int32 CUDA tensors,
    contiguous or views of one joined [rows][1 + width] tensor (PendingCode.gather_packed_ragged_device).  Returns (blob uint8, offsets
    int64 [N + 1]) as CUDA tensors, byte for byte what encode_files_segmented gives; the only host synchronisation is ONE read-back of
    offsets and status.  out: a CUDA uint8 buffer to write into (a short one costs a second run at the size the first one reports)."""
    layout, g, n_seg = _layout(blocks_per_res, segment_blocks, "encode_files_device_segmented")
    n, max_K = (K.shape[0], idx.shape[2]) if K.dim() == 2 and idx.dim() == 3 else (0, 0)
    out = U._device_out(out, lambda: _first_cap(n, layout, g, n_seg, max_K), K.device, "encode_files_device_segmented")
    return _files.encode_device(lambda o: _encode_files_device_segmented_launch(seed, image_shape, block_size, K, idx, max_index, layout, g, o),
                                K.shape[0], out, seg_status_text, "irec_rec_encode_files_device_segmented")


def decode_files_device_segmented(blob, offsets, blocks_per_res, max_K, segment_blocks=None):
    """decode_files_segmented on the device (irec_rec_decode_files_device_segmented): blob uint8 CUDA tensor, offsets [N + 1] (CUDA, CPU
    or numpy).  Returns CUDA tensors (headers [N, 9] int64, K [N, T] int32, idx [N, T, max_K] int32 with rows zero-filled past K);
    ValueError naming the first damaged file.  segment_blocks None: the word of the first file's header (a 40-byte read-back)."""
    import torch
    if segment_blocks is None:
        first = int(offsets[0])
        segment_blocks = segment_blocks_of(blob[first:min(first + FIXED_BYTES, int(offsets[1]))].cpu().numpy().tobytes()) if len(offsets) >= 2 else 1
        if not segment_blocks:
            raise ValueError("decode_files_device_segmented: the first file is not a segmented file (no magic, or segment_blocks 0)")
    hdr, K, idx, status = _decode_files_device_segmented_launch(blob, offsets, blocks_per_res, segment_blocks, max_K)
    _raise_first_status(status.cpu().numpy())
    return hdr.to(torch.int64) & 0xFFFFFFFF, K, idx
