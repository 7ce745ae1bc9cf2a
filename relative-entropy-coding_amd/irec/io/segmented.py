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
    layout = U._Layout.segmented(blocks_per_res, segment_blocks, "segmented_files_max_K_device")
    return segmented_files_max_K(*_files.gather_heads(blob, offsets, FIXED_BYTES + 4 * layout.R + 12 * layout.n_segments))


# ---- host -----------------------------------------------------------------------------------------------------------------------------------
def encode_files_segmented(seed, image_shape, block_size, K, idx, max_index, blocks_per_res, segment_blocks, n_threads=0):
    """N segmented files at once on host threads (irec_rec_encode_files_segmented), parallel over (image, segment): K [N, T] int32,
    idx [N, T, max_K] int32.  Returns (blob uint8, offsets int64 [N + 1]); ValueError naming the first image that cannot be coded."""
    layout = U._Layout.segmented(blocks_per_res, segment_blocks, "encode_files_segmented")
    K = np.ascontiguousarray(K, dtype=np.int32)
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    U._check_rows(K, idx, layout, "encode_files_segmented")
    return U._encode_rows_host(seed, image_shape, block_size, K, idx, max_index, layout, n_threads, None, "encode_files_segmented")


def _decode_files_segmented_status(blob, offsets, blocks_per_res, segment_blocks, max_K, n_threads=0):
    """irec_rec_decode_files_segmented: (headers [N, 9] uint32, K [N, T], idx [N, T, max_K], status int32 [N]) -- a verdict per file, the
    outputs of a refused one zero."""
    layout = U._Layout.segmented(blocks_per_res, segment_blocks, "decode_files_segmented")
    return U._decode_rows_host_status(blob, offsets, layout, max_K, None, n_threads, "decode_files_segmented")


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
    """U._encode_rows_device_launch for checked rows in segments (irec_rec_encode_files_device_segmented)."""
    import torch
    who = "encode_files_device_segmented"
    layout = U._Layout.segmented(blocks_per_res, segment_blocks, who)
    if not (K.is_cuda and idx.is_cuda and K.dtype == torch.int32 and idx.dtype == torch.int32):
        raise ValueError(f"{who} takes CUDA int32 tensors")
    U._check_rows(K, idx, layout, who)
    return U._encode_rows_device_launch(seed, image_shape, block_size, K, idx, max_index, layout, out, None, who)


def _decode_files_device_segmented_launch(blob, offsets, blocks_per_res, segment_blocks, max_K, on_device=False):
    """U._decode_rows_device_launch for blocks_per_res in segments (irec_rec_decode_files_device_segmented)."""
    who = "decode_files_device_segmented"
    return U._decode_rows_device_launch(blob, offsets, U._Layout.segmented(blocks_per_res, segment_blocks, who), max_K, on_device, None, who)


def encode_files_device_segmented(seed, image_shape, block_size, K, idx, max_index, blocks_per_res, segment_blocks, out=None):
    """encode_files_segmented on the device (irec_rec_encode_files_device_segmented): K [N, T], idx [N, T, max_K] int32 CUDA tensors,
    contiguous or views of one joined [rows][1 + width] tensor (PendingCode.gather_packed_ragged_device).  Returns (blob uint8, offsets
    int64 [N + 1]) as CUDA tensors, byte for byte what encode_files_segmented gives; the only host synchronisation is ONE read-back of
    offsets and status.  out: a CUDA uint8 buffer to write into (a short one costs a second run at the size the first one reports)."""
    layout = U._Layout.segmented(blocks_per_res, segment_blocks, "encode_files_device_segmented")
    n, max_K = (K.shape[0], idx.shape[2]) if K.dim() == 2 and idx.dim() == 3 else (0, 0)
    out = U._device_out(out, lambda: layout.first_cap(n, max_K), K.device, "encode_files_device_segmented")
    return _files.encode_device(lambda o: _encode_files_device_segmented_launch(seed, image_shape, block_size, K, idx, max_index, layout, segment_blocks, o),
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
