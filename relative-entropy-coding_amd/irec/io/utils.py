"""The `.rec` container (wire format of the reference, rec/io/utils.py:7-215).

Layout, all little-endian native `struct` fields as the reference writes them:

    static header  'IIIIIHHHH'   seed, block_size, max_index, height, width, channels,
                                 uses_num_aux_var_counts_file, uses_index_counts_file, R   (R = residual blocks)
    dynamic header 4 x R x 'I'   blocks per residual block | byte length of each "count" stream |
                                 byte length of each index stream | largest partition count per residual block
    R count streams, then R index streams

A stream is an arithmetic-coded message (values + 1, terminated by symbol 0; model = counts of 1 for the terminator and
101 / 1001 for everything else) with a marker 1 bit in front, right-aligned in big-endian bytes.  The entropy coder
is the C++ one of libirec_hip.so (irec.io.ArithmeticCoder).  Bytes are identical to the reference's writer
(tests/test_rec_io.py).
"""
import itertools
import struct
from dataclasses import dataclass
from typing import List, Sequence, Tuple

import numpy as np

from .. import _lib
from . import _files
from .entropy_coding import ArithmeticCoder

_STATIC = struct.Struct("IIIIIHHHH")


def header_seed(seed, who):
    """The seed as the uint32 header field of a .rec / .recs file holds it, or ValueError: a file can only name a coding seed in
    [0, 2^32), and decompress codes under the seed it reads -- the coders take any int64, and ctypes would wrap one silently into the
    field (2^32 + 5 -> 5, -1 -> 4294967295: a file that decodes to another image without an error).  THE check of every writer, host
    and device, and of the drivers above them, which call it before they code anything."""
    try:
        value = _lib.seed_int(seed)
    except ValueError as e:
        raise ValueError(f"{who}: {e} (the seed of a .rec header: an integer in [0, 2^32))")
    if not 0 <= value <= _lib.HEADER_SEED_MAX:
        raise ValueError(f"{who}: seed {value} does not fit the uint32 seed field of a .rec header: a seed that goes into a file "
                         f"must lie in [0, 2^32) = [0, {_lib.HEADER_SEED_MAX}]")
    return value


def _uniform_model(n_values: int, weight: int) -> np.ndarray:
    """Terminator count 1, every value symbol `1 + weight` (utils.py:31-35 with weight 1000, :41-47 with weight 100)."""
    model = np.full(n_values + 1, 1 + weight, dtype=np.int64)
    model[0] = 1
    return model


def _bits_to_bytes(code: Sequence[str]) -> bytes:
    lib = _lib.load()
    bits = np.frombuffer("".join(code).encode("ascii"), dtype=np.uint8) if len(code) else np.zeros(0, np.uint8)
    out = np.empty((bits.size + 8) // 8, dtype=np.uint8)
    n = lib.irec_rec_pack_bits(bits.ctypes.data if bits.size else None, bits.size, out.ctypes.data, out.size)
    if n < 0:
        raise ValueError("irec_rec_pack_bits failed")
    return out[:n].tobytes()


def _bytes_to_bits(data: bytes) -> str:
    lib = _lib.load()
    buf = np.frombuffer(data, dtype=np.uint8)
    out = np.empty(max(buf.size * 8, 1), dtype=np.uint8)
    n = lib.irec_rec_unpack_bits(buf.ctypes.data if buf.size else None, buf.size, out.ctypes.data, out.size)
    if n < 0:
        raise ValueError("corrupt .rec stream (no marker bit)")
    return out[:n].tobytes().decode("ascii")


def _encode_stream(model: np.ndarray, values) -> bytes:
    message = np.append(np.asarray(values, dtype=np.int64).reshape(-1) + 1, 0)
    return _bits_to_bytes(ArithmeticCoder(model, precision=32).encode(message))


def _decode_stream(model: np.ndarray, data: bytes) -> np.ndarray:
    message = ArithmeticCoder(model, precision=32).decode_fast(_bytes_to_bits(data))
    return np.asarray(message[:-1], dtype=np.int64) - 1


@dataclass
class RecHeader:
    seed: int
    block_size: int
    max_index: int
    image_shape: Tuple[int, int, int]
    uses_count_file: bool
    uses_index_file: bool
    blocks_per_res_block: List[int]
    count_stream_bytes: List[int]
    index_stream_bytes: List[int]
    max_partitions: List[int]

    def pack(self) -> bytes:
        r = len(self.blocks_per_res_block)
        tail = [*self.blocks_per_res_block, *self.count_stream_bytes, *self.index_stream_bytes,
                *[m & 0xFFFFFFFF for m in self.max_partitions]]
        return _STATIC.pack(header_seed(self.seed, "RecHeader.pack"), self.block_size, self.max_index, *self.image_shape, int(self.uses_count_file),
                            int(self.uses_index_file), r) + struct.pack(f"{4 * r}I", *tail)

    @classmethod
    def read(cls, fh, static_header_size=_STATIC.size) -> "RecHeader":
        seed, block_size, max_index, h, w, c, f_counts, f_index, r = _STATIC.unpack(fh.read(static_header_size))
        tail = struct.unpack(f"{4 * r}I", fh.read(16 * r))
        return cls(seed, block_size, max_index, (h, w, c), bool(f_counts), bool(f_index), list(tail[:r]),
                   list(tail[r:2 * r]), list(tail[2 * r:3 * r]), list(tail[3 * r:]))


def _native_encode(seed, image_shape, block_size, block_indices, max_index):
    """The whole container in one C++ call (irec_rec_encode_file): default symbol models only."""
    lib = _lib.load()
    seed = header_seed(seed, "write_compressed_code")
    bpr = np.array([len(rb) for rb in block_indices], dtype=np.int32)
    K = np.array([len(ix) for rb in block_indices for ix in rb], dtype=np.int32)
    flat = np.fromiter(itertools.chain.from_iterable(itertools.chain.from_iterable(block_indices)), dtype=np.int32,
                       count=int(K.sum()))
    h, w, c = (int(v) for v in image_shape)

    def call(out):
        n = lib.irec_rec_encode_file(seed, int(block_size), int(max_index), h, w, c, len(bpr), bpr.ctypes.data,
                                     K.ctypes.data, flat.ctypes.data if flat.size else None, out.ctypes.data, out.size)
        if n < 0:
            raise ValueError(lib.irec_io_last_error().decode())
        return n
    return _files.encode_host(call, 64 + 16 * len(bpr) + 4 * (K.size + flat.size) + 64).tobytes()


def _native_decode(data):
    lib = _lib.load()
    buf = np.frombuffer(data, dtype=np.uint8)
    hdr = np.zeros(9, dtype=np.uint32)
    sizes = np.zeros(3, dtype=np.int64)
    # first try with buffers sized from the header (block counts) and the file size (an index costs >= 2 bits unless
    # max_index is tiny); the library reports the exact sizes if they were short, and only then is the file decoded twice
    n_res = int(np.frombuffer(data[26:28], dtype="<u2")[0]) if len(data) >= 28 else 0
    n_blk = int(np.frombuffer(data[28:28 + 4 * n_res], dtype="<u4").sum()) if len(data) >= 28 + 4 * n_res else 0
    n_blk = min(n_blk, 8 * len(data) + 8)            # (a damaged header: a coded block costs at least a bit of its count stream)
    sizes[:] = (n_res, n_blk, 4 * len(data) + 1024)
    for _attempt in range(2):
        bpr = np.empty(max(int(sizes[0]), 1), dtype=np.int32)
        K = np.empty(max(int(sizes[1]), 1), dtype=np.int32)
        idx = np.empty(max(int(sizes[2]), 1), dtype=np.int32)
        st = lib.irec_rec_decode_file(buf.ctypes.data, buf.size, hdr.ctypes.data, sizes.ctypes.data, bpr.ctypes.data, bpr.size,
                                      K.ctypes.data, K.size, idx.ctypes.data, idx.size)
        if st != _lib.IREC_E_WORKSPACE:
            break
    if st != 0:
        raise ValueError(lib.irec_io_last_error().decode())
    blocks, kb, ib = [], 0, 0
    for r in range(int(sizes[0])):
        rb = []
        for _ in range(int(bpr[r])):
            k = int(K[kb]); kb += 1
            rb.append(idx[ib:ib + k].tolist()); ib += k
        blocks.append(rb)
    return int(hdr[0]), (int(hdr[3]), int(hdr[4]), int(hdr[5])), int(hdr[1]), blocks


# ---- N containers at once: csrc/irec_io.cpp on the host, csrc/irec_rec.hip (one lane per stream over csrc/irec_rec_core.h) on the device
#      and, host or device, under symbol tables ----------------------------------------------------------------------------------------
# Every call works over rows: K [N, T], idx [N, T, max_K], T rows per image, block j of residual block r of image i at row
# i T + first[r] + j.  The [N, R, bpt] of a call whose residual blocks are all of one size are the same rows seen as [N, R bpt].
# irec_rec_status of include/irec.h -> the text the host coder gives for that cause
_REC_STATUS_TEXT = {
    1: "irec_rec_encode_files: K out of range",
    2: "irec_rec_encode_file: an index does not fit max_index (or max_index exceeds what the 32-bit coder's range holds, ~1.07 million)",
    3: "irec_rec_encode_file: an index does not fit max_index (or max_index exceeds what the 32-bit coder's range holds, ~1.07 million)",
    4: "irec_rec_decode_file: truncated header",
    5: "irec_rec_decode_file: file uses empirical count tables (not the default models)",
    6: "irec_rec_decode_file: max_index out of range (damaged header?)",
    7: "irec_rec_decode_file: partition / block counts out of range (damaged header?)",
    8: "irec_rec_decode_file: truncated streams",
    9: "irec_rec_decode_file: corrupt count stream", 10: "irec_rec_decode_file: corrupt count stream",
    11: "irec_rec_decode_file: corrupt count stream",
    12: "irec_rec_decode_file: corrupt index stream", 13: "irec_rec_decode_file: corrupt index stream",
    14: "irec_rec_decode_file: corrupt index stream", 15: "irec_rec_decode_file: corrupt index stream",
    16: "irec_rec_decode_file: streams do not match the header",
    17: "irec_rec_decode_files: block structure differs",
    18: "irec_rec_decode_files: more partitions than max_K",
    19: "irec_rec: a symbol table whose entries cannot be coded under (cum[0] != 0, a total above 2^30, or an empty interval)",
}


def _rec_status_text(status):
    return _REC_STATUS_TEXT.get(status, "irec_rec: status %d" % status)


def _raise_first_status(status):
    """ValueError with the host's text and its "(image i)" suffix for the first image whose status is nonzero."""
    _files.raise_first_status(status, _rec_status_text)


class _Layout:
    """The blocks per residual block of a call: R residual blocks of bpt blocks each (uniform: any R the container holds), or one count
    per residual block (ragged: the two-level lossy model codes 13 blocks at level 2 and 302 at level 1).  bpr int32 [R] either way,
    T = sum(bpr) rows per image.  segment_blocks: the segmented container's cut of every residual block (irec.io.segmented), None for
    the reference's."""

    def __init__(self, R, bpt=None, bpr=None, segment_blocks=None):
        self.R, self.bpt, self.segment_blocks = int(R), bpt, segment_blocks
        self.bpr = np.full(self.R, bpt, dtype=np.int32) if bpr is None else bpr
        self.T = self.R * bpt if bpr is None else int(bpr.sum())

    @classmethod
    def ragged(cls, blocks_per_res, what):
        if isinstance(blocks_per_res, cls):
            return blocks_per_res
        bpr = np.ascontiguousarray(np.asarray(blocks_per_res, dtype=np.int64).reshape(-1))
        if bpr.size < 1 or (bpr < 1).any() or int(bpr.sum()) > _lib.INT32_MAX:
            raise ValueError(f"{what}: blocks_per_res must hold at least one entry, every entry >= 1, their sum an int32 (got {list(bpr)})")
        return cls(bpr.size, bpr=bpr.astype(np.int32))

    @classmethod
    def segmented(cls, blocks_per_res, segment_blocks, what):
        """The ragged layout of blocks_per_res in segments of segment_blocks coder blocks (a layout of that segment size: itself)."""
        ragged = cls.ragged(blocks_per_res, what)
        g = int(segment_blocks)
        if ragged.segment_blocks is not None and ragged.segment_blocks != g:
            raise ValueError(f"{what}: a layout in segments of {ragged.segment_blocks} blocks, not of {segment_blocks}")
        if ragged.segment_blocks is not None:
            return ragged
        if g < 1 or g > _lib.INT32_MAX:
            raise ValueError(f"{what}: segment_blocks must be at least 1 (got {segment_blocks})")
        return cls(ragged.R, bpr=ragged.bpr, segment_blocks=g)

    @property
    def n_segments(self):
        return int(sum(-(-int(b) // self.segment_blocks) for b in self.bpr))

    def entry(self, tables):
        """(the suffix of the library entry a call of this layout reaches, its layout arguments): the entries without a suffix take one
        count, `_ragged` an array; any tables go to `_tables`, which takes the array (at most REC_RAGGED_MAX_RES entries); `_segmented`
        takes the array and the segment size."""
        if self.segment_blocks is not None:
            return "_segmented", (self.bpr.ctypes.data, self.segment_blocks)
        if tables is not None:
            return "_tables", (self.bpr.ctypes.data,)
        return ("", (self.bpt,)) if self.bpt is not None else ("_ragged", (self.bpr.ctypes.data,))

    def first_cap(self, n, max_K):
        """irec_io.cpp's own first allowance for the files of n images: 64 + 40 bits per symbol and terminator, per stream."""
        b = self.bpr.astype(np.int64)
        if self.segment_blocks is not None:
            return n * (40 + 4 * self.R + self.n_segments * (12 + 2 * 9 + 2 * 5) + 5 * int(b.sum()) * (1 + max_K))
        return n * (28 + 16 * self.R + int(((64 + 40 * (b + 1)) // 8 + 1 + (64 + 40 * (b * max_K + 1)) // 8 + 1).sum()))

    def workspace_bytes(self, lib, n):
        """The workspace a device call of this layout over n images takes."""
        if self.segment_blocks is not None:
            return lib.irec_rec_seg_workspace_bytes(n, self.R, self.bpr.ctypes.data, self.segment_blocks)
        return lib.irec_rec_device_workspace_bytes(n, self.R)

    @property
    def status_text(self):
        """irec_rec_status -> text for a call of this layout."""
        if self.segment_blocks is not None:
            from .segmented import seg_status_text
            return seg_status_text
        return _rec_status_text


def _check_rows(K, idx, layout, who):
    """ValueError for rows (numpy or torch) that are not K [N, T], idx [N, T, max_K] of the layout."""
    if len(K.shape) != 2 or K.shape[1] != layout.T or len(idx.shape) != 3 or tuple(idx.shape[:2]) != tuple(K.shape):
        raise ValueError(f"{who}: K {tuple(K.shape)} and idx {tuple(idx.shape)} are not [N, {layout.T}] and [N, {layout.T}, max_K]")


def _block_rows(K, idx):
    """K [N, R, bpt], idx [N, R, bpt, max_K] as rows [N, R bpt], [N, R bpt, max_K]: views with the block stride kept as the row stride
    where the blocks of an image lie that far apart (a dimension of one included), copies otherwise."""
    n, r, bpt = K.shape
    T, ks, ist = r * bpt, K.stride(2), idx.stride(2)
    K = K.as_strided((n, T), (T * ks, ks)) if K.stride()[:2] == (T * ks, bpt * ks) else K.reshape(n, T)
    if idx.stride()[:2] == (T * ist, bpt * ist):
        return K, idx.as_strided((n, T, idx.shape[3]), (T * ist, ist, idx.stride(3)))
    return K, idx.reshape(n, T, idx.shape[3])


# ---- host ---------------------------------------------------------------------------------------------------------------------------------
def _encode_rows_host(seed, image_shape, block_size, K, idx, max_index, layout, n_threads, tables, who):
    """irec_rec_encode_files[_ragged|_tables|_segmented] over contiguous rows: (blob uint8, offsets int64 [N + 1])."""
    lib = _lib.load()
    seed = header_seed(seed, who)
    n, max_K = K.shape[0], idx.shape[2]
    h, w, c = (int(v) for v in image_shape)
    suffix, blocks = layout.entry(tables)
    encode = getattr(lib, "irec_rec_encode_files" + suffix)
    offsets = np.zeros(n + 1, dtype=np.int64)
    status = np.zeros(max(n, 1), dtype=np.int32)               # (per-image statuses: the entries with tables and of segments only)
    tb = () if tables is None else tables.host_args(layout.R, who)
    newer = suffix in ("_tables", "_segmented")
    last_error = lib.irec_last_error if newer else lib.irec_io_last_error
    if layout.segment_blocks is not None:
        cap = max(layout.first_cap(n, max_K), 1)
    else:
        cap = n * (64 + 16 * layout.R) + 2 * int(K.sum()) + 16 * K.size + 1024

    def call(out):
        total = encode(seed, int(block_size), int(max_index), h, w, c, n, layout.R, *blocks, max_K, K.ctypes.data,
                       idx.ctypes.data if idx.size else None, *tb, out.ctypes.data, out.size, offsets.ctypes.data,
                       *((status.ctypes.data,) if newer else ()), int(n_threads))
        if total < 0:
            raise ValueError(last_error().decode())
        _files.raise_first_status(status[:n], layout.status_text)
        return total
    return _files.encode_host(call, cap), offsets


def _decode_rows_host(blob, offsets, layout, max_K, n_threads):
    """irec_rec_decode_files[_ragged]: (headers [N, 9] uint32, K [N, T], idx [N, T, max_K] with rows zero-filled past K)."""
    lib = _lib.load()
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    n = offsets.size - 1
    hdr = np.zeros((n, 9), dtype=np.uint32)
    K = np.zeros((n, layout.T), dtype=np.int32)
    idx = np.zeros((n, layout.T, max(max_K, 1)), dtype=np.int32)
    suffix, blocks = layout.entry(None)
    st = getattr(lib, "irec_rec_decode_files" + suffix)(blob.ctypes.data, offsets.ctypes.data, n, layout.R, *blocks, int(max_K), hdr.ctypes.data,
                                                        K.ctypes.data, idx.ctypes.data, int(n_threads))
    if st != 0:
        raise ValueError(lib.irec_io_last_error().decode())
    return hdr, K, idx[..., :max_K]


def encode_files(seed, image_shape, block_size, K, idx, max_index, n_threads=0, tables=None):
    """N containers at once from a packed read-back (irec_rec_encode_files): K [N, R, bpt] int32, idx [N, R, bpt, max_K] int32.
    Returns (blob uint8, offsets int64 [N + 1]): file i = blob[offsets[i]:offsets[i + 1]], byte for byte what
    write_compressed_code writes for image i (rec/io/utils.py:7-106, default symbol models).
    tables: a SymbolTables -- the files as write_compressed_code writes them with those count files (irec_rec_encode_files_tables)."""
    K = np.ascontiguousarray(K, dtype=np.int32)
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    n, r, bpt = K.shape
    assert idx.shape[:3] == K.shape
    idx = idx.reshape(n, r * bpt, idx.shape[3]) if idx.ndim == 4 else np.zeros((n, r * bpt, 0), dtype=np.int32)
    if tables is not None:
        return encode_files_ragged(seed, image_shape, block_size, K.reshape(n, r * bpt), idx, max_index, [bpt] * r, n_threads, tables=tables)
    return _encode_rows_host(seed, image_shape, block_size, K.reshape(n, r * bpt), idx, max_index, _Layout(r, bpt), n_threads, None, "encode_files")


def decode_files(blob, offsets, n_res_blocks, blocks_per_res, max_K, n_threads=0, tables=None):
    """The inverse of encode_files (irec_rec_decode_files): (headers [N, 9] uint32 -- seed, block_size, max_index, height,
    width, channels, two flags, R --, K [N, R, bpt], idx [N, R, bpt, max_K] with rows zero-filled past K).
    tables: a SymbolTables for the files whose header flags ask for one (irec_rec_decode_files_tables); files without flags decode
    under the default models in the same call."""
    r, bpt = int(n_res_blocks), int(blocks_per_res)
    if tables is not None:
        hdr, K, idx = decode_files_ragged(blob, offsets, [bpt] * r, max_K, n_threads, tables=tables)
    else:
        hdr, K, idx = _decode_rows_host(blob, offsets, _Layout(r, bpt), max_K, n_threads)
    return hdr, K.reshape(K.shape[0], r, bpt), idx.reshape(K.shape[0], r, bpt, idx.shape[-1])


def encode_files_ragged(seed, image_shape, block_size, K, idx, max_index, blocks_per_res, n_threads=0, tables=None):
    """encode_files for residual blocks of differing sizes (irec_rec_encode_files_ragged): K [N, T] int32, idx [N, T, max_K] int32,
    T = sum(blocks_per_res).  Returns (blob uint8, offsets int64 [N + 1]); file i is byte for byte what write_compressed_code writes for
    image i's lists."""
    layout = _Layout.ragged(blocks_per_res, "encode_files_ragged")
    K = np.ascontiguousarray(K, dtype=np.int32)
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    _check_rows(K, idx, layout, "encode_files_ragged")
    return _encode_rows_host(seed, image_shape, block_size, K, idx, max_index, layout, n_threads, tables, "encode_files_ragged")


def decode_files_ragged(blob, offsets, blocks_per_res, max_K, n_threads=0, tables=None):
    """The inverse of encode_files_ragged (irec_rec_decode_files_ragged): (headers [N, 9] uint32, K [N, T], idx [N, T, max_K] with rows
    zero-filled past K); ValueError naming the first file that is damaged or of another structure."""
    layout = _Layout.ragged(blocks_per_res, "decode_files_ragged")
    if tables is None:
        return _decode_rows_host(blob, offsets, layout, max_K, n_threads)
    hdr, K, idx, status = _decode_rows_host_status(blob, offsets, layout, max_K, tables, n_threads, "decode_files_ragged")
    _raise_first_status(status)
    return hdr, K, idx


def _decode_rows_host_status(blob, offsets, layout, max_K, tables, n_threads, who):
    """irec_rec_decode_files_tables, or _segmented for a segmented layout: (headers [N, 9] uint32, K [N, T], idx [N, T, max_K], status
    int32 [N]) -- a verdict per file (its text: layout.status_text), the outputs of a refused one zero."""
    lib = _lib.load()
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    offsets = _files.host_offsets(offsets, blob.size, who)
    n = offsets.size - 1
    hdr = np.zeros((max(n, 1), 9), dtype=np.uint32)
    K = np.zeros((n, layout.T), dtype=np.int32)
    idx = np.zeros((n, layout.T, int(max_K)), dtype=np.int32)
    status = np.zeros(max(n, 1), dtype=np.int32)
    pad = np.zeros(1, dtype=np.uint8)
    suffix, blocks = layout.entry(tables)
    tb = () if tables is None else tables.host_args(layout.R, who)
    st = getattr(lib, "irec_rec_decode_files" + suffix)(
        blob.ctypes.data if blob.size else pad.ctypes.data, offsets.ctypes.data, n, layout.R, *blocks, int(max_K), *tb, hdr.ctypes.data,
        K.ctypes.data if K.size else pad.ctypes.data, idx.ctypes.data if idx.size else None, status.ctypes.data, int(n_threads))
    if st != 0:
        raise ValueError(lib.irec_last_error().decode())
    return hdr[:n], K, idx, status[:n]


def _decode_files_tables_status(blob, offsets, blocks_per_res, max_K, tables, n_threads=0):
    """_decode_rows_host_status for blocks_per_res under tables (irec_rec_decode_files_tables)."""
    return _decode_rows_host_status(blob, offsets, _Layout.ragged(blocks_per_res, "decode_files_ragged"), max_K, tables, n_threads,
                                    "decode_files_ragged")


# ---- device: CUDA tensors in and out, the launches on the current stream -----------------------------------------------------------------
def _row_strides(K, idx):
    """(K, k_stride, idx, idx_stride) of include/irec.h for K [N, T], idx [N, T, max_K]: row b = i T + t at K[b k_stride],
    idx[b idx_stride + .].  Views of the packed arrays and of one joined [rows][1 + width] tensor pass as they are; anything else is
    made contiguous."""
    n, T = K.shape
    max_K = idx.shape[2]
    row = 1 if T > 1 else 0                            # (T = 1: the next row is the next image, and a dimension of one has no stride to speak of)
    ks = K.stride(row) if K.numel() else 1
    if K.numel() and (ks < 1 or K.stride(0) != T * ks):
        K, ks = K.contiguous(), 1
    ist = idx.stride(row) if idx.numel() else max(max_K, 1)
    if idx.numel() and (ist < max_K or idx.stride(2) != 1 or idx.stride(0) != T * ist):
        idx, ist = idx.contiguous(), max_K
    return K, int(ks), idx, int(ist)


def _block_strides(K, idx):
    """_row_strides for K [N, R, bpt], idx [N, R, bpt, max_K]: block b = (i R + r) bpt + j at K[b k_stride], idx[b idx_stride + t]."""
    K2, ks, idx2, ist = _row_strides(*_block_rows(K, idx))
    return K2.view(K.shape), ks, idx2.view(idx.shape), ist


def _encode_rows_device_launch(seed, image_shape, block_size, K, idx, max_index, layout, out, tables, who):
    """One irec_rec_encode_files_device[_ragged|_tables|_segmented] call on the current stream over rows K [N, T], idx [N, T, max_K], nothing read
    back: (offsets int64 [N + 1], status int32 [N], both views of `both`, which one copy fetches).  The bytes are in `out` only if
    offsets[N] <= out.numel()."""
    import torch
    lib = _lib.load()
    seed = header_seed(seed, who)                      # (before anything is launched: _row_strides may copy)
    n, max_K = K.shape[0], idx.shape[2]
    h, w, c = (int(v) for v in image_shape)
    K, ks, idx, ist = _row_strides(K, idx)
    dev = K.device
    suffix, blocks = layout.entry(tables)
    with torch.cuda.device(dev):
        ws = torch.empty(max(layout.workspace_bytes(lib, n), 8), dtype=torch.uint8, device=dev)
        offsets, status, both = _files.offsets_and_status(n, dev)
        tb = () if tables is None else tables.to(dev).device_args(layout.R, who)
        st = getattr(lib, "irec_rec_encode_files_device" + suffix)(
            seed, int(block_size), int(max_index), h, w, c, n, layout.R, *blocks, max_K, K.data_ptr(), ks,
            idx.data_ptr() if idx.numel() else None, ist, *tb, out.data_ptr() if out.numel() else None, out.numel(), offsets.data_ptr(),
            status.data_ptr() if n else None, ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    _files.check_status(st, "irec_rec_encode_files_device" + suffix)
    return offsets, status, both


def _decode_rows_device_launch(blob, offsets, layout, max_K, on_device, tables, who):
    """One irec_rec_decode_files_device[_ragged|_tables|_segmented] call on the current stream: (headers int32 [N, 9] holding the uint32 words,
    K [N, T], idx [N, T, max_K], status int32 [N]) on the device.  Nothing is read back: host `offsets` are checked against the blob
    before any kernel sees them, and with on_device those that are on the device stay there (_files.device_offsets)."""
    import torch
    lib = _lib.load()
    if not (blob.is_cuda and blob.dtype == torch.uint8):
        raise ValueError(f"{who} takes a CUDA uint8 tensor")
    blob = blob.contiguous()
    dev = blob.device
    max_K = int(max_K)
    offsets = _files.device_offsets(offsets, blob, dev, on_device, who)
    n = offsets.numel() - 1
    suffix, blocks = layout.entry(tables)
    with torch.cuda.device(dev):
        ws = torch.empty(max(layout.workspace_bytes(lib, n), 8), dtype=torch.uint8, device=dev)
        hdr = torch.zeros((n, 9), dtype=torch.int32, device=dev)
        K = torch.empty((n, layout.T), dtype=torch.int32, device=dev)
        idx = torch.empty((n, layout.T, max_K), dtype=torch.int32, device=dev)
        status = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
        tb = () if tables is None else tables.to(dev).device_args(layout.R, who)
        st = getattr(lib, "irec_rec_decode_files_device" + suffix)(
            blob.data_ptr() if blob.numel() else ws.data_ptr(), offsets.data_ptr(), n, layout.R, *blocks, max_K, *tb, hdr.data_ptr(),
            K.data_ptr(), idx.data_ptr() if idx.numel() else None, status.data_ptr(), ws.data_ptr(), ws.numel(),
            torch.cuda.current_stream().cuda_stream)
    _files.check_status(st, "irec_rec_decode_files_device" + suffix)
    return hdr, K, idx, status[:n]


def _encode_files_device_launch(seed, image_shape, block_size, K, idx, max_index, out):
    """_encode_rows_device_launch for K [N, R, bpt], idx [N, R, bpt, max_K] (irec_rec_encode_files_device)."""
    return _encode_rows_device_launch(seed, image_shape, block_size, *_block_rows(K, idx), max_index, _Layout(K.shape[1], K.shape[2]), out, None,
                                      "encode_files_device")


def _encode_files_device_ragged_launch(seed, image_shape, block_size, K, idx, max_index, blocks_per_res, out, tables=None):
    """_encode_rows_device_launch for checked rows (irec_rec_encode_files_device_ragged, or _tables with tables)."""
    import torch
    layout = _Layout.ragged(blocks_per_res, "encode_files_device_ragged")
    if not (K.is_cuda and idx.is_cuda and K.dtype == torch.int32 and idx.dtype == torch.int32):
        raise ValueError("encode_files_device_ragged takes CUDA int32 tensors")
    _check_rows(K, idx, layout, "encode_files_device_ragged")
    return _encode_rows_device_launch(seed, image_shape, block_size, K, idx, max_index, layout, out, tables, "encode_files_device_ragged")


def _decode_files_device_ragged_launch(blob, offsets, blocks_per_res, max_K, on_device=False, tables=None):
    """_decode_rows_device_launch for blocks_per_res (irec_rec_decode_files_device_ragged, or _tables with tables)."""
    layout = _Layout.ragged(blocks_per_res, "decode_files_device_ragged")
    return _decode_rows_device_launch(blob, offsets, layout, max_K, on_device, tables, "decode_files_device_ragged")


def _decode_files_device_launch(blob, offsets, n_res_blocks, blocks_per_res, max_K, on_device=False, tables=None):
    """_decode_rows_device_launch for R residual blocks of bpt blocks (irec_rec_decode_files_device): K [N, R, bpt], idx [N, R, bpt, max_K]."""
    r, bpt = int(n_res_blocks), int(blocks_per_res)
    if tables is not None:                             # (the entry point with tables takes the ragged layout: R equal entries)
        hdr, K, idx, status = _decode_files_device_ragged_launch(blob, offsets, [bpt] * r, max_K, on_device=on_device, tables=tables)
    else:
        hdr, K, idx, status = _decode_rows_device_launch(blob, offsets, _Layout(r, bpt), max_K, on_device, None, "decode_files_device")
    return hdr, K.view(K.shape[0], r, bpt), idx.view(K.shape[0], r, bpt, int(max_K)), status


def _device_out(out, first_cap, dev, who):
    """The buffer a device writer writes into: the caller's, or a first allowance."""
    import torch
    if out is None:
        return torch.empty(max(first_cap(), 1), dtype=torch.uint8, device=dev)
    if not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.device == dev):
        raise ValueError(f"{who}: out must be a contiguous CUDA uint8 tensor on the indices' device")
    return out


def encode_files_device(seed, image_shape, block_size, K, idx, max_index, out=None, tables=None):
    """encode_files on the device (irec_rec_encode_files_device): K [N, R, bpt], idx [N, R, bpt, max_K] int32 CUDA tensors, contiguous
    or views of one joined [rows][1 + width] tensor (PendingCode.gather_packed_device).  Returns (blob uint8, offsets int64 [N + 1]) as
    CUDA tensors, byte for byte what encode_files gives; the only host synchronisation is ONE read-back of offsets and status.
    out: a CUDA uint8 buffer to write into (a short one costs a second run at the size the first one reports)."""
    import torch
    seed = header_seed(seed, "encode_files_device")    # (here as well: _block_rows below may copy on the device)
    if not (K.is_cuda and idx.is_cuda and K.dtype == torch.int32 and idx.dtype == torch.int32):
        raise ValueError("encode_files_device takes CUDA int32 tensors")
    if K.dim() != 3 or idx.dim() != 4 or tuple(idx.shape[:3]) != tuple(K.shape):
        raise ValueError(f"encode_files_device: K {tuple(K.shape)} and idx {tuple(idx.shape)} are not [N, R, bpt] and [N, R, bpt, max_K]")
    n, r, bpt = K.shape
    if tables is not None:                             # (R <= IREC_REC_RAGGED_MAX_RES: the entry point with tables takes the ragged layout)
        return encode_files_device_ragged(seed, image_shape, block_size, *_block_rows(K, idx), max_index, [bpt] * r, out, tables=tables)
    out = _device_out(out, lambda: _Layout(r, bpt).first_cap(n, idx.shape[3]), K.device, "encode_files_device")
    return _files.encode_device(lambda o: _encode_files_device_launch(seed, image_shape, block_size, K, idx, max_index, o), n, out,
                                _rec_status_text, "irec_rec_encode_files_device")


def decode_files_device(blob, offsets, n_res_blocks, blocks_per_res, max_K, tables=None):
    """decode_files on the device (irec_rec_decode_files_device): blob uint8 CUDA tensor, offsets [N + 1] (CUDA, CPU or numpy).
    Returns CUDA tensors (headers [N, 9] int64 -- seed, block_size, max_index, height, width, channels, two flags, R --,
    K [N, R, bpt] int32, idx [N, R, bpt, max_K] int32 with rows zero-filled past K); ValueError naming the first damaged file."""
    import torch
    r, bpt = int(n_res_blocks), int(blocks_per_res)
    if tables is not None:
        hdr, K, idx = decode_files_device_ragged(blob, offsets, [bpt] * r, max_K, tables=tables)
        return hdr, K.view(-1, r, bpt), idx.view(-1, r, bpt, int(max_K))
    hdr, K, idx, status = _decode_files_device_launch(blob, offsets, n_res_blocks, blocks_per_res, max_K)
    _raise_first_status(status.cpu().numpy())
    return hdr.to(torch.int64) & 0xFFFFFFFF, K, idx


def encode_files_device_ragged(seed, image_shape, block_size, K, idx, max_index, blocks_per_res, out=None, tables=None):
    """encode_files_ragged on the device (irec_rec_encode_files_device_ragged): K [N, T], idx [N, T, max_K] int32 CUDA tensors, contiguous
    or views of one joined [rows][1 + width] tensor (PendingCode.gather_packed_ragged_device).  Returns (blob uint8, offsets int64
    [N + 1]) as CUDA tensors, byte for byte what encode_files_ragged gives; the only host synchronisation is ONE read-back of offsets
    and status.  out: a CUDA uint8 buffer to write into (a short one costs a second run at the size the first one reports)."""
    layout = _Layout.ragged(blocks_per_res, "encode_files_device_ragged")
    n, max_K = (K.shape[0], idx.shape[2]) if K.dim() == 2 and idx.dim() == 3 else (0, 0)
    out = _device_out(out, lambda: layout.first_cap(n, max_K), K.device, "encode_files_device_ragged")
    return _files.encode_device(lambda o: _encode_files_device_ragged_launch(seed, image_shape, block_size, K, idx, max_index, layout, o, tables),
                                K.shape[0], out, _rec_status_text, "irec_rec_encode_files_device_ragged")


def decode_files_device_ragged(blob, offsets, blocks_per_res, max_K, tables=None):
    """decode_files_ragged on the device (irec_rec_decode_files_device_ragged): blob uint8 CUDA tensor, offsets [N + 1] (CUDA, CPU or
    numpy).  Returns CUDA tensors (headers [N, 9] int64, K [N, T] int32, idx [N, T, max_K] int32 with rows zero-filled past K);
    ValueError naming the first damaged file."""
    import torch
    hdr, K, idx, status = _decode_files_device_ragged_launch(blob, offsets, blocks_per_res, max_K, tables=tables)
    _raise_first_status(status.cpu().numpy())
    return hdr.to(torch.int64) & 0xFFFFFFFF, K, idx


def rec_header_words(data):
    """The header of one .rec file from its bytes (a pure function: RecHeader over the 28 + 16 R header bytes): a dict of seed,
    image_shape (h, w, c), block_size, max_index, R, bpt (blocks per residual block, a list), max_partitions (a list), or None for
    bytes too short to hold their own header."""
    import io
    data = bytes(memoryview(np.ascontiguousarray(data)) if isinstance(data, np.ndarray) else data)
    if len(data) < _STATIC.size:
        return None
    r = _STATIC.unpack(data[:_STATIC.size])[8]
    if len(data) < _STATIC.size + 16 * r:
        return None
    try:
        h = RecHeader.read(io.BytesIO(data[:_STATIC.size + 16 * r]))
    except (struct.error, ValueError):
        return None
    return {"seed": h.seed, "image_shape": tuple(h.image_shape), "block_size": h.block_size, "max_index": h.max_index, "R": r,
            "bpt": list(h.blocks_per_res_block), "max_partitions": list(h.max_partitions)}


def rec_files_max_K(blob, offsets, tables=None):
    """Index slots per block that decode the files blob[offsets[i]:offsets[i + 1]] (host bytes): the largest max_partitions word of their
    headers, at least 1.  A word above IREC_MAX_PARTITIONS does not count: the reader refuses that file whatever max_K is
    (IREC_REC_E_BLOCK_COUNTS), and a damaged word must not size a buffer.  tables: with count tables the header word is useless
    (0xFFFFFFFF), so the bound is the tables' largest K."""
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    need = 1
    for i in range(len(offsets) - 1):
        words = rec_header_words(blob[int(offsets[i]):int(offsets[i + 1])])
        if words is not None:
            need = max([need] + [m for m in words["max_partitions"] if m <= _lib.MAX_PARTITIONS])
    if tables is not None and tables.max_K is not None:
        need = max(need, tables.max_K)                 # (a file coded under count tables says 0xFFFFFFFF: the bound is the tables')
    return need


def rec_files_max_K_device(blob, offsets, n_res_blocks, tables=None):
    """rec_files_max_K for a blob on the device: only the 28 + 16 R header bytes of every file are gathered and copied to the host."""
    return rec_files_max_K(*_files.gather_heads(blob, offsets, _STATIC.size + 16 * int(n_res_blocks)), tables)


def write_compressed_code(file_path, seed, image_shape, block_size, block_indices, max_index,
                          num_aux_var_counts_file=None, index_counts_file=None):
    """Same signature as rec/io/utils.py:7.  block_indices[r][k] = sample indices of coded block k of residual block r.
    With the default symbol models (no count files) the container is assembled natively in one call; the per-stream Python
    path below is the reference-shaped one (byte-identical, tests/test_rec_io.py) and serves the count-file variants."""
    if len(image_shape) != 3:
        raise ValueError(f"Image shape must be rank 3, but was {image_shape}!")
    seed = header_seed(seed, "write_compressed_code")      # (before the file is opened: a refused seed leaves nothing behind)
    if num_aux_var_counts_file is None and index_counts_file is None and len(block_indices) > 0 and \
            all(len(rb) > 0 for rb in block_indices):
        with open(file_path, "wb") as fh:
            fh.write(_native_encode(seed, image_shape, block_size, block_indices, max_index))
        return
    return _write_compressed_code_py(file_path, seed, image_shape, block_size, block_indices, max_index,
                                     num_aux_var_counts_file, index_counts_file)


def _write_compressed_code_py(file_path, seed, image_shape, block_size, block_indices, max_index,
                              num_aux_var_counts_file=None, index_counts_file=None):
    """The reference-shaped writer: one ArithmeticCoder call per stream (rec/io/utils.py:7-106)."""
    seed = header_seed(seed, "write_compressed_code")
    partition_counts = [[len(ix) for ix in res_block] for res_block in block_indices]
    flat_indices = [np.concatenate([np.asarray(ix, dtype=np.int64).reshape(-1) for ix in res_block])
                    for res_block in block_indices]
    index_model = _uniform_model(max_index, 1000) if index_counts_file is None else np.load(index_counts_file)
    for vec in flat_indices:
        if vec.size and (vec.min() < 0 or vec.max() + 1 >= len(index_model)):
            # the reference overruns its count table silently here (max_index=20 with S=36)
            raise ValueError(f"index {int(vec.max())} does not fit max_index={len(index_model) - 1}")
    if num_aux_var_counts_file is None:
        max_partitions = [int(max(pc)) for pc in partition_counts]
        count_models = [_uniform_model(m + 1, 100) for m in max_partitions]
    else:
        count_models = np.load(num_aux_var_counts_file, allow_pickle=True)
        max_partitions = [-1] * len(block_indices)
    count_streams = [_encode_stream(model, pc) for model, pc in zip(count_models, partition_counts)]
    index_streams = [_encode_stream(index_model, vec) for vec in flat_indices]
    header = RecHeader(seed, block_size, max_index, tuple(int(v) for v in image_shape),
                       num_aux_var_counts_file is not None, index_counts_file is not None,
                       [len(rb) for rb in block_indices], [len(s) for s in count_streams],
                       [len(s) for s in index_streams], max_partitions)
    with open(file_path, "wb") as fh:
        fh.write(header.pack())
        fh.writelines(count_streams)
        fh.writelines(index_streams)


def read_compressed_code(file_path, static_header_size=28, num_aux_var_counts_file=None, index_counts_file=None):
    """Same signature and return value as rec/io/utils.py:109: (seed, image_shape, block_size, block_indices)."""
    if static_header_size == 28 and num_aux_var_counts_file is None and index_counts_file is None:
        with open(file_path, "rb") as fh:
            data = fh.read()
        if len(data) >= 28 and data[22:26] == b"\x00\x00\x00\x00":     # neither count-file flag set: default models
            return _native_decode(data)
    return _read_compressed_code_py(file_path, static_header_size, num_aux_var_counts_file, index_counts_file)


def _read_compressed_code_py(file_path, static_header_size=28, num_aux_var_counts_file=None, index_counts_file=None):
    """The reference-shaped reader (rec/io/utils.py:109-216)."""
    with open(file_path, "rb") as fh:
        hdr = RecHeader.read(fh, static_header_size)
        if hdr.uses_index_file and index_counts_file is None:
            raise ValueError("The compressed file is using empirical index counts, but no counts file was supplied!")
        if hdr.uses_count_file and num_aux_var_counts_file is None:
            raise ValueError("The compressed file is using empirical num_aux_var counts, but no counts file was supplied!")
        count_streams = [fh.read(n) for n in hdr.count_stream_bytes]
        index_streams = [fh.read(n) for n in hdr.index_stream_bytes]
    index_model = np.load(index_counts_file) if hdr.uses_index_file else _uniform_model(hdr.max_index, 1000)
    count_models = (np.load(num_aux_var_counts_file, allow_pickle=True) if hdr.uses_count_file
                    else [_uniform_model(m + 1, 100) for m in hdr.max_partitions])
    block_indices = []
    for model, cs, xs in zip(count_models, count_streams, index_streams):
        counts = _decode_stream(model, cs)
        values = _decode_stream(index_model, xs)
        cuts = np.concatenate([[0], np.cumsum(counts)])
        block_indices.append([values[cuts[i]:cuts[i + 1]].tolist() for i in range(len(counts))])
    return hdr.seed, hdr.image_shape, hdr.block_size, block_indices
