"""What the models' decompress_rec forms share: a batch of .rec files (plain, under symbol tables or segmented; read on host threads or
on the device) to rows on the device, the joined per-image status and its texts, and the strict tail.  The models keep what is theirs:
their layouts, their generative pass over the rows, and BidirectionalResNetVAE.status_text with the ratio-table message."""
import numpy as np
import torch

from .. import _lib
from ..coding.utils import CodingError

# the joined per-image status of decompress_rec / decompress_packed beside irec_rec_status (1 .. 18)
STATUS_HEADER = 19      # the file's seed, height, width, channels or R differ from the call's
STATUS_TABLE = 20       # IREC_REC_E_TABLE (19 on the wire, which STATUS_HEADER has here): a symbol table that cannot be coded under
STATUS_SEGMENTED = 21   # + (irec_rec_status - 20): IREC_REC_E_SEG_MAGIC, _SEG_DIRECTORY, _SEG_BLOCKS (20 .. 22 on the wire) as 21 .. 23
STATUS_ROWS = 32        # + irec_rows_status (1 K_RANGE, 2 INDEX_RANGE, 3 RATIO_TABLE)
STATUS_RESIDUAL = 48    # + irec_res_status (decompress_lossless: the .res file of an image whose .rec file decoded)


def status_text(status, table_length=None, requested=None):
    """The coder's text for a joined status.  A count beyond the fitted ratio table gets the reference's message when the table's
    length and the count that was asked for are known."""
    from ..coding.coder import RATIO_TABLE_TEXT
    from ..io.residual import res_status_text
    from ..io.utils import _REC_STATUS_TEXT
    status = int(status)
    if status > STATUS_RESIDUAL:
        return res_status_text(status - STATUS_RESIDUAL)
    if status == STATUS_ROWS + _lib.IREC_ROWS_E_RATIO_TABLE:
        if table_length is not None and requested is not None:
            return RATIO_TABLE_TEXT.format(table_length, requested)
        return RATIO_TABLE_TEXT.split(".")[0] + "."
    if STATUS_SEGMENTED <= status <= STATUS_SEGMENTED + 2:
        from ..io.segmented import seg_status_text
        return seg_status_text(status - STATUS_SEGMENTED + _lib.IREC_REC_E_SEG_MAGIC)
    own = {STATUS_HEADER: "decompress_rec: the file's header (seed, image shape, residual blocks) differs from the arguments",
           STATUS_TABLE: _REC_STATUS_TEXT[_lib.IREC_REC_E_TABLE],
           STATUS_ROWS + _lib.IREC_ROWS_E_K_RANGE: "partition count out of range [min_K, max_K]",
           STATUS_ROWS + _lib.IREC_ROWS_E_INDEX_RANGE: "index out of range [0, n_samples)"}
    return own.get(status) or _REC_STATUS_TEXT.get(status, f"irec_rec: status {status}")


# ---- device constants of the packed decompress path, per batch shape (cached: the device pass must not touch the host, so that
#      GraphedDecompress can capture it).  Two caches, so that many seeds -- a header_want each -- do not turn the row maps out ------------
_ROWS_CACHE, _WANT_CACHE = {}, {}


def _cached(cache, key, make):
    if key not in cache:
        if len(cache) > 16:
            cache.clear()
        cache[key] = make()
    return cache[key]


def packed_rows(n, blocks_per_res, device):
    """Per residual block r the int32 device map (image i, block j) -> row i T + first[r] + j of packed K [N, T] arrays (for R residual
    blocks of bpt blocks that is (i R + r) bpt + j, the row of K [N, R, bpt])."""
    bpr = tuple(int(b) for b in blocks_per_res)

    def make():
        T, first = sum(bpr), np.concatenate([[0], np.cumsum(bpr)])
        i = torch.arange(n, dtype=torch.int32).reshape(n, 1)
        return [(i * T + int(first[r]) + torch.arange(b, dtype=torch.int32).reshape(1, b)).reshape(-1).contiguous().to(device) for r, b in enumerate(bpr)]
    return _cached(_ROWS_CACHE, (n, bpr, str(device)), make)


def header_want(seed, image_shape, n_res_blocks, device):
    """The header words (seed, height, width, channels, R) a file of this call must carry, int64 on the device.  A seed that no header
    holds (outside [0, 2^32)) is wanted as -1, which no file carries: every file then has STATUS_HEADER, instead of the files whose
    seed equals the call's low 32 bits being decoded under another seed."""
    _, c, h, w = (int(v) for v in image_shape)
    seed = int(seed)
    words = [seed if 0 <= seed <= 0xFFFFFFFF else -1, h, w, c, int(n_res_blocks)]
    return _cached(_WANT_CACHE, (*words, str(device)), lambda: torch.tensor(words, dtype=torch.int64).to(device))


# ---- files to rows -------------------------------------------------------------------------------------------------------------------------
def _decode_files_host(blob, offsets, bpr, max_K, tables=None):
    """irec.io.decode_files_ragged with a verdict per file: (headers, K, idx, status int32 [N]).  The host reader stops at the first
    file it refuses; only then is every file read alone, a refused one leaving zero rows and the irec_rec_status of the reader's
    words for it (the first of a class that shares its text)."""
    from ..io.utils import _REC_STATUS_TEXT, _decode_files_tables_status, decode_files_ragged
    n = len(offsets) - 1
    if tables is not None:                          # (the reader with tables gives a verdict per file itself)
        return _decode_files_tables_status(blob, offsets, bpr, max_K, tables)
    try:
        hdr, K, idx = decode_files_ragged(blob, offsets, bpr, max_K)
        return hdr, K, idx, np.zeros(n, dtype=np.int32)
    except ValueError:
        pass
    hdr, K, idx = np.zeros((n, 9), np.uint32), np.zeros((n, sum(bpr)), np.int32), np.zeros((n, sum(bpr), max_K), np.int32)
    status = np.zeros(n, dtype=np.int32)
    for i in range(n):
        one = blob[int(offsets[i]):int(offsets[i + 1])]
        try:
            hdr[i], K[i], idx[i] = (a[0] for a in decode_files_ragged(one if one.size else np.zeros(1, np.uint8), np.array([0, one.size]), bpr,
                                                                     max_K, n_threads=1))
        except ValueError as e:
            text = str(e).rsplit(" (image", 1)[0]
            status[i] = next((code for code, t in sorted(_REC_STATUS_TEXT.items()) if t == text and code >= 4), 16)
    return hdr, K, idx, status


def read_rows(blob, offsets, layout, max_K, *, rec_on_device, tables=None, segment_blocks=None, device=None):
    """The rows of N .rec files (file i = blob[offsets[i]:offsets[i + 1]]) on `device`: (header words int64 [N, 9], K [N, T] int32,
    idx [N, T, max_K] int32, rec_status int32 [N]), all on the device.  layout: the blocks per residual block (a list, or irec.io's
    layout of R residual blocks of one size: the reader without tables takes that as one count).  tables: the irec.io.SymbolTables the
    files were written under; segment_blocks: g for the segmented container (NAME.recs), None for the reference's.
    rec_on_device: blob is a CUDA tensor and the rows never leave the device -- irec.io's launch forms of the device readers, no host
    synchronisation when max_K is given; otherwise the files are read on host threads and the rows uploaded once.  max_K None: the
    largest word of the files' headers or directories (with count tables, their largest K); on the device that is a second, small
    read-back of those bytes alone.
    rec_status is irec_rec_status with IREC_REC_E_TABLE moved to STATUS_TABLE and the segmented reader's own causes to
    STATUS_SEGMENTED + 0 .. 2."""
    from ..io import segmented as SG
    from ..io import utils as U
    if segment_blocks is not None:
        layout = U._Layout.segmented(layout, segment_blocks, "decode_files_device_segmented" if rec_on_device else "decode_files_segmented")
    else:
        layout = U._Layout.ragged(layout, "decode_files_device_ragged" if rec_on_device else "decode_files_ragged")
    if rec_on_device:
        if max_K is None:
            max_K = SG.segmented_files_max_K_device(blob, offsets, layout, segment_blocks) if segment_blocks is not None else \
                U.rec_files_max_K_device(blob, offsets, layout.R, tables)
        who = "decode_files_device" + ("_segmented" if segment_blocks is not None else "" if layout.bpt is not None else "_ragged")
        hdr, K, idx, status = U._decode_rows_device_launch(blob, offsets, layout, int(max_K), True, tables, who)
        words = hdr.to(torch.int64).bitwise_and_(0xFFFFFFFF)
    else:
        blob_h = np.ascontiguousarray(blob.cpu().numpy() if hasattr(blob, "cpu") else blob, dtype=np.uint8)
        off_h = np.ascontiguousarray(offsets.cpu().numpy() if hasattr(offsets, "cpu") else offsets, dtype=np.int64)
        if max_K is None:
            max_K = SG.segmented_files_max_K(blob_h, off_h) if segment_blocks is not None else U.rec_files_max_K(blob_h, off_h, tables)
        if segment_blocks is not None:
            hdr, K, idx, status = U._decode_rows_host_status(blob_h, off_h, layout, int(max_K), None, 0, "decode_files_segmented")
        else:
            hdr, K, idx, status = _decode_files_host(blob_h, off_h, [int(b) for b in layout.bpr], int(max_K), tables)
        both = torch.from_numpy(np.concatenate([K[..., None], idx], axis=2)).to(device)           # one upload for the rows
        K, idx = both[..., 0], both[..., 1:]
        words, status = torch.from_numpy(hdr.astype(np.int64)).to(device), torch.from_numpy(status).to(device)
    if tables is not None:
        status = torch.where(status == _lib.IREC_REC_E_TABLE, torch.full_like(status, STATUS_TABLE), status)
    if segment_blocks is not None:
        status = torch.where(status >= _lib.IREC_REC_E_SEG_MAGIC, status + (STATUS_SEGMENTED - _lib.IREC_REC_E_SEG_MAGIC), status)
    return words, K, idx, status


# ---- the joined status and the tail of every decompress call -----------------------------------------------------------------------------
def join_status(rec_status, words, want, rows_status):
    """The joined status on the device, first cause first: the reader's verdict on the file; STATUS_HEADER where its words (seed, height,
    width, channels, R of header_want) differ from the call's; STATUS_ROWS + the coders' verdict on the rows."""
    differs = (torch.cat([words[:, 0:1], words[:, 3:6], words[:, 8:9]], dim=1) != want).any(dim=1)
    return torch.where(rec_status != 0, rec_status,
                       torch.where(differs, torch.full_like(rec_status, STATUS_HEADER),
                                   torch.where(rows_status != 0, rows_status + STATUS_ROWS, rows_status)))


def raise_status(status, text_of=lambda i, status: status_text(status)):
    """CodingError for the first image with a nonzero joined status: text_of(i, status[i]), "(image i)" appended."""
    bad = np.flatnonzero(status)
    if bad.size:
        i = int(bad[0])
        raise CodingError(f"{text_of(i, int(status[i]))} (image {i})")


def finish(result, host_status, strict, raise_fn=raise_status):
    """strict: raise_fn(host_status) raises for the first refused image, else `result`; strict=False: (result, host_status)."""
    if strict:
        raise_fn(host_status)
        return result
    return result, host_status
