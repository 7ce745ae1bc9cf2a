"""Per-image compression driver: the loop of the reference's lossless evaluation script
(examples/lossless/compression_performance.py:305-430) around `model.compress` -- compress, write the `.rec` file
(:350-365), read it back and compare the indices (:369-375), bits / bits-per-pixel / bits-per-dimension of the code per
image (:367,380-384) -- with two changes the MI355X path is built around:

  * images are independent, so a rank compresses its images in BATCHES through `BidirectionalResNetVAE.compress`
    (one coder launch per residual block for the whole batch, one device-to-host copy per batch);
  * image i belongs to rank i mod G (irec/sharding.py); the per-image bits are gathered once at the end with the path's
    only collective (RCCL over xGMI on the GPU box, gloo in the CPU tests).

No dataset or checkpoint exists in the reference tree: the caller supplies images and a model.  By default
"bpd" is the CODE's share, file bits / (pixels * channels).  lossless=True adds the residual as real bytes -- NAME.res beside
NAME.rec, the pixels arithmetic-coded under the model's discretized-logistic likelihood given the reconstruction
(model.compress_lossless) -- and with it the reference's code + residual figures (:381-384) and the image itself, exactly.
"""
import os
import time

import numpy as np
import torch

from . import sharding
from .coding import CodingError
from .io import decode_files, decode_files_device, encode_files, header_seed, read_compressed_code, rec_header_words, write_compressed_code
from .models.resnet_vae import STATUS_RESIDUAL, status_text


# ---- what every leg of the drivers does: files written and read back, rows compared, one result row per image ----------------------------
def _joined(datas):
    """N files' bytes as (blob uint8, offsets int64 [N + 1])."""
    sizes = np.array([len(d) for d in datas], dtype=np.int64)
    return np.frombuffer(b"".join(datas), dtype=np.uint8), np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def _upload(host, dev):
    return torch.from_numpy(host.copy()).to(dev)              # (a copy: bytes objects are read-only)


def _write_and_read_back(out_dir, names, ext, blob, offsets):
    """File i = blob[offsets[i]:offsets[i + 1]] (numpy, or device tensors: one copy each) written as NAME.ext and all of them read back:
    (back_blob uint8 numpy, off2 int64 [N + 1], sizes int64 [N])."""
    host, off = (blob.cpu().numpy(), offsets.cpu().numpy()) if hasattr(blob, "cpu") else (blob, offsets)
    paths = [os.path.join(out_dir, f"{nm}.{ext}") for nm in names]
    mv = memoryview(host)
    for i, path in enumerate(paths):
        with open(path, "wb") as fh:
            fh.write(mv[off[i]:off[i + 1]])
    datas = []
    for path in paths:
        with open(path, "rb") as fh:
            datas.append(fh.read())
    back, off2 = _joined(datas)
    return back, off2, np.diff(off2)


def _rows_match(hdr, K2, idx2, K, idx, want_words):
    """bool [N]: the files of a batch decoded to what they were built from -- K2 [N, T] equals K, idx2 [N, T, max_K] equals idx in the
    K live slots of every row (what lies past them does not count) and the header words seed, block_size, height, width, channels
    equal want_words.  numpy arrays give a numpy array, torch tensors a tensor on their device (nothing is read back here)."""
    if isinstance(K, np.ndarray):
        slots, want = np.arange(idx.shape[2]), np.asarray(want_words, dtype=np.int64)
    else:
        slots, want = torch.arange(idx.shape[2], device=idx.device), torch.tensor(want_words, dtype=torch.int64, device=hdr.device)
    live = slots[None, None, :] < K[..., None]
    return (K2 == K).all(1) & ((idx2 == idx) | ~live).all(2).all(1) & (hdr[:, [0, 1, 3, 4, 5]] == want).all(1)


def _rec_row(name, size_bytes, h, w, n_idx, S, recovered, comp_time):
    """The result row of one image (reference CSV columns where they apply) from its file's size and its index count."""
    bits = int(size_bytes) * 8
    return {"name": name, "comp_codelength": bits, "comp_lossy_bpp": bits / (h * w), "comp_code_bpd": bits / (h * w * 3),
            "code_nats": int(n_idx) * float(np.log(S)), "n_indices": int(n_idx), "indices_recovered": bool(recovered), "comp_time": comp_time}


def _in_batches(n, batch, names, fn):
    """[fn(lo, hi) for the batches of n images in order]; a batch the coder refuses (CodingError) is the error rows of its images
    instead (compression_performance.py:375-377: log and move on).  What fn returns is the caller's: rows, or a future of rows."""
    out = []
    for lo in range(0, n, batch):
        hi = min(lo + batch, n)
        try:
            out.append(fn(lo, hi))
        except CodingError as e:
            out.append([{"name": names[i], "error": str(e)} for i in range(lo, hi)])
    return out


def _check_leg(out_dir, names, ext, blob, offsets, K, idx, decode, want_words, S, t_compress, t1):
    """The file half of a batch (compression_performance.py:350-375 per image): the files blob / offsets written, read back, decoded
    together by decode(back_blob, off2) -> (headers, K2, idx2) and compared with the rows K [N, T], idx [N, T, max_K] they were built
    from (or both as [N, R, bpt], [N, R, bpt, max_K]) -- numpy rows on the host, device rows on the device (the bytes uploaded once,
    the verdicts and the index counts read back once each).  t1: when this half began.  One _rec_row per image."""
    n, (_, _, h, w, _) = len(names), want_words
    back, off2, sizes = _write_and_read_back(out_dir, names, ext, blob, offsets)
    on_device = not isinstance(K, np.ndarray)
    hdr, K2, idx2 = decode(_upload(back, K.device) if on_device else back, off2)
    same, n_idx = _rows_match(hdr, *_as_rows(K2, idx2), *_as_rows(K, idx), want_words), K.reshape(n, -1).sum(1)
    if on_device:
        same, n_idx = same.cpu().numpy(), n_idx.cpu().numpy()
    t_host = (time.perf_counter() - t1) / n
    return [_rec_row(names[i], sizes[i], h, w, n_idx[i], S, same[i], t_compress / n + t_host) for i in range(n)]


def _as_rows(K, idx):
    """K [N, R, bpt], idx [N, R, bpt, max_K] as the rows [N, R bpt], [N, R bpt, max_K] they are (rows stay as they are)."""
    K = K.reshape(K.shape[0], -1)
    return K, idx.reshape(*K.shape, idx.shape[-1])


def _host_leg(chunk_shape, names, seed, block_size, out_dir, S, K, idx, t_compress, tables=None):
    """_check_leg for one batch's packed read-back: the containers are built natively for all images at once (irec_rec_encode_files,
    host threads), and decoded together (irec_rec_decode_files)."""
    _, _, h, w = chunk_shape
    t1 = time.perf_counter()
    blob, off = encode_files(seed, (h, w, 3), block_size, K, idx, max_index=S, tables=tables)   # the reference passes 20 < S = 36
    decode = lambda b, o: decode_files(b, o, K.shape[1], K.shape[2], idx.shape[3], tables=tables)  # noqa: E731
    return _check_leg(out_dir, names, "rec", blob, off, K, idx, decode, (seed, block_size, h, w, 3), S, t_compress, t1)


def _device_leg(model, chunk, names, seed, block_size, out_dir, S, tables=None):
    """_host_leg with the files built and checked on the device: the batch's files come from model.compress_rec (the arithmetic coder
    runs on the device), are written, read back, decoded on the device (irec_rec_decode_files_device) and compared there with the
    indices that compress_rec's coders left.  The rows carry the same keys."""
    _, _, h, w = chunk.shape
    t0 = time.perf_counter()
    (blob, off, _), (K, idx) = model.compress_rec(chunk, seed=seed, update_sampler=False, block_size=block_size, return_pendings=True,
                                                  tables=tables)   # K, idx: views of the joined device tensor the files were built from
    t_compress, t1 = time.perf_counter() - t0, time.perf_counter()
    decode = lambda b, o: decode_files_device(b, o, K.shape[1], K.shape[2], idx.shape[3], tables=tables)  # noqa: E731
    return _check_leg(out_dir, names, "rec", blob, off, K, idx, decode, (seed, block_size, h, w, 3), S, t_compress, t1)


def _lists_leg(model, chunk, names, seed, block_size, out_dir, S):
    """The per-image form: model.compress's nested lists through the reference's write_compressed_code / read_compressed_code."""
    n, _, h, w = chunk.shape
    t0 = time.perf_counter()
    block_indices, _ = model.compress(chunk, seed=seed, update_sampler=False)
    t_compress = time.perf_counter() - t0
    rows = []
    for name, bi in zip(names, [block_indices] if n == 1 else block_indices):
        t1 = time.perf_counter()
        path = os.path.join(out_dir, f"{name}.rec")
        write_compressed_code(file_path=path, seed=seed, image_shape=(h, w, 3), block_size=block_size,
                              block_indices=bi, max_index=S)       # the reference passes 20 < S = 36
        size = os.path.getsize(path)
        s, shape, bs, bi_ = read_compressed_code(file_path=path)
        ok = (s, tuple(shape), bs) == (seed, (h, w, 3), block_size) and bi_ == bi
        rows.append(_rec_row(name, size, h, w, sum(len(ix) for blk in bi for ix in blk), S, ok, t_compress / n + (time.perf_counter() - t1)))
    return rows


def _lossless_leg(model, chunk, names, seed, block_size, out_dir, S, stream_len):
    """_device_leg for uint8 images with the residual: model.compress_lossless, NAME.rec and NAME.res written, both read back and
    decoded on the device (model.decompress_lossless, one read-back), the pixels compared there.  The rows carry _device_leg's keys
    (the code's share) and comp_residual (the .res file's bits), comp_lossless_bpp and comp_bpd ((rec + res bits) per pixel and per
    dimension: compression_performance.py:381-384 with bits that were written), residual_model_bits (the ideal bits of the integer
    model), pixels_recovered."""
    from .io.residual import residual_model_bits
    n, _, h, w = chunk.shape
    t0 = time.perf_counter()
    (blob, off, res_blob, res_off, rec), (K, _) = model.compress_lossless(chunk, seed=seed, stream_len=stream_len, block_size=block_size,
                                                                           return_pendings=True)
    t_compress, t1 = time.perf_counter() - t0, time.perf_counter()
    back, off2, sizes = _write_and_read_back(out_dir, names, "rec", blob, off)
    res_back, res_off2, res_sizes = _write_and_read_back(out_dir, names, "res", res_blob, res_off)
    pixels, status = model.decompress_lossless(_upload(back, chunk.device), off2, _upload(res_back, chunk.device), res_off2, seed, tuple(chunk.shape),
                                               max_K=max(int(K.max()), 1), strict=False, stream_len=stream_len)
    same = ((pixels == chunk).reshape(n, -1).all(dim=1)).cpu().numpy() & (status == 0)
    ideal = residual_model_bits(chunk, rec, model.residual_scale())
    n_idx = K.sum(dim=(1, 2)).cpu().numpy()
    t_host = (time.perf_counter() - t1) / n
    rows = []
    for i in range(n):
        total = (int(sizes[i]) + int(res_sizes[i])) * 8
        rows.append(_rec_row(names[i], sizes[i], h, w, n_idx[i], S, status[i] == 0 or status[i] > STATUS_RESIDUAL, t_compress / n + t_host))
        rows[-1].update({"comp_residual": int(res_sizes[i]) * 8, "comp_lossless_bpp": total / (h * w), "comp_bpd": total / (h * w * 3),
                         "residual_model_bits": float(ideal[i]), "pixels_recovered": bool(same[i])})
    return rows


class _IdealRows:
    """The rows of a batch (a list, or the future of the packed host leg) that gain the ideal columns when they are asked for: the
    columns were launched after the batch's compression pass and are read back here, with the batch's one extra copy."""

    def __init__(self, job, columns, h, w):
        self.job, self.columns, self.h, self.w = job, columns, h, w

    def result(self):
        rows = self.job if isinstance(self.job, list) else self.job.result()
        residual, kl, comp_kl = self.columns.cpu().numpy()            # the one extra read-back
        for i, row in enumerate(rows):
            if "error" not in row:
                row.update(_ideal_row(float(residual[i]), float(kl[i]), float(comp_kl[i]), row["comp_codelength"], self.h, self.w))
        return rows


def _ideal_row(residual, kl, comp_kl, comp_codelength, h, w):
    """The reference's ideal columns (compression_performance.py:337-342) from an image's residual = -log_likelihood and kl, in nats,
    and the coded pass's comp_kl with what the code spends above it."""
    ln2 = float(np.log(2.0))
    return {"residual": residual, "kl": kl, "lossless_bpp": (kl + residual) / (h * w * ln2), "lossy_bpp": kl / (h * w * ln2),
            "bpd": (kl + residual) / (h * w * 3 * ln2), "comp_kl": comp_kl, "overhead_bits": comp_codelength - comp_kl / ln2}


def _ideal_columns(model, chunk, seed, image_base):
    """float64 [3, m] on the device: residual, kl of a seeded sampling pass over the chunk (model.forward: image i draws as image number
    image_base + i) and, before it, the KL of the distributions the compression pass just coded under.  No synchronisation."""
    comp_kl = model.coded_kl()
    x = chunk.to(torch.float32).mul(1.0 / 256.0).sub(0.5) if chunk.dtype == torch.uint8 else chunk
    model.forward(x, seed=seed, image_base=image_base)
    return torch.stack([-model.log_likelihood, model.kl_divergence(), comp_kl])


def compress_images(model, images, names, seed, block_size, out_dir, batch=None, packed=True, rec_on_device=False, lossless=False,
                    stream_len=None, tables=None, ideal=False):
    """images: [n, 3, H, W] in [-0.5, 0.5] on the model's device.  Returns one dict per image (reference CSV columns where
    they apply: comp_codelength, comp_lossy_bpp, comp_time) plus `indices_recovered`, `code_nats`.
    packed (default): the indices stay packed arrays from the device to the files (model.compress_packed, irec.io.encode_files
    / decode_files), and the host leg of a batch runs on a worker thread while the device codes the next batch; packed=False is
    the per-image form with the reference's write_compressed_code / read_compressed_code on nested lists.
    rec_on_device: a batch's files are built on the device (model.compress_rec) and the read-back check runs there
    (irec.io.decode_files_device); same rows, byte-identical files.  The default stays the host leg.
    lossless: images are uint8 [n, 3, H, W] (the model sees x / 256 - 0.5); NAME.res is written beside NAME.rec, both are read back
    and decoded to the pixels on the device, and the rows gain comp_residual, comp_lossless_bpp, comp_bpd, residual_model_bits and
    pixels_recovered (_lossless_leg).  stream_len: symbols per .res stream (default irec.io.residual.DEFAULT_STREAM_LEN).
    tables: an irec.io.SymbolTables (fit_symbol_tables) the files are coded under, on the packed host leg or the device leg;
    decompress_images_tables reads them.  The per-image form and the lossless pair keep the default models (ValueError).
    ideal: every row also carries the ideal half of the reference's results row (compression_performance.py:321-342), from a seeded
    sampling forward pass over the batch after its compression pass (model.forward(chunk, seed, image_base): the library's own
    seeded draws, irec.ideal) -- `residual` = -log_likelihood and `kl` in nats, `lossless_bpp` = (kl + residual) / (h w ln 2),
    `lossy_bpp` = kl / (h w ln 2), `bpd` = lossless_bpp / 3 -- and `comp_kl`, the KL of the distributions the indices were coded
    under (through the same kernel), with `overhead_bits` = comp_codelength - comp_kl / ln 2: what the files spend above the KL they
    code.  All of it stays on the device until ONE extra read-back per batch.  image_base is the image's number in the call, not in
    the batch, so a row's draws do not depend on batch=.  ideal=False: the rows and the work are as before."""
    if tables is not None and (lossless or not (rec_on_device or (packed and hasattr(model, "compress_packed")))):
        raise ValueError("compress_images: tables go with the packed host leg or rec_on_device, not with lossless or packed=False")
    seed = header_seed(seed, "compress_images")            # (before out_dir is made or a batch coded: no leg could write this seed)
    os.makedirs(out_dir, exist_ok=True)
    n = images.shape[0]
    batch = n if not batch else int(batch)
    S = model.residual_blocks[0].coder.n_samples
    if ideal:
        h, w = int(images.shape[2]), int(images.shape[3])

        def with_ideal(leg):            # the leg's rows (or their future), then the ideal pass launched behind the compression pass
            def run(lo, hi):
                job = leg(lo, hi)
                return _IdealRows(job, _ideal_columns(model, images[lo:hi], seed, lo), h, w)
            return run
    else:
        with_ideal = lambda leg: leg  # noqa: E731
    if lossless:
        leg = lambda lo, hi: _lossless_leg(model, images[lo:hi], names[lo:hi], seed, block_size, out_dir, S, stream_len)  # noqa: E731
    elif rec_on_device:
        leg = lambda lo, hi: _device_leg(model, images[lo:hi], names[lo:hi], seed, block_size, out_dir, S, tables)  # noqa: E731
    elif packed and hasattr(model, "compress_packed"):
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=1) as pool:         # the host leg of a batch runs while the device codes the next one

            def leg(lo, hi):
                t0 = time.perf_counter()
                K, idx, _ = model.compress_packed(images[lo:hi], seed=seed, update_sampler=False)
                return pool.submit(_host_leg, tuple(images[lo:hi].shape), names[lo:hi], seed, block_size, out_dir, S, K, idx,
                                   time.perf_counter() - t0, tables)
            return [row for job in _in_batches(n, batch, names, with_ideal(leg)) for row in (job if isinstance(job, list) else job.result())]
    else:
        leg = lambda lo, hi: _lists_leg(model, images[lo:hi], names[lo:hi], seed, block_size, out_dir, S)  # noqa: E731
    return [row for rows in _in_batches(n, batch, names, with_ideal(leg)) for row in (rows if isinstance(rows, list) else rows.result())]


def _segmented_words(data):
    """rec_header_words' dict for a segmented file's bytes, or None for bytes too short to hold the fixed part and the block counts."""
    from .io import segmented_header_words
    from .io.segmented import FIXED_BYTES
    w = segmented_header_words(data)
    if w is None or w["bpt"] is None:
        return None
    g, at = w["segment_blocks"], FIXED_BYTES + 4 * w["R"]
    n_seg = min(sum(-(-b // g) for b in w["bpt"]) if g else 0, (len(data) - at) // 12)
    w["max_partitions"] = np.frombuffer(data[at:at + 12 * n_seg], dtype="<u4")[::3].tolist() if n_seg > 0 else []
    return w


def rec_file_groups(datas):
    """The header grouping of decompress_images, a pure function over the files' bytes: (infos, groups).  infos[i]: the header words of
    file i (irec.io.rec_header_words: seed, image_shape, block_size, max_index, R, bpt, max_partitions), None for bytes too short to
    hold their header.  groups: {(seed, image_shape, R, bpt): [file indices, in the order given]} -- the files one decompress_rec call
    takes together; bpt is the one block count of every residual block, or the tuple of counts of a ragged file (which the device
    reader does not take).
    A file that begins with the segmented container's magic (NAME.recs) has the words of
    irec.io.segmented_header_words -- `segment_blocks` among them, max_partitions the max_part words of its directory -- and its bpt
    in the key is ("segmented", segment_blocks, *counts): the two containers never share a group, and a driver that reads plain files
    only sees a block structure it does not take."""
    from .io import is_segmented
    infos, groups = [], {}
    for i, data in enumerate(datas):
        w = _segmented_words(data) if is_segmented(data) else rec_header_words(data)
        infos.append(w)
        if w is None:
            continue
        if "segment_blocks" in w:
            bpt = ("segmented", w["segment_blocks"], *w["bpt"])
        else:
            bpt = w["bpt"][0] if len(set(w["bpt"])) == 1 else tuple(w["bpt"])
        groups.setdefault((w["seed"], w["image_shape"], w["R"], bpt), []).append(i)
    return infos, groups


def _read(path, missing=None):
    if missing is not None and not os.path.exists(path):
        return missing
    with open(path, "rb") as fh:
        return fh.read()


def _decompress_groups(model, paths, batch, strict, fits, decode, tables=None, res=False):
    """The read side of compress_images: .rec files -> (images, rows).  The files are read and their headers parsed on the host
    (RecHeader over the 28 + 16 R header bytes), files of equal (seed, shape, R, bpt) are grouped, each group's bytes are uploaded
    once per batch and decoded by model.decompress_rec -- the arithmetic decoder, the row checks and the generative pass on the
    device, one read-back (the per-image status) per batch.
    images: [n, 3, H, W] in the order of `paths` -- a list of [3, H, W] tensors when the files hold more than one shape or a file is
    too short for its header (its entry is None: its shape is not known); rows: one dict per file (name, status, and where the
    header could be read seed, image_shape, block_size, decomp_time; `error` with the coder's text where status != 0).
    strict: CodingError for the first file, in the order of `paths`, that cannot be decoded; strict=False reports it in its row and
    leaves its image zero.
    What is the model's: fits(info, key) -- whether the model decodes the group `key` of rec_file_groups, info being the header words
    of its first file -- and decode(part, info, blob, off, seed, shape, max_K) -> (images [n, 3, H, W], status [n], the texts of the
    nonzero ones) for the files `part` (indices into paths) of such a group: blob / off their bytes on the host, max_K their headers'
    largest word or the largest K of `tables` (a file under count tables says 0xFFFFFFFF).
    res: the images are uint8 pixels (decompress_images_lossless): the dtype of a refused group's zeros."""
    dev = next(model.parameters()).device
    datas = [_read(path) for path in paths]
    infos, groups = rec_file_groups(datas)
    images, rows = [None] * len(paths), [None] * len(paths)
    for i, w in enumerate(infos):
        if w is None:
            rows[i] = {"name": os.path.basename(paths[i]), "status": 4, "error": status_text(4)}     # IREC_REC_E_TRUNCATED_HEADER
    for key, members in groups.items():
        seed, (h, w_, c), R, bpt = key
        ok = fits(infos[members[0]], key)
        step = len(members) if not batch else int(batch)
        for lo in range(0, len(members), step):
            part = members[lo:lo + step]
            t0 = time.perf_counter()
            if ok:
                blob, off = _joined([datas[i] for i in part])
                max_K = max([1] + [m for i in part for m in infos[i]["max_partitions"] if m <= 65536])
                if tables is not None and tables.max_K is not None:
                    max_K = max(max_K, tables.max_K)
                rec, status, texts = decode(part, infos[members[0]], blob, off, seed, (len(part), c, h, w_), max_K)
            else:                                                       # IREC_REC_E_STRUCTURE: not this model's block structure
                rec, status = torch.zeros((len(part), 3, h, w_), device=dev, dtype=torch.uint8 if res else None), [17] * len(part)
                texts = [f"{status_text(17)}: {R} residual blocks of {bpt} blocks for a {h} x {w_} x {c} image do not match the model"] * len(part)
            dt = (time.perf_counter() - t0) / len(part)
            for k, i in enumerate(part):
                images[i] = rec[k] if status[k] == 0 else torch.zeros_like(rec[k])
                rows[i] = {"name": os.path.basename(paths[i]), "seed": seed, "image_shape": (h, w_, c), "block_size": infos[i]["block_size"],
                           "status": int(status[k]), "decomp_time": dt}
                if status[k]:
                    rows[i]["error"] = texts[k]
    if strict:
        for i, row in enumerate(rows):
            if row["status"]:
                raise CodingError(f"{row['error']} (image {i})")
    shapes = {tuple(im.shape) for im in images if im is not None}
    if len(shapes) == 1 and all(im is not None for im in images):
        return torch.stack(images, dim=0), rows
    return images, rows


def _decompress_images(model, paths, batch, strict, lossless, tables=None):
    """_decompress_groups for BidirectionalResNetVAE: the files' bytes uploaded once per batch and decoded by model.decompress_rec[_tables]
    -- the arithmetic decoder, the row checks and the generative pass on the device, one read-back (the per-image status) per batch.
    lossless: beside every NAME.rec lies NAME.res (a missing one reads as an empty file); the images are the uint8 pixels of
    model.decompress_lossless, and status may be STATUS_RESIDUAL + irec_res_status."""
    from .io.residual import stream_len_of
    dev = next(model.parameters()).device

    def fits(info, key):
        _, (h, w, c), R, bpt = key
        return isinstance(bpt, int) and R == model.num_res_blocks and c == 3 and h % 2 == 0 and w % 2 == 0 and bpt == model.blocks_per_tensor((1, c, h, w))

    def decode(part, info, blob, off, seed, shape, max_K):
        if lossless:
            res = [_read(os.path.splitext(paths[i])[0] + ".res", missing=b"") for i in part]
            res_blob, res_off = _joined(res)
            L = stream_len_of(res[0])
            rec, status, K = model._decompress_lossless_status(_upload(blob, dev), off, _upload(res_blob, dev), res_off, seed, shape, max_K,
                                                               L if L and 1 <= L <= 4096 else None)
        else:
            rec, status, K = model._decompress_rec_status(_upload(blob, dev), off, seed, shape, max_K, tables)
        return rec, status, [model.status_text(st, K[k]) if st else "" for k, st in enumerate(status)]
    return _decompress_groups(model, paths, batch, strict, fits, decode, tables, lossless)


def decompress_images(model, paths, batch=None, strict=True):
    """The read side of compress_images (_decompress_groups has the description)."""
    return _decompress_images(model, paths, batch, strict, False)


def decompress_images_tables(model, paths, tables, batch=None, strict=True):
    """decompress_images for files written under an irec.io.SymbolTables (compress_images(tables=)); files without header flags decode
    in the same call.  A function of its own: decompress_images' signature is pinned."""
    return _decompress_images(model, paths, batch, strict, False, tables)


def decompress_images_lossless(model, paths, batch=None, strict=True):
    """The read side of compress_images(lossless=True): decompress_images over NAME.rec + NAME.res pairs (`paths` names the .rec
    files), the images being the uint8 pixels.  A function of its own: decompress_images' signature is pinned."""
    return _decompress_images(model, paths, batch, strict, True)


# ---- the lossy models (irec.models.lossy: Large2LevelVAE, Large1LevelVAE): the same two drivers over ragged files -------------------
def _gaussian_kl_per_image(posterior, prior):
    """sum over an image's latent dims of KL(N(loc_q, scale_q) || N(loc_p, scale_p)), closed form, float64 on the device: [N]."""
    mq, sq, mp, sp = (t.to(torch.float64) for t in (posterior.loc, posterior.scale, prior.loc, prior.scale))
    kl = torch.log(sp / sq) + (sq * sq + (mq - mp) ** 2) / (2.0 * sp * sp) - 0.5
    return kl.reshape(kl.shape[0], -1).sum(dim=1)


def _psnr_ms_ssim(reconstruction, chunk, image_range):
    """(psnr, ms_ssim) float64 [m] on the device, irec.metrics under the reference's convention for images in image_range.  An image
    with a side below metrics.min_side(5) = 161 has no five-scale MS-SSIM (tf.image.ssim_multiscale asserts there): its ms_ssim is
    NaN, its psnr what it is.  Only the any-size driver brings such images; at 161 and above the call is metrics.quality, as it was."""
    from . import metrics
    kw = metrics.transform_for(image_range)
    if min(chunk.shape[2:]) >= metrics.min_side(metrics.MAX_SCALES):
        return metrics.quality(reconstruction, chunk, **kw)[:2]
    psnr = metrics.psnr(reconstruction, chunk, **kw)
    return psnr, torch.full_like(psnr, float("nan"))


def _lossy_quality_columns(model, chunk, reconstruction, image_range):
    """float64 [3, m] on the device: psnr, ms_ssim of the reconstruction against the chunk (irec.metrics, the reference's convention
    for images in image_range) and the levels' KL in nats, from the distributions the model's last pass left (a two-level model's
    level_1_* and level_2_*, a one-level model's posterior and prior).  No synchronisation."""
    from . import metrics
    psnr, ms_ssim = _psnr_ms_ssim(reconstruction, chunk, image_range)
    if hasattr(model, "level_1_posterior"):
        kld = _gaussian_kl_per_image(model.level_1_posterior, model.level_1_prior) + \
            _gaussian_kl_per_image(model.level_2_posterior, model.level_2_prior)
    else:
        kld = _gaussian_kl_per_image(model.posterior, model.prior)
    return torch.stack([psnr, ms_ssim, kld])


def _lossy_ideal_columns(model, chunk, seed, image_base, image_range):
    """float64 [3, m] on the device: psnr, ms_ssim of the reconstruction of a seeded sampling pass over the chunk against the chunk, and
    the pass's KL (every level's, irec.ideal.posterior_draw's, added in file order) in nats.  No synchronisation."""
    from . import metrics
    _, reconstruction = model.forward(chunk, seed=seed, image_base=image_base)
    psnr, ms_ssim = _psnr_ms_ssim(reconstruction, chunk, image_range)
    kl, *more = model.kl_divergence()
    for level in more:
        kl = kl + level
    return torch.stack([psnr, ms_ssim, kl])


def _lossy_groups(images, resize):
    """What compress_images_lossy codes: ([(images [m, 3, H, W] float32, members)], sizes) -- the images brought to the size they are
    coded at and grouped by it, a group's members being its images' numbers in the call, in order, the groups in the order of their
    first image; sizes[i] = (orig_h, orig_w, h, w), or None for the call of one 4-D float tensor as it is (resize=False), which is one
    group and passes through untouched.  A list holds [3, h_i, w_i] tensors, float32 or uint8 (x / 255); resize=True brings every
    image to image.driver_size(h_i, w_i) through image.resize_bilinear, images of one size in one launch.  ValueError, before
    anything is coded, for an image below 64 x 64 or, with resize=False, one whose sides are not multiples of 64."""
    from . import image
    if isinstance(images, torch.Tensor) and images.dim() == 4 and not resize and images.dtype != torch.uint8:
        return [(images, list(range(images.shape[0])))], None
    images = list(images)
    for i, im in enumerate(images):
        if not isinstance(im, torch.Tensor) or im.dim() != 3 or im.shape[0] != 3 or im.dtype not in (torch.float32, torch.uint8):
            raise ValueError(f"compress_images_lossy: image {i} is not a [3, h, w] float32 or uint8 tensor")
    sizes = []
    for i, im in enumerate(images):
        h, w = int(im.shape[1]), int(im.shape[2])
        if resize:
            sizes.append((h, w, *image.driver_size(h, w)))
        elif h % 64 or w % 64 or not h or not w:
            raise ValueError(f"compress_images_lossy: image {i} is {h} x {w}; the models code multiples of 64 (resize=True brings an "
                             "image to the next one below, as the reference's driver does)")
        else:
            sizes.append((h, w, h, w))
    sources, coded = {}, [None] * len(images)
    for i, im in enumerate(images):
        sources.setdefault((sizes[i], im.dtype), []).append(i)
    for (size, dtype), members in sources.items():
        stacked = torch.stack([images[i] for i in members])
        if resize or dtype == torch.uint8:                    # (equal sizes: the copy that converts)
            stacked = image.resize_bilinear(stacked, size[2:])
        for k, i in enumerate(members):
            coded[i] = stacked[k]
    groups = {}
    for i, size in enumerate(sizes):
        groups.setdefault(size[2:], []).append(i)
    return [(torch.stack([coded[i] for i in members]), members) for members in groups.values()], sizes


def _runs(members):
    """[(a, b)]: members[a:b] the maximal runs of consecutive numbers."""
    cuts = [0] + [k for k in range(1, len(members)) if members[k] != members[k - 1] + 1] + [len(members)]
    return list(zip(cuts[:-1], cuts[1:]))


def compress_images_lossy(model, sampler, images, names, seed, block_size, out_dir, batch=None, rec_on_device=False, tables=None,
                          quality=False, image_range=(0., 1.), segment_blocks=None, ideal=False, resize=False):
    """compress_images for a lossy model (Large2LevelVAE, Large1LevelVAE) and its coder `sampler`: images [n, 3, H, W] on the model's
    device, in batches through model.compress_rec (one coder launch per level and batch, one read-back), one NAME.rec per image --
    byte for byte the file model.compress(file_path, ...) writes for it -- read back and compared with the rows the files were built from.
    rec_on_device: the files are built and checked on the device (irec.io.encode_files_device_ragged / decode_files_device_ragged)
    instead of on host threads, the default.  tables: an irec.io.SymbolTables (fit_symbol_tables_lossy) the files are coded under.
    Returns one dict per image with compress_images' keys.
    images may also be a LIST of [3, h_i, w_i] tensors, float32 or uint8 (x / 255), of any sizes: with resize=True every image is brought
    to image.driver_size(h_i, w_i) = (h_i - h_i % 64, w_i - w_i % 64) by image.resize_bilinear -- the reference driver's
    tf.image.resize (compress_with_lossy_model.py:183-184), on the device -- the images are grouped by the size they are coded at and
    coded group by group in batches, and the rows come back in the order of the images, each also carrying `orig_h`, `orig_w`, `h`,
    `w`; quality and ideal measure against the RESIZED image, as the reference does.  resize=True takes a 4-D tensor too.
    resize=False with a list wants every side a multiple of 64: ValueError otherwise, before out_dir exists.  resize=False with one
    4-D float tensor: the call, the work and the rows are what they were.
    quality=True: every row also carries the distortion half of the reference's results row
    (examples/lossy/compress_with_lossy_model.py:192-270) -- `psnr` and `ms_ssim` of compress_rec's reconstruction against the
    image (irec.metrics on the device: tf.image.psnr / tf.image.ssim_multiscale of clip(reconstruction) * 255 against image * 255 for
    images in image_range, (0, 1) as the reference has them, (-0.5, 0.5) as the shim's tests do; images of at least 161 x 161 for all
    five scales of ms_ssim, fewer scales below),
    `kld`, the closed-form Gaussian KL of every level in nats (float64 on the device), and `lossy_bpp` = kld / (h w ln 2) -- all
    of it in ONE extra read-back per batch.  quality=False: the rows and the work are as before.
    ideal=True: every row also carries the ideal half of that row (compress_with_lossy_model.py:193-215), from a seeded sampling
    forward pass over the batch (model.forward(chunk, seed=seed, image_base=the image's number in the call): the library's own seeded
    draws, irec.ideal, where the reference's are unseeded; a batch of a group whose images are not neighbours in the call takes one
    pass per run of neighbours) -- `ideal_psnr` and `ideal_ms_ssim` of that pass's reconstruction
    (irec.metrics, as above), `ideal_kld`, every level's KL in nats through irec.ideal's kernel, and `ideal_lossy_bpp` =
    ideal_kld / (h w ln 2) -- read back with the batch's one extra copy.  ideal=False: the rows and the work are as before.
    segment_blocks: None for the reference's files; g >= 1 writes NAME.recs, the segmented container (model.compress_rec has the
    description; default symbol models only, so together with tables it is a ValueError), on host threads or on the device alike."""
    from .io import decode_files_device_ragged, decode_files_device_segmented, decode_files_ragged, decode_files_segmented
    if segment_blocks is not None and tables is not None:
        raise ValueError("compress_images_lossy: the segmented container codes under the default symbol models only (tables= with segment_blocks=)")
    seed = header_seed(seed, "compress_images_lossy")      # (before out_dir is made or a batch coded)
    groups, sizes = _lossy_groups(images, resize)           # (likewise)
    os.makedirs(out_dir, exist_ok=True)
    S = model._max_index(sampler)
    ragged, segmented = (decode_files_device_ragged, decode_files_device_segmented) if rec_on_device else (decode_files_ragged, decode_files_segmented)
    out = [None] * sum(len(members) for _, members in groups)

    for group, members in groups:
        group_names = [names[i] for i in members]

        def leg(lo, hi):
            chunk = group[lo:hi]
            _, _, h, w = chunk.shape
            t0 = time.perf_counter()
            (blob, off, reconstruction), (K, idx, bpr) = model.compress_rec(chunk, seed, sampler, block_size=block_size, rec_on_device=rec_on_device,
                                                                            return_pendings=True, tables=tables, segment_blocks=segment_blocks)
            columns = _lossy_quality_columns(model, chunk, reconstruction, image_range) if quality else None   # (launched; read below)
            if ideal:                                                            # (after the quality columns: the pass replaces the model's distributions)
                ideal_columns = [_lossy_ideal_columns(model, chunk[a:b], seed, members[lo + a], image_range) for a, b in _runs(members[lo:hi])]
                ideal_columns = ideal_columns[0] if len(ideal_columns) == 1 else torch.cat(ideal_columns, dim=1)
                columns = ideal_columns if columns is None else torch.cat([columns, ideal_columns])
            t_compress, t1 = time.perf_counter() - t0, time.perf_counter()
            if segment_blocks is None:
                decode = lambda b, o: ragged(b, o, bpr, idx.shape[2], tables=tables)  # noqa: E731
            else:
                decode = lambda b, o: segmented(b, o, bpr, idx.shape[2], segment_blocks)  # noqa: E731
            rows = _check_leg(out_dir, group_names[lo:hi], "rec" if segment_blocks is None else "recs", blob, off, K, idx, decode,
                              (seed, block_size, h, w, 3), S, t_compress, t1)
            host = columns.cpu().numpy() if (quality or ideal) else None         # the one extra read-back
            if quality:
                psnr, ms_ssim, kld = host[:3]
                for i, row in enumerate(rows):
                    row.update({"psnr": float(psnr[i]), "ms_ssim": float(ms_ssim[i]), "kld": float(kld[i]),
                                "lossy_bpp": float(kld[i]) / (h * w * float(np.log(2.0)))})
            if ideal:
                psnr, ms_ssim, kld = host[-3:]
                for i, row in enumerate(rows):
                    row.update({"ideal_psnr": float(psnr[i]), "ideal_ms_ssim": float(ms_ssim[i]), "ideal_kld": float(kld[i]),
                                "ideal_lossy_bpp": float(kld[i]) / (h * w * float(np.log(2.0)))})
            return rows
        m = len(members)
        for i, row in zip(members, (row for rows in _in_batches(m, m if not batch else int(batch), group_names, leg) for row in rows)):
            if sizes is not None and "error" not in row:
                row.update(dict(zip(("orig_h", "orig_w", "h", "w"), sizes[i])))
            out[i] = row
    return out


def decompress_images_lossy(model, sampler, paths, batch=None, strict=True, rec_on_device=False, tables=None):
    """decompress_images for a lossy model (Large2LevelVAE, Large1LevelVAE) and its coder `sampler`: .rec files -> (images, rows), the
    files grouped by header (seed, shape, block structure) -- files of several image sizes, as compress_images_lossy writes for a list,
    decode in one call and come back as a list in the order of `paths`; a file whose block structure is not the model's own (another
    level count among them: a two-level file under a one-level model) has status 17 -- and each group decoded in batches by
    model.decompress_rec -- on host threads, or with rec_on_device on
    the device -- with one read-back per batch, the per-image status.  images, rows and strict as decompress_images has them.
    tables: the irec.io.SymbolTables the files were written under (files without header flags decode in the same call).
    Segmented files (NAME.recs) are told from the reference's by their magic and decoded in groups of their own, under the
    segment_blocks their headers name and the default symbol models."""
    dev = next(model.parameters()).device

    def fits(info, key):
        _, (h, w, c), R, _ = key
        if not (c == 3 and h % 64 == 0 and w % 64 == 0 and h > 0 and w > 0 and info.get("segment_blocks") != 0):
            return False
        bpr = model.blocks_per_res((1, c, h, w), sampler.block_size)    # (one entry per level: a file of R blocks is a model of R levels')
        return R == len(bpr) and list(info["bpt"]) == bpr

    def decode(part, info, blob, off, seed, shape, max_K):
        g = info.get("segment_blocks")                   # None: the reference's container
        rec, status = model.decompress_rec(_upload(blob, dev) if rec_on_device else blob, off, seed, shape, sampler, max_K=max_K,
                                           strict=False, rec_on_device=rec_on_device, tables=tables if g is None else None, segment_blocks=g)
        return rec, status, [status_text(int(st)) if st else "" for st in status]
    return _decompress_groups(model, paths, batch, strict, fits, decode, tables)


# ---- fitting symbol tables (irec.io.SymbolTables) to a model's own rows -----------------------------------------------------------------
def _fit_batches(batches, n_index_values, n_count_values):
    """hist_rows over (K [N, T], idx [N, T, max_K], blocks_per_res) device batches, accumulated on the device, finalised once."""
    from .io import hist_rows, tables_from_histograms
    hist = None
    for K, idx, bpr in batches:
        hist = hist_rows(K, idx, bpr, n_index_values, n_count_values, into=hist)
    if hist is None:
        raise ValueError("fit_symbol_tables: no images")
    host = hist.numpy()
    if int(host.rejected[0]):
        raise CodingError(f"fit_symbol_tables: {int(host.rejected[0])} values outside the tables' ranges")
    return tables_from_histograms(host)


def fit_symbol_tables(model, images, seed, batch=None, max_K=None):
    """An irec.io.SymbolTables fitted to what BidirectionalResNetVAE `model` codes for `images` [n, 3, H, W] (on its device): the
    batches go through the model's packed device pass, their rows are histogrammed where they lie (irec.io.hist_rows) and the counts
    are read back once.  One index table over the coder's samples, one count table per residual block over K in [0, max_K]
    (default: the largest index-slot count a batch came with, doubled: a K the fit never saw still has a symbol)."""
    from .coding.pending import PendingCode, recode
    n = images.shape[0]
    step = n if not batch else int(batch)
    coder = model.residual_blocks[0].coder
    S = coder.sampler.n_samples() if coder.sampler is not None else coder.n_samples
    rows = []
    with torch.no_grad():
        for lo in range(0, n, step):
            (K, idx), _ = recode(lambda: model._compress_device(images[lo:lo + step], seed, False), PendingCode.gather_packed_device,
                                 [b.coder for b in model.residual_blocks])
            m, R, bpt = K.shape
            rows.append((K.reshape(m, R * bpt), idx.reshape(m, R * bpt, idx.shape[3]), [bpt] * R))
    if max_K is None:
        max_K = 2 * max(idx.shape[2] for _, idx, _ in rows)
    return _fit_batches(rows, S, int(max_K) + 1)


def fit_likelihood_scale(model, images, seed, per_channel=False, batch=None, block_size=None):
    """Fit BidirectionalResNetVAE `model`'s likelihood scale to uint8 `images` [n, 3, H, W] (on its device) and set it on the model
    (model.fit_likelihood_scale: the batches' pixels are costed where they lie under candidate scales, one small read-back per round
    of the search): one scale, and version-1 .res files as before, or with per_channel=True one per colour channel and version-2
    files.  compress_images(lossless=True) and decompress_images_lossless work with the model as it then is.  Returns the fitted
    log-scale(s) and their coded bits, (float, float) or (float64 [3], float64 [3])."""
    log_scales, units, _ = model.fit_likelihood_scale(images, seed, per_channel=per_channel, batch=batch, block_size=block_size)
    return log_scales, np.asarray(units, dtype=np.float64) / 65536.0 if per_channel else float(units) / 65536.0


def fit_symbol_tables_lossy(model, sampler, images, seed, block_size, batch=None, max_K=None):
    """fit_symbol_tables for a lossy model (Large2LevelVAE, Large1LevelVAE) and its coder `sampler`: one index table, one count table
    for each of the model's levels.
    block_size: the coder's, as compress_images_lossy takes it (the layout is the sampler's own)."""
    from .coding.pending import PendingCode
    n = images.shape[0]
    step = n if not batch else int(batch)
    rows = []
    with torch.no_grad():
        for lo in range(0, n, step):
            (K, idx, bpr), _ = model._compress_gather(images[lo:lo + step], seed, sampler, PendingCode.gather_packed_ragged_device)
            rows.append((K, idx, bpr))
    if max_K is None:
        max_K = 2 * max(idx.shape[2] for _, idx, _ in rows)
    return _fit_batches(rows, model._max_index(sampler), int(max_K) + 1)


def compress_sharded(model, all_images, seed, block_size, out_dir, rank=0, world=1, dist=None, batch=None):
    """Config 3 (300 images over G GPUs): this rank compresses images rank, rank + G, ...; every rank gets the [n_images]
    vectors of file bits and code nats back (one all_gather each, <= 38 floats per rank: latency only)."""
    n_items = all_images.shape[0]
    mine = sharding.shard_indices(n_items, rank, world)
    names = [f"img_{int(i):05d}" for i in mine]
    dev = next(model.parameters()).device
    rows = compress_images(model, all_images[torch.as_tensor(mine)].to(dev), names, seed, block_size, out_dir, batch)
    coll_dev = dev if (dist is not None and dist.get_backend() == "nccl") else torch.device("cpu")
    bits = torch.tensor([r.get("comp_codelength", -1) for r in rows], dtype=torch.float64, device=coll_dev)
    nats = torch.tensor([r.get("code_nats", -1.0) for r in rows], dtype=torch.float64, device=coll_dev)
    all_bits = sharding.gather_per_item(bits, n_items, rank, world, dist)
    all_nats = sharding.gather_per_item(nats, n_items, rank, world, dist)
    return rows, all_bits, all_nats
