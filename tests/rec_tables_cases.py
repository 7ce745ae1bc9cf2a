"""Shared by tests/test_rec_tables_host.py and tests/test_rec_tables_gpu.py: the cases of the .rec coder under empirical symbol tables,
their referee results -- the files that the reference-shaped Python writer (_write_compressed_code_py: one ArithmeticCoder call per
stream, tables loaded from .npy) makes of every image, computed once and never changed --, the core's host hooks
(irec_rec_test_core_*_tables: csrc/irec_rec_core.h over irec_rec::Tables in a plain loop) and the damaged set of flagged files."""
import functools
import os
import tempfile

import numpy as np

SEED, SHAPE, BLOCK_SIZE, MAX_K = 42, (32, 48, 3), 1000, 9
LDS_SYMBOLS = 4096                                   # IREC_REC_TABLE_LDS_SYMBOLS (irec._lib.REC_TABLE_LDS_SYMBOLS; test_rec_tables_host pins it)

# (N, blocks_per_res): one stream of a kind | uniform | ragged | 420 streams of a kind: more than one 256-lane workgroup | R at
# IREC_REC_RAGGED_MAX_RES.  "zeroK": a call whose every K is 0 (streams of a terminator alone, no index at all)
LAYOUTS = {"1x1": (1, (1,)), "3x3_3": (3, (3, 3)), "5x4_1_7": (5, (4, 1, 7)), "70x2_2_2": (70, (2, 2, 2)), "2x64ones": (2, (1,) * 64),
           "zeroK": (3, (3, 3))}
COMBOS = ("index", "counts", "both")
COUNT_LENGTHS = (11, 3, 16)                          # symbols of the count table of residual block r, cycled: K <= 9, 1, 14


def index_tables():
    """name -> counts (terminator first).  one value | geometric | all ones: the smallest total | total exactly 2^30 | a table that is
    staged in LDS whole | one symbol more: read from global memory."""
    rng = np.random.default_rng(7)
    return {"one": np.array([1, 5], dtype=np.int64),
            "geo20": np.array([7] + [max(1, (1 << 20) >> m) for m in range(1, 21)], dtype=np.int64),
            "ones20": np.ones(21, dtype=np.int64),
            "total2p30": np.array([1, (1 << 30) - 3, 1, 1], dtype=np.int64),
            "lds": rng.integers(1, 65, LDS_SYMBOLS).astype(np.int64),
            "lds_plus1": rng.integers(1, 65, LDS_SYMBOLS + 1).astype(np.int64)}


def count_tables(R):
    """Skewed, lengths differing per residual block; the values 8 and up have count 1 (and K = 9 is used: make_rows)."""
    return [np.array([3] + [max(1, 256 >> m) for m in range(COUNT_LENGTHS[r % 3] - 1)], dtype=np.int64) for r in range(R)]


def make_rows(rng, n, bpr, index_counts, with_count_tables, zero=False):
    """K [N, T] in [0, MAX_K] with zeros (within every count table's range), idx [N, T, MAX_K] within the index table's."""
    T, first = sum(bpr), np.concatenate([[0], np.cumsum(bpr)])
    K = rng.integers(0, MAX_K + 1, (n, T)).astype(np.int32)
    K[rng.random((n, T)) < 0.15] = 0
    if with_count_tables:
        for r in range(len(bpr)):
            K[:, first[r]:first[r + 1]] = np.minimum(K[:, first[r]:first[r + 1]], COUNT_LENGTHS[r % 3] - 2)
        K[0, 0] = MAX_K                                                # a used value of count 1
    if zero:
        K[:] = 0
    n_values = len(index_counts) - 1 if index_counts is not None else 20
    if index_counts is not None and len(index_counts) == 4 and index_counts[1] > (1 << 29):
        idx = rng.choice(3, size=(n, T, MAX_K), p=[0.98, 0.01, 0.01]).astype(np.int32)      # almost all 0
    else:
        idx = rng.integers(0, n_values, (n, T, MAX_K)).astype(np.int32)
        if K[0, 0] > 0:
            idx[0, 0, 0] = n_values - 1                                # the last value is used
    return K, idx


def case_names():
    return [f"{lay}-{combo}" for lay in LAYOUTS for combo in COMBOS] + [f"3x3_3-index-{t}" for t in index_tables() if t != "geo20"]


def lists_of(K, idx, bpr):
    first = np.concatenate([[0], np.cumsum(bpr)])
    return [[[idx[i, b, :K[i, b]].tolist() for b in range(first[r], first[r + 1])] for r in range(len(bpr))] for i in range(K.shape[0])]


def python_files(K, idx, bpr, max_index, tables, directory):
    """_write_compressed_code_py per image, the tables saved in the reference's .npy forms: (files, index file or None, count file or None)."""
    from irec.io import utils as U
    fi = os.path.join(directory, "index_counts.npy") if tables.index_counts is not None else None
    fc = os.path.join(directory, "num_aux_var_counts.npy") if tables.num_aux_var_counts is not None else None
    tables.save(fi, fc)
    files = []
    for i, lists in enumerate(lists_of(K, idx, bpr)):
        path = os.path.join(directory, f"py_{i}.rec")
        U._write_compressed_code_py(path, SEED, SHAPE, BLOCK_SIZE, lists, max_index, fc, fi)
        with open(path, "rb") as fh:
            files.append(fh.read())
    return files, fi, fc


@functools.lru_cache(maxsize=None)
def cases():
    """Every case with its referee result, read-only: files (the Python writer per image), blob / offsets (their concatenation)."""
    from irec.io import SymbolTables
    rng = np.random.default_rng(20260131)
    itabs = index_tables()
    plan = [(lay, combo, "geo20") for lay in LAYOUTS for combo in COMBOS] + [("3x3_3", "index", t) for t in itabs if t != "geo20"]
    out = []
    with tempfile.TemporaryDirectory() as d:
        for lay, combo, tname in plan:
            n, bpr = LAYOUTS[lay]
            ic = itabs[tname] if combo in ("index", "both") else None
            cc = count_tables(len(bpr)) if combo in ("counts", "both") else None
            K, idx = make_rows(rng, n, bpr, ic, cc is not None, zero=lay == "zeroK")
            tables = SymbolTables(ic, cc)
            max_index = len(ic) - 1 if ic is not None else 20
            files, _, _ = python_files(K, idx, bpr, max_index, tables, d)
            c = {"name": f"{lay}-{combo}" + ("" if tname == "geo20" else f"-{tname}"), "K": K, "idx": idx, "bpr": bpr, "max_index": max_index,
                 "tables": tables, "files": files, "blob": np.frombuffer(b"".join(files), dtype=np.uint8),
                 "offsets": np.concatenate([[0], np.cumsum([len(f) for f in files])]).astype(np.int64),
                 "idx_zeroed": np.where(np.arange(MAX_K)[None, None, :] < K[..., None], idx, 0).astype(np.int32)}
            for a in (c["K"], c["idx"], c["blob"], c["offsets"], c["idx_zeroed"]):
                a.setflags(write=False)
            out.append(c)
    assert [c["name"] for c in out] == case_names()
    return tuple(out)


def joined(K, idx):
    """One [rows][1 + width] tensor, K in column 0 (what PendingCode.gather_packed_ragged builds on the device)."""
    return np.ascontiguousarray(np.concatenate([K.reshape(-1, 1), idx.reshape(K.size, -1)], axis=1).astype(np.int32))


def raw_tables(tables):
    """(index_cum, n_index_symbols, count_cum, count_first, n_count_cum) as arrays (None where the call has no such table)."""
    return (tables.index_cum, tables.n_index_symbols, tables.count_cum, tables.count_first, 0 if tables.count_cum is None else tables.count_cum.size)


def _ptr(a):
    return None if a is None else a.ctypes.data


def core_encode(K, idx, max_index, bpr, raw, cap, strided=False):
    """irec_rec_test_core_encode_files_tables over `raw` = (index_cum, n_index_symbols, count_cum, count_first, n_count_cum), which goes
    to the core as it is: (out uint8 [cap + 8] pre-filled with 0xAB, offsets, status), all pre-filled so that an untouched output shows."""
    from irec import _lib
    lib = _lib.load()
    bpr = np.asarray(bpr, dtype=np.int32)
    n, mk = K.shape[0], idx.shape[2]
    if strided:
        both = joined(K, idx)
        k_ptr, ks, i_ptr, ist = both.ctypes.data, 1 + mk, both.ctypes.data + 4, 1 + mk
    else:
        K, idx = np.ascontiguousarray(K, dtype=np.int32), np.ascontiguousarray(idx, dtype=np.int32)
        k_ptr, ks, i_ptr, ist = K.ctypes.data, 1, idx.ctypes.data, mk
    out = np.full(cap + 8, 0xAB, dtype=np.uint8)
    offsets, status = np.full(n + 1, -1, dtype=np.int64), np.full(n, -1, dtype=np.int32)
    ic, ni, cc, cf, ncc = raw
    st = lib.irec_rec_test_core_encode_files_tables(SEED, BLOCK_SIZE, max_index, *SHAPE, n, bpr.size, bpr.ctypes.data, mk, k_ptr, ks, i_ptr, ist,
                                                    _ptr(ic), ni, _ptr(cc), _ptr(cf), ncc, out.ctypes.data, cap, offsets.ctypes.data,
                                                    status.ctypes.data)
    assert st == 0, lib.irec_last_error()
    return out, offsets, status


def core_decode(blob, offsets, bpr, mk, raw):
    """irec_rec_test_core_decode_files_tables: (headers uint32 [N, 9], K [N, T], idx [N, T, mk], status), outputs pre-filled with -1."""
    from irec import _lib
    lib = _lib.load()
    bpr = np.asarray(bpr, dtype=np.int32)
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    if blob.size == 0:
        blob = np.zeros(1, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    n, T = offsets.size - 1, int(bpr.sum())
    hdr = np.full((n, 9), 0xFFFFFFFF, dtype=np.uint32)
    K = np.full((n, T), -1, dtype=np.int32)
    idx = np.full((n, T, mk), -1, dtype=np.int32)
    status = np.full(n, -1, dtype=np.int32)
    ic, ni, cc, cf, ncc = raw
    st = lib.irec_rec_test_core_decode_files_tables(blob.ctypes.data, offsets.ctypes.data, n, bpr.size, bpr.ctypes.data, mk, _ptr(ic), ni, _ptr(cc),
                                                    _ptr(cf), ncc, hdr.ctypes.data, K.ctypes.data, idx.ctypes.data, status.ctypes.data)
    assert st == 0, lib.irec_last_error()
    return hdr, K, idx, status


# ---- the damaged set: the truncations and replaced bytes of rec_device_cases.damaged_set(), applied to a flagged file ----------------------
DAMAGED_BPR, DAMAGED_MK = (9,) * 6, 29


def _python_verdict(raw, fi, fc, directory):
    """What the reference-shaped reader makes of one file: None if _read_compressed_code_py raises, or if what it returns is not a
    file of the call's structure -- the checks that the batched readers add and the Python reader, which trusts its file, does not have:
    no largest-K word above 65536 in a file without the count flag; the streams lie inside the file; max_index in [1, 2^24]; R and the blocks per residual block are the call's; no K above max_K; as
    many indices as the counts say.  Else (header words, K [T], idx [T, max_K])."""
    import io
    from irec.io import utils as U
    path = os.path.join(directory, "damaged.rec")
    with open(path, "wb") as fh:
        fh.write(raw)
    try:
        hdr = U.RecHeader.read(io.BytesIO(raw))
        if not hdr.uses_count_file and max(hdr.max_partitions, default=0) > 65536:
            return None                   # (IREC_REC_E_BLOCK_COUNTS; the Python reader would build a default model of that many symbols)
        seed, shape, bs, blocks = U._read_compressed_code_py(path, 28, fc, fi)
    except Exception:
        return None
    if 28 + 16 * len(hdr.blocks_per_res_block) + sum(hdr.count_stream_bytes) + sum(hdr.index_stream_bytes) > len(raw):
        return None
    if not 1 <= hdr.max_index <= 1 << 24 or tuple(hdr.blocks_per_res_block) != DAMAGED_BPR or [len(rb) for rb in blocks] != list(DAMAGED_BPR):
        return None
    tables, index_table = np.load(fc, allow_pickle=True), np.load(fi)
    at = 28 + 16 * len(DAMAGED_BPR)
    x_at = at + sum(hdr.count_stream_bytes)
    K = np.zeros(sum(DAMAGED_BPR), dtype=np.int32)
    idx = np.zeros((sum(DAMAGED_BPR), DAMAGED_MK), dtype=np.int32)
    b = 0
    for r, rb in enumerate(blocks):
        counts = U._decode_stream(tables[r], raw[at:at + hdr.count_stream_bytes[r]])       # (the lists alone hide a count the stream did not honour)
        at += hdr.count_stream_bytes[r]
        if len(counts) != len(rb) or [len(ix) for ix in rb] != counts.tolist() or (counts > DAMAGED_MK).any():
            return None
        model = index_table if hdr.uses_index_file else U._uniform_model(hdr.max_index, 1000)
        if len(U._decode_stream(model, raw[x_at:x_at + hdr.index_stream_bytes[r]])) != int(counts.sum()):
            return None                   # (more indices than the counts say: the lists, cut by the counts, do not show them)
        x_at += hdr.index_stream_bytes[r]
        for ix in rb:
            K[b] = len(ix)
            idx[b, :len(ix)] = ix
            b += 1
    return U._STATIC.unpack(raw[:28]), K, idx       # (the nine words as they stand in the file: a flag word is any nonzero value)


@functools.lru_cache(maxsize=None)
def damaged_set():
    """One flagged container (both kinds under tables) of rec_device_cases.damaged_set()'s rows and, as ONE blob: every prefix, 800 copies
    with one to three random bytes replaced, 200 copies with one byte replaced inside the seed, block-size, height, width and channel
    fields.  With the Python reader's verdict on every file (_python_verdict): ok, and where it accepts, headers / K / idx."""
    import rec_device_cases as D
    from irec.io import SymbolTables
    d0 = D.damaged_set()
    R, bpt, mk = D.DAMAGED_SHAPE
    assert (bpt,) * R == DAMAGED_BPR and mk == DAMAGED_MK
    K0, idx0 = d0["K0"].reshape(1, R * bpt), d0["idx0"].reshape(1, R * bpt, mk)
    rng = np.random.default_rng(12)
    tables = SymbolTables(rng.integers(1, 200, 37), [rng.integers(1, 50, mk + 2) for _ in range(R)])
    with tempfile.TemporaryDirectory() as d:
        (data,), fi, fc = python_files(K0, idx0, DAMAGED_BPR, 36, tables, d)
        files = [data[:n] for n in range(len(data))]
        for _ in range(800):
            b = bytearray(data)
            for _ in range(int(rng.integers(1, 4))):
                b[int(rng.integers(0, len(b)))] = int(rng.integers(0, 256))
            files.append(bytes(b))
        fields = list(range(0, 8)) + list(range(12, 22))
        for _ in range(200):
            b = bytearray(data)
            b[fields[int(rng.integers(0, len(fields)))]] = int(rng.integers(0, 256))
            files.append(bytes(b))
        verdicts = [_python_verdict(raw, fi, fc, d) for raw in files]
    ok = np.array([v is not None for v in verdicts])
    hdr = np.zeros((len(files), 9), dtype=np.uint32)
    K = np.zeros((len(files), R * bpt), dtype=np.int32)
    idx = np.zeros((len(files), R * bpt, mk), dtype=np.int32)
    for f, v in enumerate(verdicts):
        if v is not None:
            hdr[f], K[f], idx[f] = v
    out = {"blob": np.frombuffer(b"".join(files), dtype=np.uint8), "tables": tables, "ok": ok, "hdr": hdr, "K": K, "idx": idx, "n_prefix": len(data),
           "offsets": np.concatenate([[0], np.cumsum([len(f) for f in files])]).astype(np.int64)}
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out
