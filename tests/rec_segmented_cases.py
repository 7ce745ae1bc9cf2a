"""Shared by tests/test_rec_segmented_host.py and tests/test_rec_segmented_gpu.py: the segmented .rec container (NAME.recs,
INTEGRATION.md §8) restated in Python, the cases, their expected files, the damaged set and the core's host hooks.  A helper, no tests.

The restatement shares nothing with csrc/irec_rec_seg_core.h: a file is put together field by field with `struct`, and every stream is
one call of an arithmetic coder on the message `values + 1, 0` under the default model, '1' + code as a big-endian integer -- exactly
what write_compressed_code does for a residual block, here for the blocks of one segment.  The coder is irec.io.ArithmeticCoder
(irec_ac_encode, which tests/test_rec_io.py holds to the reference bit for bit) or, through `coder=`, the compiled reference's own."""
import functools
import struct

import numpy as np

import rec_ragged_cases as RC

STRUCTURES = RC.STRUCTURES                               # blocks per residual block -> max_K
N_IMAGES, MAX_INDEX = RC.N_IMAGES, RC.MAX_INDEX
SEGMENT_BLOCKS = (1, 2, 4, 16, 512)                      # 512 exceeds every block count: one segment per residual block
SEED, SHAPE, BLOCK_SIZE = RC.SEED, RC.SHAPE, RC.BLOCK_SIZE
E_SEG_MAGIC, E_SEG_DIRECTORY, E_SEG_BLOCKS = 20, 21, 22  # irec_rec_status of include/irec.h


EDGES = (((1, 4), 0, 36, 0), ((3, 1, 5), 3, 36, 0))       # (structure, N, max_index, max_K) beside the grid: no images; no index slots


def grid():
    """[(blocks per residual block, N, max_index, max_K)]: every structure with its max_K at every N and max_index, then EDGES."""
    return [(bpr, n, S, STRUCTURES[bpr]) for bpr in STRUCTURES for n in N_IMAGES for S in MAX_INDEX] + list(EDGES)


def case_names():
    return [f"{'_'.join(map(str, bpr))}-N{n}-S{S}" + ("" if mk == STRUCTURES[bpr] else f"-K{mk}") for bpr, n, S, mk in grid()]


def irec_coder(model, message):
    from irec.io import ArithmeticCoder
    return "".join(ArithmeticCoder(np.asarray(model, dtype=np.int64), precision=32).encode(np.asarray(message, dtype=np.int64)))


def stream_of(values, n_values, weight, coder=irec_coder):
    """One stream: the model [1, 1 + weight, ...] over n_values values, the message values + 1 and the terminator 0, the leading '1'."""
    model = np.array([1] + [1 + weight] * n_values, dtype=np.int64)
    code = "1" + coder(model, np.append(np.asarray(values, dtype=np.int64) + 1, 0))
    return int(code, 2).to_bytes((len(code) + 7) // 8, "big")


def segments_of(bpr, g):
    """[(r, first row, blocks)] of an image's segments in directory order."""
    first = np.concatenate([[0], np.cumsum(bpr)])
    return [(r, int(first[r]) + j, min(g, b - j)) for r, b in enumerate(bpr) for j in range(0, b, g)]


def file_of(K, idx, bpr, g, max_index, coder=irec_coder, seed=SEED, shape=SHAPE, block_size=BLOCK_SIZE):
    """The segmented file of one image's rows K [T], idx [T, max_K]."""
    h, w, c = shape
    head = struct.pack("<4sHHIIIIIHHHHI", b"IRSG", 1, 0, seed, block_size, max_index, h, w, c, 0, 0, len(bpr), g) + struct.pack(f"<{len(bpr)}I", *bpr)
    directory, streams = [], []
    for _r, row, nb in segments_of(bpr, g):
        ks = [int(k) for k in K[row:row + nb]]
        counts = stream_of(ks, max(ks) + 1, 100, coder)
        indices = stream_of([int(v) for j, k in enumerate(ks) for v in idx[row + j, :k]], max_index, 1000, coder)
        directory.append(struct.pack("<III", max(ks), len(counts), len(indices)))
        streams += [counts, indices]
    return head + b"".join(directory) + b"".join(streams)


def rows_of(rng, bpr, mk, n, S, g):
    """K [n, T], idx [n, T, mk]: any K in [0, mk], then -- where the call has the rows for it -- the first segment of the last residual block
    all K = 0 (an index stream of the terminator alone), one K = 0 row and one K = max_K row elsewhere."""
    T = sum(bpr)
    K = rng.integers(0, mk + 1, (n, T)).astype(np.int32)
    idx = rng.integers(0, S, (n, T, mk)).astype(np.int32)
    if n == 0:
        return K, idx
    r, row, nb = [s for s in segments_of(bpr, g) if s[0] == len(bpr) - 1][0]
    free = np.ones((n, T), dtype=bool)
    if n * T > nb + 1:
        K[0, row:row + nb] = 0
        free[0, row:row + nb] = False
    at = rng.permutation(np.flatnonzero(free.reshape(-1)))
    K.reshape(-1)[at[0]] = mk
    if at.size >= 2:
        K.reshape(-1)[at[1]] = 0
    return K, idx


@functools.lru_cache(maxsize=None)
def case(which, g):
    """Case `which` of case_names() at segment size g with its expected files, read-only."""
    bpr, n, S, mk = grid()[which]
    K, idx = rows_of(np.random.default_rng(20260000 + 97 * which + g), bpr, mk, n, S, g)
    files = [file_of(K[i], idx[i], bpr, g, S) for i in range(n)]
    c = {"name": case_names()[which], "bpr": bpr, "g": g, "max_index": S, "K": K, "idx": idx, "files": files,
         "blob": np.frombuffer(b"".join(files), dtype=np.uint8),
         "offsets": np.concatenate([[0], np.cumsum([len(f) for f in files])]).astype(np.int64),
         "idx_zeroed": np.where(np.arange(mk)[None, None, :] < K[..., None], idx, 0).astype(np.int32)}
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def first_allowance(n, bpr, g, mk):
    return n * (40 + 4 * len(bpr) + len(segments_of(bpr, g)) * 40 + 5 * sum(bpr) * (1 + mk)) + 64


def core_encode(K, idx, max_index, bpr, g, cap=None, strided=False, seed=SEED, shape=SHAPE, block_size=BLOCK_SIZE, expect=0):
    """irec_rec_test_core_encode_files_segmented: (out uint8 [cap + 8] pre-filled with 0xAB, offsets, status), all pre-filled so that an
    untouched output shows."""
    from irec import _lib
    lib = _lib.load()
    n, mk = K.shape[0], idx.shape[2]
    bpr_a = np.asarray(bpr, dtype=np.int32)
    if strided:
        both = RC.joined(K, idx)
        k_ptr, ks, i_ptr, ist = both.ctypes.data, 1 + mk, both.ctypes.data + 4, 1 + mk
    else:
        K, idx = np.ascontiguousarray(K, dtype=np.int32), np.ascontiguousarray(idx, dtype=np.int32)
        k_ptr, ks, i_ptr, ist = K.ctypes.data, 1, idx.ctypes.data, mk
    cap = first_allowance(n, [int(b) for b in bpr if b > 0], max(g, 1), mk) if cap is None else cap
    out = np.full(cap + 8, 0xAB, dtype=np.uint8)
    offsets, status = np.full(n + 1, -1, dtype=np.int64), np.full(n, -1, dtype=np.int32)
    st = lib.irec_rec_test_core_encode_files_segmented(seed, block_size, max_index, *shape, n, bpr_a.size, bpr_a.ctypes.data, g, mk, k_ptr, ks, i_ptr, ist,
                                                       out.ctypes.data, cap, offsets.ctypes.data, status.ctypes.data)
    assert st == expect, lib.irec_last_error()
    return out, offsets, status


def core_decode(blob, offsets, bpr, g, mk, expect=0):
    """irec_rec_test_core_decode_files_segmented: (headers uint32 [N, 9], K [N, T], idx [N, T, mk], status), outputs pre-filled with -1."""
    from irec import _lib
    lib = _lib.load()
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    if blob.size == 0:
        blob = np.zeros(1, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    n, T = offsets.size - 1, int(sum(b for b in bpr if b > 0))
    bpr_a = np.asarray(bpr, dtype=np.int32)
    hdr = np.full((n, 9), 0xFFFFFFFF, dtype=np.uint32)
    K = np.full((n, T), -1, dtype=np.int32)
    idx = np.full((n, T, max(mk, 1)), -1, dtype=np.int32)
    status = np.full(n, -1, dtype=np.int32)
    st = lib.irec_rec_test_core_decode_files_segmented(blob.ctypes.data, offsets.ctypes.data, n, bpr_a.size, bpr_a.ctypes.data, g, mk, hdr.ctypes.data,
                                                       K.ctypes.data, idx.ctypes.data, status.ctypes.data)
    assert st == expect, lib.irec_last_error()
    return hdr, K, idx[..., :mk] if mk else idx[..., :0], status


def host_decode(blob, offsets, bpr, g, mk, n_threads=16):
    """irec_rec_decode_files_segmented on host threads: (headers, K, idx, status)."""
    from irec.io import segmented as SG
    return SG._decode_files_segmented_status(blob, offsets, bpr, g, mk, n_threads)


# ---- the damaged set -------------------------------------------------------------------------------------------------------------------------
DAMAGED_BPR, DAMAGED_G, DAMAGED_MAX_K, DAMAGED_MAX_INDEX = (3, 1, 9), 4, 29, 36
N_RANDOM = RC.N_RANDOM


def _with(data, at, fmt, value):
    b = bytearray(data)
    b[at:at + struct.calcsize(fmt)] = struct.pack(fmt, value)
    return bytes(b)


@functools.lru_cache(maxsize=None)
def damaged_set():
    """One valid file of structure (3, 1, 9), g = 4 (five segments, the last of one block), max_K = 29, max_index = 36 and, as ONE blob in
    which every file's neighbours are other files: the named damages below, each with the status the format's rules give it, then the
    files whose verdict the rules leave open (the readers must agree with one another): damages that turn a stream into another bit
    string, and N_RANDOM copies with one to three random bytes replaced as rec_ragged_cases.damaged_set makes them.  Valid copies stand between the groups, so that every damaged file has an intact
    neighbour."""
    rng = np.random.default_rng(12)
    bpr, g, mk, S = DAMAGED_BPR, DAMAGED_G, DAMAGED_MAX_K, DAMAGED_MAX_INDEX
    T, R = sum(bpr), len(bpr)
    K0 = rng.integers(0, mk + 1, (1, T)).astype(np.int32)
    K0[0, 4] = mk                                              # (a max_part word equal to max_K, so that a max_K one lower refuses the file)
    idx0 = rng.integers(0, S, (1, T, mk)).astype(np.int32)
    data = file_of(K0[0], idx0[0], bpr, g, S)
    idx0 = np.where(np.arange(mk)[None, None, :] < K0[..., None], idx0, 0).astype(np.int32)
    n_seg = len(segments_of(bpr, g))
    d0 = 40 + 4 * R                                            # the directory
    s0 = d0 + 12 * n_seg                                       # the first stream
    entries = np.frombuffer(data[d0:s0], dtype="<u4").reshape(n_seg, 3)
    named = [("valid", data, 0)]
    named += [(f"truncated_header_{n}", data[:n], 4) for n in (0, 3, 39)]
    named += [(f"truncated_blocks_{n}", data[:n], 4) for n in (40, d0 - 1)]
    named += [(f"truncated_directory_{n}", data[:n], 4) for n in (d0, d0 + 13, s0 - 1)]
    named += [(f"truncated_stream_{n}", data[:n], E_SEG_DIRECTORY) for n in (s0, s0 + 1, len(data) - 1)]
    named += [("one_byte_more", data + b"\x00", E_SEG_DIRECTORY)]
    for s in (0, n_seg - 1):
        for word, what in ((1, "count"), (2, "index")):
            at = d0 + 12 * s + 4 * word
            named += [(f"entry_{s}_{what}_bytes_plus_1", _with(data, at, "<I", int(entries[s, word]) + 1), E_SEG_DIRECTORY),
                      (f"entry_{s}_{what}_bytes_minus_1", _with(data, at, "<I", int(entries[s, word]) - 1), E_SEG_DIRECTORY)]
    named += [("magic", _with(data, 0, "<4s", b"IRSH"), E_SEG_MAGIC), ("magic_plain_seed", _with(data, 0, "<I", 42), E_SEG_MAGIC),
              ("version_2", _with(data, 4, "<H", 2), E_SEG_MAGIC), ("version_0", _with(data, 4, "<H", 0), E_SEG_MAGIC),
              ("reserved", _with(data, 6, "<H", 1), E_SEG_MAGIC)]
    named += [("count_flag", _with(data, 30, "<H", 1), 5), ("index_flag", _with(data, 32, "<H", 1), 5)]
    named += [("g_0", _with(data, 36, "<I", 0), E_SEG_BLOCKS), ("g_other", _with(data, 36, "<I", 2), E_SEG_BLOCKS),
              ("g_huge", _with(data, 36, "<I", 0xFFFFFFFF), E_SEG_BLOCKS)]
    named += [("R_other", _with(data, 34, "<H", 2), 17), ("blocks_other", _with(data, 40 + 8, "<I", 8), 17),
              ("max_index_0", _with(data, 16, "<I", 0), 6), ("max_index_huge", _with(data, 16, "<I", 1 << 25), 6)]
    named += [("max_part_above_max_K", _with(data, d0 + 12, "<I", mk + 1), 18), ("max_part_above_limit", _with(data, d0, "<I", 65537), 7),
              ("max_part_huge", _with(data, d0 + 24, "<I", 0xFFFFFFFF), 7)]
    open_verdict = [("entry_0_bytes_moved", _with(_with(data, d0 + 4, "<I", int(entries[0, 1]) + 1), d0 + 8, "<I", int(entries[0, 2]) - 1)),
                    ("max_part_lower", _with(data, d0 + 24, "<I", mk - 1))]
    at = s0
    for s in range(n_seg):                                     # a stream without a marker bit: all of it zero; and its marker bit alone cleared
        for word, status in ((1, 9), (2, 13)):
            kind, n_b = "count" if word == 1 else "index", int(entries[s, word])
            b = bytearray(data)
            b[at:at + n_b] = bytes(n_b)
            named.append((f"segment_{s}_{kind}_no_marker", bytes(b), status))
            b = bytearray(data)
            k = next(k for k in range(at, at + n_b) if b[k])
            b[k] &= ~(1 << (b[k].bit_length() - 1))
            open_verdict.append((f"segment_{s}_{kind}_marker_bit", bytes(b)))
            at += n_b
    files, want, names = [], [], []
    for name, raw, status in named:
        files += [raw, data]
        want += [status, 0]
        names += [name, "valid"]
    n_named = len(files)
    for name, raw in open_verdict:
        files.append(raw)
        names.append(name)
    for _ in range(N_RANDOM):
        b = bytearray(data)
        for _ in range(int(rng.integers(1, 4))):
            b[int(rng.integers(0, len(b)))] = int(rng.integers(0, 256))
        files.append(bytes(b))
        names.append("random")
    files.append(data)
    names.append("valid")
    out = {"blob": np.frombuffer(b"".join(files), dtype=np.uint8),
           "offsets": np.concatenate([[0], np.cumsum([len(f) for f in files])]).astype(np.int64),
           "names": names, "want": want, "n_named": n_named, "K0": K0, "idx0": idx0, "data": data}
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out
