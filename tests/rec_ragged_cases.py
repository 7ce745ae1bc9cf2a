"""Shared by tests/test_rec_ragged_host.py and tests/test_rec_ragged_gpu.py: the cases of the ragged .rec coder (residual blocks of differing
sizes), their referee results -- irec_rec_encode_file / read_compressed_code of irec_io.cpp, one file per call, computed once and never
changed -- and the core's host hooks (irec_rec_test_core_*_ragged: csrc/irec_rec_core.h over host memory in a plain loop)."""
import functools
import os
import tempfile

import numpy as np

from rec_device_cases import IREC_REC_E_STRUCTURE  # noqa: F401

# blocks per residual block -> max_K: one stream pair | a short block before a longer one | three sizes | uniform (the twin of encode_files) |
# the two levels of a Kodak image
STRUCTURES = {(1,): 4, (1, 4): 7, (3, 1, 5): 12, (2, 2, 2): 3, (13, 302): 9}
N_IMAGES = (1, 3)
MAX_INDEX = (1, 20, 36)
SEED, SHAPE, BLOCK_SIZE = 42, (32, 48, 3), 1000


def case_names():
    return [f"{'_'.join(map(str, bpr))}-N{n}-S{S}" for bpr in STRUCTURES for n in N_IMAGES for S in MAX_INDEX]


def lists_of(K, idx, bpr):
    """block_indices of every image, as write_compressed_code takes them: [image][residual block][block] -> list of indices."""
    first = np.concatenate([[0], np.cumsum(bpr)])
    return [[[idx[i, b, :K[i, b]].tolist() for b in range(first[r], first[r + 1])] for r in range(len(bpr))] for i in range(K.shape[0])]


def file_of(lists, max_index, seed=SEED, shape=SHAPE, block_size=BLOCK_SIZE):
    """irec_rec_encode_file on one image's lists."""
    from irec.io import utils as U
    return U._native_encode(seed, shape, block_size, lists, max_index)


@functools.lru_cache(maxsize=None)
def cases():
    """Every case with its referee result, read-only: files (irec_rec_encode_file per image), blob / offsets (their concatenation)."""
    rng = np.random.default_rng(20250301)
    out = []
    for bpr, mk in STRUCTURES.items():
        T = sum(bpr)
        for n in N_IMAGES:
            for S in MAX_INDEX:
                K = rng.integers(0, mk + 1, (n, T)).astype(np.int32)
                flat = K.reshape(-1)
                if flat.size >= 2:
                    at = rng.choice(flat.size, 2, replace=False)
                    flat[at[0]], flat[at[1]] = 0, mk                  # at least one K = 0 row and one K = max_K row per call
                else:
                    flat[0] = mk                                      # (a call of one row cannot hold both)
                idx = rng.integers(0, S, (n, T, mk)).astype(np.int32)
                files = [file_of(l, S) for l in lists_of(K, idx, bpr)]
                c = {"name": f"{'_'.join(map(str, bpr))}-N{n}-S{S}", "bpr": bpr, "max_index": S, "K": K, "idx": idx, "files": files,
                     "blob": np.frombuffer(b"".join(files), dtype=np.uint8),
                     "offsets": np.concatenate([[0], np.cumsum([len(f) for f in files])]).astype(np.int64),
                     "idx_zeroed": np.where(np.arange(mk)[None, None, :] < K[..., None], idx, 0).astype(np.int32)}
                for a in c.values():
                    if isinstance(a, np.ndarray):
                        a.setflags(write=False)
                out.append(c)
    assert [c["name"] for c in out] == case_names()
    return tuple(out)


def read_file(raw):
    """read_compressed_code on one file's bytes: (seed, image_shape, block_size, block_indices)."""
    from irec.io import utils as U
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "f.rec")
        with open(path, "wb") as fh:
            fh.write(raw)
        return U.read_compressed_code(path)


def first_allowance(n, bpr, mk):
    """irec_io.cpp's own first allowance: 64 + 40 bits per symbol and terminator, per stream."""
    return n * (28 + 16 * len(bpr) + sum((64 + 40 * (b + 1)) // 8 + 1 + (64 + 40 * (b * mk + 1)) // 8 + 1 for b in bpr))


def joined(K, idx):
    """One [rows][1 + width] tensor, K in column 0 (what PendingCode.gather_packed_ragged builds on the device)."""
    return np.ascontiguousarray(np.concatenate([K.reshape(-1, 1), idx.reshape(K.size, idx.shape[-1])], axis=1).astype(np.int32))


def core_encode(K, idx, max_index, bpr, cap=None, strided=False, seed=SEED, shape=SHAPE, block_size=BLOCK_SIZE, expect=0):
    """irec_rec_test_core_encode_files_ragged: (out uint8 [cap + 8] pre-filled with 0xAB, offsets, status), all pre-filled so that an
    untouched output shows."""
    from irec import _lib
    lib = _lib.load()
    n, mk = K.shape[0], idx.shape[2]
    bpr_a = np.asarray(bpr, dtype=np.int32)
    if strided:
        both = joined(K, idx)
        k_ptr, ks, i_ptr, ist = both.ctypes.data, 1 + mk, both.ctypes.data + 4, 1 + mk
    else:
        K, idx = np.ascontiguousarray(K, dtype=np.int32), np.ascontiguousarray(idx, dtype=np.int32)
        k_ptr, ks, i_ptr, ist = K.ctypes.data, 1, idx.ctypes.data, mk
    cap = first_allowance(n, [int(b) for b in bpr if b > 0], mk) if cap is None else cap
    out = np.full(cap + 8, 0xAB, dtype=np.uint8)
    offsets, status = np.full(n + 1, -1, dtype=np.int64), np.full(n, -1, dtype=np.int32)
    st = lib.irec_rec_test_core_encode_files_ragged(seed, block_size, max_index, *shape, n, bpr_a.size, bpr_a.ctypes.data, mk, k_ptr, ks, i_ptr, ist,
                                                    out.ctypes.data, cap, offsets.ctypes.data, status.ctypes.data)
    assert st == expect, lib.irec_last_error()
    return out, offsets, status


def core_decode(blob, offsets, bpr, mk, expect=0):
    """irec_rec_test_core_decode_files_ragged: (headers uint32 [N, 9], K [N, T], idx [N, T, mk], status), outputs pre-filled with -1."""
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
    st = lib.irec_rec_test_core_decode_files_ragged(blob.ctypes.data, offsets.ctypes.data, n, bpr_a.size, bpr_a.ctypes.data, mk, hdr.ctypes.data,
                                                    K.ctypes.data, idx.ctypes.data, status.ctypes.data)
    assert st == expect, lib.irec_last_error()
    return hdr, K, idx[..., :mk] if mk else idx[..., :0], status


DAMAGED_BPR, DAMAGED_MAX_K = (3, 1, 9), 29
N_RANDOM = 300   # copies of the damaged set with one to three random bytes replaced


@functools.lru_cache(maxsize=None)
def damaged_set():
    """One container of structure (3, 1, 9), max_K = 29, max_index = 36 and, as ONE blob in which every file's neighbours are other files
    (a read past a file's own range finds their bytes and changes a verdict): every prefix, N_RANDOM copies with one to three random bytes
    replaced, 100 copies with a byte of the seed / block-size / height / width / channel fields replaced, 300 copies with a byte of the
    dynamic header or the count streams replaced, and the same rows written as (3, 9, 1), (1, 3, 9) and (13,).  With the host reader's verdict on every file (irec_rec_decode_files_ragged, one file per call): ok and,
    where it accepts, headers / K / idx."""
    from irec.io import utils as U
    rng = np.random.default_rng(12)
    bpr, mk = DAMAGED_BPR, DAMAGED_MAX_K
    T = sum(bpr)
    K0 = rng.integers(0, mk + 1, (1, T)).astype(np.int32)
    idx0 = rng.integers(0, 36, (1, T, mk)).astype(np.int32)
    data = file_of(lists_of(K0, idx0, bpr)[0], 36)
    idx0 = np.where(np.arange(mk)[None, None, :] < K0[..., None], idx0, 0).astype(np.int32)
    files = [data[:n] for n in range(len(data))]
    for _ in range(N_RANDOM):
        b = bytearray(data)
        for _ in range(int(rng.integers(1, 4))):
            b[int(rng.integers(0, len(b)))] = int(rng.integers(0, 256))
        files.append(bytes(b))
    fields = list(range(0, 8)) + list(range(12, 22))
    for _ in range(100):
        b = bytearray(data)
        b[fields[int(rng.integers(0, len(fields)))]] = int(rng.integers(0, 256))
        files.append(bytes(b))
    R = len(bpr)
    counts_hi = 28 + 16 * R + int(np.frombuffer(data[28 + 4 * R:28 + 8 * R], dtype="<u4").sum())
    for _ in range(300):                                       # the count streams and their header words are a few bytes of the file: damage aimed at them
        b = bytearray(data)
        b[int(rng.integers(28, counts_hi))] = int(rng.integers(0, 256))
        files.append(bytes(b))
    n_same = len(files)
    for other in ((3, 9, 1), (1, 3, 9), (13,)):
        files.append(file_of(lists_of(K0, idx0, other)[0], 36))
    offsets = np.concatenate([[0], np.cumsum([len(f) for f in files])]).astype(np.int64)
    blob = np.frombuffer(b"".join(files), dtype=np.uint8)
    ok = np.zeros(len(files), dtype=bool)
    hdr = np.zeros((len(files), 9), dtype=np.uint32)
    K = np.zeros((len(files), T), dtype=np.int32)
    idx = np.zeros((len(files), T, mk), dtype=np.int32)
    for f, raw in enumerate(files):
        try:
            h, k, ix = U.decode_files_ragged(np.frombuffer(raw, dtype=np.uint8) if raw else np.zeros(1, np.uint8), np.array([0, len(raw)]), bpr, mk,
                                             n_threads=1)
        except ValueError:
            continue
        ok[f], hdr[f], K[f], idx[f] = True, h[0], k[0], ix[0]
    out = {"blob": blob, "offsets": offsets, "ok": ok, "hdr": hdr, "K": K, "idx": idx, "K0": K0, "idx0": idx0, "n_prefix": len(data),
           "n_same": n_same}
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


class StubCoder:
    """What PendingCode's checks read of a coder, for calls built by hand on host tensors."""
    _split_strikes, extrapolate_auxiliary_ratios = 0, True

    def __init__(self):
        self._max_K_hint, self._K_seen, self._K_reads = 0, 0, 0
