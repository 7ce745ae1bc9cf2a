"""Shared by tests/test_rec_device_host.py and tests/test_rec_device_gpu.py: the cases of the device .rec coder, their referee results
(irec_rec_encode_files / irec_rec_decode_files of irec_io.cpp and the golden files, computed once and never changed), and the core's
host hooks (irec_rec_test_core_*: csrc/irec_rec_core.h over host memory in a plain loop)."""
import functools
import os

import numpy as np

from conftest import GOLDEN_DIR

IREC_REC_E_STRUCTURE = 17

# (N, R, bpt, max_K, max_index): fewer streams than a wave | ragged K with 0, stream byte counts of six residues mod 8 | a residual block
# whose counts are all zero (model [1, 101], 64 blocks in two bytes) | near-deterministic model, long pending run | R just under 2^30,
# products near 2^62 | more images than any workgroup is wide
SHAPES = [(3, 1, 1, 4, 20), (9, 5, 9, 12, 36), (2, 2, 64, 2, 36), (2, 1, 3, 300, 1), (2, 2, 5, 6, 1 << 20), (1500, 1, 1, 2, 36)]


def _golden_repacks():
    """The golden containers of rec_files.npz (written by the real reference) in the packed form.  Both are ragged -- 9, 9, 4 and 13, 5, 1
    coded blocks per residual block -- and the packed form holds one block count per call, so each residual block is its own one-block
    case.  Its expected file is cut from the golden bytes alone: the static header with R = 1, the block's four dynamic-header words, its
    count stream and its index stream, exactly as the reference wrote them."""
    g = np.load(os.path.join(GOLDEN_DIR, "rec_files.npz"))
    out = []
    for name in g["names"]:
        seed, bs, max_index, h, w, c = (int(v) for v in g[f"{name}_meta"])
        flat, lens, nblocks = g[f"{name}_flat"], g[f"{name}_lens"], [int(v) for v in g[f"{name}_nblocks"]]
        raw = g[f"{name}_bytes"].tobytes()
        R = len(nblocks)
        dyn = np.frombuffer(raw[28:28 + 16 * R], dtype="<u4").reshape(4, R)
        assert dyn[0].tolist() == nblocks and 28 + 16 * R + int(dyn[1].sum() + dyn[2].sum()) == len(raw)
        c_at = [28 + 16 * R + int(dyn[1, :q].sum()) for q in range(R + 1)]
        x_at = [c_at[-1] + int(dyn[2, :q].sum()) for q in range(R + 1)]
        blk = pos = 0
        for r, bpt in enumerate(nblocks):
            ks = lens[blk:blk + bpt].astype(np.int32)
            mk = max(int(ks.max()), 1)
            idx = np.zeros((1, 1, bpt, mk), dtype=np.int32)
            for j, k in enumerate(ks):
                idx[0, 0, j, :k] = flat[pos:pos + k]
                pos += int(k)
            blk += bpt
            want = raw[:26] + (1).to_bytes(2, "little") + dyn[:, r].astype("<u4").tobytes() + raw[c_at[r]:c_at[r + 1]] + raw[x_at[r]:x_at[r + 1]]
            out.append({"name": f"golden_{name}_r{r}", "seed": seed, "shape": (h, w, c), "block_size": bs, "max_index": max_index,
                        "K": ks.reshape(1, 1, bpt).copy(), "idx": idx, "golden": [want]})
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """Every case with its referee result: blob / offsets of irec_rec_encode_files, read-only."""
    from irec.io import utils as U
    rng = np.random.default_rng(20240611)
    out = []
    for n, R, bpt, mk, S in SHAPES:
        K = rng.integers(0, mk + 1, (n, R, bpt)).astype(np.int32)
        if bpt == 64:
            K[:, 1, :] = 0
        idx = rng.integers(0, S, (n, R, bpt, mk)).astype(np.int32)
        out.append({"name": f"{n}x{R}x{bpt}x{mk}_S{S}", "seed": 42, "shape": (32, 32, 3), "block_size": 1000, "max_index": S, "K": K, "idx": idx,
                    "golden": None})
    out += _golden_repacks()
    assert [c["name"] for c in out] == case_names()
    for c in out:
        c["blob"], c["offsets"] = U.encode_files(c["seed"], c["shape"], c["block_size"], c["K"], c["idx"], c["max_index"])
        live = np.arange(c["idx"].shape[3])[None, None, None, :] < c["K"][..., None]
        c["idx_zeroed"] = np.where(live, c["idx"], 0).astype(np.int32)
        for a in (c["K"], c["idx"], c["blob"], c["offsets"], c["idx_zeroed"]):
            a.setflags(write=False)
    return tuple(out)


def case_names():
    return [f"{n}x{R}x{bpt}x{mk}_S{S}" for n, R, bpt, mk, S in SHAPES] + [f"golden_{name}_r{r}" for name in ("rvae", "ragged") for r in range(3)]


def first_allowance(n, R, bpt, mk):
    """irec_io.cpp's own first allowance: 64 + 40 bits per symbol and terminator, per stream."""
    return n * (28 + 16 * R + R * ((64 + 40 * (bpt + 1)) // 8 + 1 + (64 + 40 * (bpt * mk + 1)) // 8 + 1))


def joined(K, idx):
    """One [rows][1 + width] tensor, K in column 0 (what PendingCode.gather_packed builds on the device)."""
    n, R, bpt = K.shape
    return np.ascontiguousarray(np.concatenate([K.reshape(-1, 1), idx.reshape(n * R * bpt, -1)], axis=1).astype(np.int32))


def core_encode(seed, shape, block_size, K, idx, max_index, cap=None, strided=False):
    """irec_rec_test_core_encode_files: (out uint8 [cap + 8] pre-filled with 0xAB, offsets, status)."""
    from irec import _lib
    lib = _lib.load()
    n, R, bpt = K.shape
    mk = idx.shape[3]
    if strided:
        both = joined(K, idx)
        k_ptr, ks, i_ptr, ist = both.ctypes.data, 1 + mk, both.ctypes.data + 4, 1 + mk
    else:
        K, idx = np.ascontiguousarray(K, dtype=np.int32), np.ascontiguousarray(idx, dtype=np.int32)
        k_ptr, ks, i_ptr, ist = K.ctypes.data, 1, idx.ctypes.data, mk
    cap = first_allowance(n, R, bpt, mk) if cap is None else cap
    out = np.full(cap + 8, 0xAB, dtype=np.uint8)
    offsets, status = np.full(n + 1, -1, dtype=np.int64), np.full(n, -1, dtype=np.int32)
    st = lib.irec_rec_test_core_encode_files(seed, block_size, max_index, *shape, n, R, bpt, mk, k_ptr, ks, i_ptr, ist, out.ctypes.data, cap,
                                             offsets.ctypes.data, status.ctypes.data)
    assert st == 0, lib.irec_last_error()
    return out, offsets, status


def core_decode(blob, offsets, R, bpt, mk):
    """irec_rec_test_core_decode_files: (headers uint32 [N, 9], K, idx, status), outputs pre-filled with -1."""
    from irec import _lib
    lib = _lib.load()
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    if blob.size == 0:
        blob = np.zeros(1, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    n = offsets.size - 1
    hdr = np.full((n, 9), 0xFFFFFFFF, dtype=np.uint32)
    K = np.full((n, R, bpt), -1, dtype=np.int32)
    idx = np.full((n, R, bpt, max(mk, 1)), -1, dtype=np.int32)
    status = np.full(n, -1, dtype=np.int32)
    st = lib.irec_rec_test_core_decode_files(blob.ctypes.data, offsets.ctypes.data, n, R, bpt, mk, hdr.ctypes.data, K.ctypes.data, idx.ctypes.data,
                                             status.ctypes.data)
    assert st == 0, lib.irec_last_error()
    return hdr, K, idx[..., :mk] if mk else idx[..., :0], status


DAMAGED_SHAPE = (6, 9, 29)   # R, bpt, max_K of the damaged container


@functools.lru_cache(maxsize=None)
def damaged_set():
    """The 746-byte container of R = 6, bpt = 9, max_K = 29, max_index = 36 (default_rng(11)) and, as ONE blob of 1746 files: every prefix,
    800 copies with one to three random bytes replaced, 200 copies with one byte replaced inside the seed, block-size, height, width and
    channel fields.  With the host reader's verdict on every file (irec_rec_decode_files, one file per call): ok [1746] and, where it
    accepts, headers / K / idx."""
    from irec.io import utils as U
    rng = np.random.default_rng(11)
    R, bpt, mk = DAMAGED_SHAPE
    K0 = rng.integers(0, mk + 1, (R, bpt)).astype(np.int32)
    idx0 = rng.integers(0, 36, (R, bpt, mk)).astype(np.int32)
    blob0, _ = U.encode_files(42, (32, 32, 3), 1000, K0[None], idx0[None], 36)
    data = blob0.tobytes()
    assert len(data) == 746
    idx0 = np.where(np.arange(mk)[None, None, :] < K0[..., None], idx0, 0).astype(np.int32)
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
    sizes = np.array([len(f) for f in files], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    blob = np.frombuffer(b"".join(files), dtype=np.uint8)
    ok = np.zeros(len(files), dtype=bool)
    hdr = np.zeros((len(files), 9), dtype=np.uint32)
    K = np.zeros((len(files), R, bpt), dtype=np.int32)
    idx = np.zeros((len(files), R, bpt, mk), dtype=np.int32)
    for f, raw in enumerate(files):
        try:
            h, k, ix = U.decode_files(np.frombuffer(raw, dtype=np.uint8) if raw else np.zeros(1, np.uint8), np.array([0, len(raw)]), R, bpt, mk, n_threads=1)
        except ValueError:
            continue
        ok[f], hdr[f], K[f], idx[f] = True, h[0], k[0], ix[0]
    out = {"blob": blob, "offsets": offsets, "ok": ok, "hdr": hdr, "K": K, "idx": idx, "K0": K0, "idx0": idx0, "n_prefix": len(data)}
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out
