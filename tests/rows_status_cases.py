"""The case list of the row check (irec_decode_rows_status, csrc/irec_rows_core.h), shared by tests/test_rows_status_host.py (host twin
against a numpy referee) and tests/test_decompress_device_gpu.py (device against the host twin).

Every combination of bpg in {1, 3, 9}, max_K in {1, 5, 70}, n_groups in {1, 3, 65}, packed / joined strides, identity / shuffled
block_row and min_K in {0, 1}; group g of combination c carries plant (c + g) mod N_PLANTS, so that every plant also meets the
one-group calls.  A case holds the LOGICAL rows (K [rows], idx [rows, max_K]); `buffers` lays them out at their exact size, so that a
read past idx[b * idx_stride + max_K - 1] leaves the allocation."""
import ctypes
import functools
import itertools

import numpy as np

S = 36
INT32_MAX = 2 ** 31 - 1
OK, K_RANGE, INDEX_RANGE, RATIO_TABLE = 0, 1, 2, 3
BAD_INDEX = (-1, S, INT32_MAX)
# (name, ...): what a group's planted block(s) hold
PLANTS = (["none", "K=0", "K=max_K", "K=max_K+1", "K=-1", "K=int32max"] +
          [f"idx{v}@{pos}" for pos in ("0", "K-1", "K") for v in BAD_INDEX] +
          ["two:index-then-K", "two:K-then-index", "preset", "K>k_limit"])
N_PLANTS = len(PLANTS)


def _plant(rng, name, Kg, Ig, max_K, k_limit, status0, g):
    """Kg [bpg], Ig [bpg, max_K]: the group's rows (views), healthy on entry."""
    bpg = Kg.shape[0]
    j = int(rng.integers(bpg))
    if name == "K=0":
        Kg[j] = 0
    elif name == "K=max_K":
        Kg[j] = min(max_K, k_limit)
    elif name == "K=max_K+1":
        Kg[j] = max_K + 1
    elif name == "K=-1":
        Kg[j] = -1
    elif name == "K=int32max":
        Kg[j] = INT32_MAX
    elif name.startswith("idx"):
        v, pos = name[3:].split("@")
        if pos == "0":
            Kg[j] = max(1, Kg[j]); Ig[j, 0] = int(v)
        elif pos == "K-1":
            Kg[j] = max(1, Kg[j]); Ig[j, Kg[j] - 1] = int(v)
        else:                                      # position K: past the row's end, must not count
            Kg[j] = min(Kg[j], max_K - 1); Ig[j, Kg[j]] = int(v)
    elif name.startswith("two") and bpg >= 2:
        lo, hi = sorted(rng.choice(bpg, size=2, replace=False).tolist())
        first_index = name == "two:index-then-K"
        a, b = (lo, hi) if first_index else (hi, lo)
        Kg[a] = max(1, Kg[a]); Ig[a, int(rng.integers(Kg[a]))] = S      # an index out of range in block a
        Kg[b] = max_K + 1                                                # a count out of range in block b
    elif name == "preset":
        status0[g] = 7
        Kg[j] = -5
    elif name == "K>k_limit" and k_limit < max_K:
        Kg[j] = k_limit + 1


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    grid = itertools.product((1, 3, 9), (1, 5, 70), (1, 3, 65), ("packed", "joined"), (False, True), (0, 1))
    for c, (bpg, max_K, n_groups, form, shuffled, min_K) in enumerate(grid):
        rng = np.random.default_rng(1000 + c)
        rows = n_groups * bpg
        k_limit = max(1, max_K - 2) if (max_K >= 5 and c % 3 == 0) else INT32_MAX
        K = rng.integers(min_K, min(max_K, k_limit) + 1, size=rows).astype(np.int32)
        idx = rng.integers(0, S, size=(rows, max_K)).astype(np.int32)
        block_row = rng.permutation(rows).astype(np.int32) if shuffled else None
        status0 = np.zeros(n_groups, dtype=np.int32)
        for g in range(n_groups):
            at = np.arange(g * bpg, (g + 1) * bpg)
            b = block_row[at] if shuffled else at
            Kg, Ig = K[b], idx[b]                  # (copies: fancy indexing)
            _plant(rng, PLANTS[(c + g) % N_PLANTS], Kg, Ig, max_K, k_limit, status0, g)
            K[b], idx[b] = Kg, Ig
        for a in (K, idx, status0):
            a.setflags(write=False)
        out.append({"name": f"bpg{bpg}-mK{max_K}-g{n_groups}-{form}-{'shuf' if shuffled else 'id'}-min{min_K}", "bpg": bpg, "max_K": max_K,
                    "n_groups": n_groups, "form": form, "block_row": block_row, "min_K": min_K, "k_limit": k_limit, "K": K, "idx": idx,
                    "status0": status0, "plants": [PLANTS[(c + g) % N_PLANTS] for g in range(n_groups)]})
    return out


def buffers(case):
    """(base int32 array of EXACTLY the bytes the call may read, K offset, k_stride, idx offset, idx_stride), offsets in elements."""
    K, idx, max_K = case["K"], case["idx"], case["max_K"]
    rows = K.shape[0]
    if case["form"] == "joined":                   # one [rows][1 + max_K] tensor, K in column 0
        return np.ascontiguousarray(np.concatenate([K[:, None], idx], axis=1)).reshape(-1), 0, 1 + max_K, 1, 1 + max_K
    return np.concatenate([K, idx.reshape(-1)]), 0, 1, rows, max_K      # K [rows], then idx [rows][max_K] to its last element


def host_status(lib, case):
    """irec_test_rows_status_host on the case: status int32 [n_groups]."""
    base, k_at, ks, i_at, ist = buffers(case)
    base = base.copy()
    status = case["status0"].copy()
    br = case["block_row"]
    st = lib.irec_test_rows_status_host(case["n_groups"], case["bpg"], br.ctypes.data if br is not None else None,
                                        base.ctypes.data + 4 * k_at, ks, base.ctypes.data + 4 * i_at, ist, case["max_K"], case["min_K"],
                                        case["k_limit"], S, status.ctypes.data)
    assert st == 0, lib.irec_last_error()
    return status


def device_status(lib, case, torch):
    """irec_decode_rows_status on the case (current stream): status int32 [n_groups] (numpy, after one read-back)."""
    base, k_at, ks, i_at, ist = buffers(case)
    dev = torch.from_numpy(base.copy()).cuda()
    status = torch.from_numpy(case["status0"].copy()).cuda()
    br = torch.from_numpy(case["block_row"].copy()).cuda() if case["block_row"] is not None else None
    st = lib.irec_decode_rows_status(case["n_groups"], case["bpg"], br.data_ptr() if br is not None else None, dev.data_ptr() + 4 * k_at, ks,
                                     dev.data_ptr() + 4 * i_at, ist, case["max_K"], case["min_K"], case["k_limit"], S, status.data_ptr(),
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == 0, lib.irec_last_error()
    return status.cpu().numpy()
