"""CPU tests of the ragged .rec coder: residual blocks of differing sizes through the host-thread coder (irec_rec_encode_files_ragged /
irec_rec_decode_files_ragged) and through the device core's host hooks (irec_rec_test_core_*_ragged: the lane functions of the kernels
over host memory in a plain loop).  The referees are the per-file coder of irec_io.cpp (irec_rec_encode_file, read_compressed_code),
which is byte-identical to the compiled reference (tests/test_rec_io.py), and the Python glue _write_compressed_code_py, which shares no
container code with either.  Every comparison is byte or integer equality."""
import numpy as np
import pytest

import rec_device_cases as U0
import rec_ragged_cases as C

pytestmark = [pytest.mark.both_suites, pytest.mark.usefixtures("suite")]

CASES = range(len(C.case_names()))


@pytest.mark.parametrize("which", CASES, ids=C.case_names())
def test_host_files_equal_the_per_file_coder_and_the_python_glue(which, tmp_path):
    from irec.io import utils as U
    c = C.cases()[which]
    blob, off = U.encode_files_ragged(C.SEED, C.SHAPE, C.BLOCK_SIZE, c["K"], c["idx"], c["max_index"], c["bpr"])
    assert np.array_equal(off, c["offsets"]) and np.array_equal(blob, c["blob"])
    for i, lists in enumerate(C.lists_of(c["K"], c["idx"], c["bpr"])):
        path = str(tmp_path / f"py_{i}.rec")
        U._write_compressed_code_py(path, C.SEED, C.SHAPE, C.BLOCK_SIZE, lists, c["max_index"])
        with open(path, "rb") as fh:
            assert fh.read() == c["files"][i] == blob[off[i]:off[i + 1]].tobytes()
    if len(set(c["bpr"])) == 1:                                # the uniform twin: the same bytes and offsets
        n, R, bpt = c["K"].shape[0], len(c["bpr"]), c["bpr"][0]
        blob_u, off_u = U.encode_files(C.SEED, C.SHAPE, C.BLOCK_SIZE, c["K"].reshape(n, R, bpt), c["idx"].reshape(n, R, bpt, -1), c["max_index"])
        assert np.array_equal(blob_u, blob) and np.array_equal(off_u, off)


@pytest.mark.parametrize("which", CASES, ids=C.case_names())
def test_host_reader_equals_read_compressed_code(which):
    from irec.io import utils as U
    c = C.cases()[which]
    mk = c["idx"].shape[2]
    hdr, K, idx = U.decode_files_ragged(c["blob"], c["offsets"], c["bpr"], mk)
    assert np.array_equal(K, c["K"]) and np.array_equal(idx, c["idx_zeroed"])
    h, w, ch = C.SHAPE
    assert (hdr == np.array([C.SEED, C.BLOCK_SIZE, c["max_index"], h, w, ch, 0, 0, len(c["bpr"])], dtype=np.uint32)).all()
    want = C.lists_of(c["K"], c["idx"], c["bpr"])
    for i, raw in enumerate(c["files"]):
        seed, shape, bs, blocks = C.read_file(raw)
        assert (seed, tuple(shape), bs) == (C.SEED, C.SHAPE, C.BLOCK_SIZE) and blocks == want[i]
        assert blocks == C.lists_of(K[i:i + 1], idx[i:i + 1], c["bpr"])[0]
    # a wider max_K only adds zero columns
    hdr2, K2, idx2 = U.decode_files_ragged(c["blob"], c["offsets"], c["bpr"], mk + 3)
    assert np.array_equal(K2, K) and np.array_equal(idx2[..., :mk], idx) and not idx2[..., mk:].any()


@pytest.mark.parametrize("which", CASES, ids=C.case_names())
def test_core_files_equal_the_host_coder(which):
    c = C.cases()[which]
    K, idx, bpr, S = c["K"], c["idx"], c["bpr"], c["max_index"]
    mk, total = idx.shape[2], int(c["offsets"][-1])
    out, off, status = C.core_encode(K, idx, S, bpr)
    assert (status == 0).all() and np.array_equal(off, c["offsets"])
    assert np.array_equal(out[:total], c["blob"]) and (out[total:] == 0xAB).all()      # the host's bytes, and not one byte more
    out_s, off_s, status_s = C.core_encode(K, idx, S, bpr, strided=True)
    assert (status_s == 0).all() and np.array_equal(off_s, off) and np.array_equal(out_s[:total], c["blob"])
    out_c, off_c, status_c = C.core_encode(K, idx, S, bpr, cap=total - 1)              # one byte short: nothing written, sizes reported
    assert (out_c == 0xAB).all() and np.array_equal(off_c, off) and (status_c == 0).all()
    out_e, off_e, _ = C.core_encode(K, idx, S, bpr, cap=total)
    assert np.array_equal(out_e[:total], c["blob"]) and (out_e[total:] == 0xAB).all()
    hdr, K2, idx2, st = C.core_decode(c["blob"], c["offsets"], bpr, mk)
    assert (st == 0).all() and np.array_equal(K2, K) and np.array_equal(idx2, c["idx_zeroed"])
    h, w, ch = C.SHAPE
    assert (hdr == np.array([C.SEED, C.BLOCK_SIZE, S, h, w, ch, 0, 0, len(bpr)], dtype=np.uint32)).all()
    if len(set(bpr)) == 1:                                     # the uniform hooks on the same rows: the same bytes
        n, R = K.shape[0], len(bpr)
        out_u, off_u, st_u = U0.core_encode(C.SEED, C.SHAPE, C.BLOCK_SIZE, K.reshape(n, R, bpr[0]), idx.reshape(n, R, bpr[0], mk), S)
        assert (st_u == 0).all() and np.array_equal(off_u, off) and np.array_equal(out_u[:total], c["blob"])


@pytest.mark.parametrize("bpr", [(1, 4), (3, 1, 5), (13, 302)], ids=str)
def test_core_refuses_one_image_alone(bpr):
    """A K out of range or an index >= max_index in one image gives that image's status alone: the other files are unchanged and the
    refused file has no bytes."""
    from irec.io import utils as U
    c = next(c for c in C.cases() if c["bpr"] == bpr and c["K"].shape[0] == 3 and c["max_index"] == 20)
    K, idx, mk = np.array(c["K"]), np.array(c["idx"]), c["idx"].shape[2]
    first = np.concatenate([[0], np.cumsum(bpr)])
    files = c["files"]
    row = int(first[-2])                                       # the first block of the last residual block
    for image in range(3):
        bad = idx.copy()
        K1 = K.copy()
        K1[image, row] = max(K1[image, row], 1)
        bad[image, row, 0] = 20                               # an index equal to max_index, among the first K
        want = [C.file_of(l, 20) if i != image else b"" for i, l in enumerate(C.lists_of(K1, idx, bpr))]
        out, off, status = C.core_encode(K1, bad, 20, bpr)
        assert status.tolist() == [2 if i == image else 0 for i in range(3)]
        assert [out[off[i]:off[i + 1]].tobytes() for i in range(3)] == want and (out[off[3]:] == 0xAB).all()
        with pytest.raises(ValueError, match=rf"max_index.*\(image {image}\)"):
            U._raise_first_status(status)
        with pytest.raises(ValueError, match=rf"\(image {image}\)"):
            U.encode_files_ragged(C.SEED, C.SHAPE, C.BLOCK_SIZE, K1, bad, 20, bpr)
        for k_bad in (mk + 1, -1):
            Kbad = K.copy()
            Kbad[image, row] = k_bad
            out, off, status = C.core_encode(Kbad, idx, 20, bpr)
            assert status.tolist() == [1 if i == image else 0 for i in range(3)]
            assert [out[off[i]:off[i + 1]].tobytes() for i in range(3)] == [f if i != image else b"" for i, f in enumerate(files)]
            with pytest.raises(ValueError) as e:
                U.encode_files_ragged(C.SEED, C.SHAPE, C.BLOCK_SIZE, Kbad, idx, 20, bpr)
            assert str(e.value) == f"irec_rec_encode_files: K out of range (image {image})"


def test_a_file_split_differently_is_another_structure():
    from irec.io import utils as U
    rng = np.random.default_rng(5)
    K = rng.integers(0, 4, (2, 5)).astype(np.int32)
    idx = rng.integers(0, 36, (2, 5, 3)).astype(np.int32)
    blob, off = U.encode_files_ragged(1, (8, 8, 3), 10, K, idx, 36, (4, 1))
    hdr, K2, idx2, st = C.core_decode(blob, off, (4, 1), 3)
    assert (st == 0).all() and np.array_equal(K2, K)
    for other in ((1, 4), (5,), (4, 1, 1), (4, 2)):
        hdr, K2, idx2, st = C.core_decode(blob, off, other, 3)
        assert (st == C.IREC_REC_E_STRUCTURE).all(), other
        assert not hdr.any() and not K2.any() and not idx2.any()                        # zeroed outputs
        with pytest.raises(ValueError, match=r"structure differs \(image 0\)"):
            U.decode_files_ragged(blob, off, other, 3)
        with pytest.raises(ValueError, match=r"structure.*\(image 0\)"):
            U._raise_first_status(st)
    # one file of three of another structure: that image alone
    other_blob, _ = U.encode_files_ragged(1, (8, 8, 3), 10, K[:1], idx[:1], 36, (1, 4))
    files = [blob[off[0]:off[1]], other_blob, blob[off[1]:off[2]]]
    mixed, moff = np.concatenate(files), np.concatenate([[0], np.cumsum([f.size for f in files])])
    hdr, K3, idx3, st = C.core_decode(mixed, moff, (4, 1), 3)
    assert st.tolist() == [0, C.IREC_REC_E_STRUCTURE, 0]
    assert np.array_equal(K3[[0, 2]], K) and not K3[1].any() and not idx3[1].any() and not hdr[1].any()
    with pytest.raises(ValueError, match=r"structure differs \(image 1\)"):
        U.decode_files_ragged(mixed, moff, (4, 1), 3)
    # a block with more partitions than the call's max_K
    st = C.core_decode(blob, off, (4, 1), 2)[3]
    assert K.max() == 3 and set(st.tolist()) <= {0, 18} and 18 in st.tolist()


def test_core_reader_agrees_with_the_host_reader_on_damaged_files():
    """The damaged set of a (3, 1, 9) container as ONE blob: the core's status is nonzero exactly where the host reader fails, where both
    accept K, idx and the header are equal, the outputs of a refused image are zero -- and the statuses it reaches are all those the
    uniform damaged set reaches."""
    D = C.damaged_set()
    bpr, mk = C.DAMAGED_BPR, C.DAMAGED_MAX_K
    ok, n_prefix, n_same, R = D["ok"], D["n_prefix"], D["n_same"], C.N_RANDOM
    assert not ok[:n_prefix].any() and (~ok[n_prefix:n_prefix + R]).sum() >= 3 * R // 4 and ok[n_prefix + R:n_prefix + R + 100].all() and not ok[n_same:].any()
    assert (D["K"][n_prefix + R:n_prefix + R + 100] == D["K0"]).all() and (D["idx"][n_prefix + R:n_prefix + R + 100] == D["idx0"]).all()
    hdr, K, idx, st = C.core_decode(D["blob"], D["offsets"], bpr, mk)
    assert np.array_equal(st == 0, ok), np.flatnonzero((st == 0) != ok)
    assert np.array_equal(hdr[ok], D["hdr"][ok]) and np.array_equal(K[ok], D["K"][ok]) and np.array_equal(idx[ok], D["idx"][ok])
    assert not hdr[~ok].any() and not K[~ok].any() and not idx[~ok].any()
    assert (st[n_same:] == C.IREC_REC_E_STRUCTURE).all()
    U = U0.damaged_set()
    st_u = U0.core_decode(U["blob"], U["offsets"], *U0.DAMAGED_SHAPE)[3]
    print("statuses: ragged", sorted(set(st.tolist())), "uniform", sorted(set(st_u.tolist())))
    assert set(st_u.tolist()) <= set(st.tolist())


def test_argument_errors():
    from irec import _lib
    from irec.io import utils as U
    lib = _lib.load()
    K, idx = np.ones((2, 65), dtype=np.int32), np.zeros((2, 65, 1), dtype=np.int32)
    out, off, status = C.core_encode(K, idx, 36, (1,) * 65, expect=_lib.IREC_E_INVALID)
    assert b"IREC_REC_RAGGED_MAX_RES" in lib.irec_last_error()
    assert (out == 0xAB).all() and (off == -1).all() and (status == -1).all()           # outputs untouched
    out, off, status = C.core_encode(K[:, :64], idx[:, :64], 36, (1,) * 64)             # 64 is accepted
    blob, off_h = U.encode_files_ragged(C.SEED, C.SHAPE, C.BLOCK_SIZE, K[:, :64], idx[:, :64], 36, (1,) * 64)
    assert (status == 0).all() and np.array_equal(off, off_h) and np.array_equal(out[:off[-1]], blob)
    hdr, K2, idx2, st = C.core_decode(blob, off_h, (1,) * 64, 1)
    assert (st == 0).all() and np.array_equal(K2, K[:, :64])
    hdr, K2, idx2, st = C.core_decode(blob, off_h, (1,) * 65, 1, expect=_lib.IREC_E_INVALID)
    assert (st == -1).all() and (K2 == -1).all() and (hdr == 0xFFFFFFFF).all()
    for bad in ((2, 0, 1), (3, -1)):
        n = sum(b for b in bad if b > 0)
        C.core_encode(K[:, :n], idx[:, :n], 36, bad, expect=_lib.IREC_E_INVALID)
        assert b"below 1" in lib.irec_last_error()
        C.core_decode(blob, off_h, bad, 1, expect=_lib.IREC_E_INVALID)
        with pytest.raises(ValueError, match="blocks_per_res"):
            U.encode_files_ragged(C.SEED, C.SHAPE, C.BLOCK_SIZE, K[:, :n], idx[:, :n], 36, bad)
        with pytest.raises(ValueError, match="blocks_per_res"):
            U.decode_files_ragged(blob, off_h, bad, 1)
    big = np.array([2 ** 30, 2 ** 30], dtype=np.int32)                                  # T = 2^31: past int32, refused before any row is read
    o, s = np.full(3, -1, np.int64), np.full(2, -1, np.int32)
    assert lib.irec_rec_test_core_encode_files_ragged(1, 10, 36, 8, 8, 3, 2, 2, big.ctypes.data, 1, K.ctypes.data, 1, idx.ctypes.data, 1, None, 0,
                                                      o.ctypes.data, s.ctypes.data) == _lib.IREC_E_INVALID
    assert b"int32" in lib.irec_last_error() and (o == -1).all()
    assert lib.irec_rec_encode_files_ragged(1, 10, 36, 8, 8, 3, 2, 2, big.ctypes.data, 1, K.ctypes.data, idx.ctypes.data, None, 0, o.ctypes.data, 1) == -1
    with pytest.raises(ValueError, match=r"not \[N, 5\]"):
        U.encode_files_ragged(C.SEED, C.SHAPE, C.BLOCK_SIZE, K[:, :4], idx[:, :4], 36, (4, 1))


def test_gather_packed_ragged_row_order():
    """Two calls on three images, 2 and 5 blocks per image (the second with a short tail, so its rows are NOT in natural order), against
    rows placed by hand: image-major, call r's blocks of image i in natural block order from row i T + first[r]."""
    import torch
    from irec.coding.beam_search_coder import MorePartitionsNeeded, PendingCode
    from irec.engine import BlockLayout
    n = 3
    lay_a, lay_b = BlockLayout("cpu", n, 8, 5, 42), BlockLayout("cpu", n, 21, 5, 42)   # blocks of 5, 3 dims | 5, 5, 5, 5, 1 dims
    assert (lay_a.blocks_per_tensor, lay_b.blocks_per_tensor) == (2, 5)
    assert not np.array_equal(lay_b.natural, np.arange(15))                            # largest first: the tails sit at the end
    coder = C.StubCoder()

    def call(lay, width, tag):
        # the row of natural block (i, j) says so itself: K = 1 + (i + j) % width, idx[t] = tag + 100 i + 10 j + t
        K = torch.zeros(lay.n_blocks, dtype=torch.int32)
        idx = torch.full((lay.n_blocks, width), -7, dtype=torch.int32)
        for i in range(n):
            for j in range(lay.blocks_per_tensor):
                row = int(lay.natural[i * lay.blocks_per_tensor + j])
                K[row] = 1 + (i + j) % width
                idx[row] = torch.arange(width, dtype=torch.int32) + tag + 100 * i + 10 * j
        return PendingCode(coder, lay, K, idx, None, width)

    pend = [call(lay_a, 2, 1000), call(lay_b, 4, 2000)]
    K, idx, bpr = PendingCode.gather_packed_ragged(pend)
    assert bpr == [2, 5] and K.shape == (3, 7) and idx.shape == (3, 7, 4) and K.dtype == np.int32 and idx.dtype == np.int32
    for i in range(n):
        for r, (first, bpt, width, tag) in enumerate([(0, 2, 2, 1000), (2, 5, 4, 2000)]):
            for j in range(bpt):
                assert K[i, first + j] == 1 + (i + j) % width
                assert idx[i, first + j, :width].tolist() == [tag + 100 * i + 10 * j + t for t in range(width)]
                assert not idx[i, first + j, width:].any()                             # the narrower call's rows are zero-padded
    assert coder._max_K_hint == 4 and coder._K_reads == 2                              # each call's checks ran on its own share
    Kd, idxd, bpr_d = PendingCode.gather_packed_ragged_device(pend)
    assert bpr_d == bpr and np.array_equal(Kd.numpy(), K) and np.array_equal(idxd.numpy(), idx)
    assert Kd.data_ptr() + 4 == idxd.data_ptr() and Kd.stride() == (35, 5) and idxd.stride() == (35, 5, 1)   # views of one joined tensor
    # a block that needs more partitions than its call allowed: raised from that call's share alone
    pend[1].K[int(lay_b.natural[6])] = 9
    with pytest.raises(MorePartitionsNeeded) as e:
        PendingCode.gather_packed_ragged(pend)
    assert e.value.need == 9
    # calls on different tensor counts do not join
    from irec.coding.utils import CodingError
    with pytest.raises(CodingError):
        PendingCode.gather_packed_ragged([pend[0], call(BlockLayout("cpu", 3, 8, 5, 43), 2, 0)])
