"""GPU tests of the ragged device .rec coder (csrc/irec_rec.hip through irec.io.encode_files_device_ragged / decode_files_device_ragged):
device == host coder (irec_io.cpp, one file per call) == core hook, byte for byte, on the cases of tests/test_rec_ragged_host.py; every
file the device is given has been through the same core on the CPU first.  All comparisons are byte or integer equality."""
import numpy as np
import pytest
import torch

import rec_ragged_cases as C

pytestmark = pytest.mark.gpu


def _cuda(a):
    return torch.from_numpy(np.array(a)).cuda()          # (a copy: the cases are read-only)


def _check_case(K, idx, bpr, S, want_blob, want_off, idx_zeroed):
    from irec.io import utils as U
    n, T = K.shape
    mk, total = idx.shape[2], int(want_off[-1])
    args = (C.SEED, C.SHAPE, C.BLOCK_SIZE)
    out_core, off_core, st_core = C.core_encode(K, idx, S, bpr)                           # the core on the CPU first
    assert (st_core == 0).all() and np.array_equal(out_core[:total], want_blob) and np.array_equal(off_core, want_off)
    blob, off = U.encode_files_device_ragged(*args, _cuda(K), _cuda(idx), S, bpr)
    assert blob.is_cuda and off.is_cuda and blob.dtype == torch.uint8 and off.dtype == torch.int64
    assert np.array_equal(off.cpu().numpy(), want_off) and np.array_equal(blob.cpu().numpy(), want_blob)
    # the strided input: the K / idx views of one joined [rows][1 + width] tensor, taken without a copy
    both = _cuda(C.joined(K, idx)).reshape(n, T, 1 + mk)
    Kv, iv = both[..., 0], both[..., 1:]
    K2, ks, i2, ist = U._row_strides(Kv, iv)
    assert (ks, ist) == (1 + mk, 1 + mk) and K2.data_ptr() == both.data_ptr() and i2.data_ptr() == both.data_ptr() + 4
    blob_s, off_s = U.encode_files_device_ragged(*args, Kv, iv, S, bpr)
    assert np.array_equal(blob_s.cpu().numpy(), want_blob) and np.array_equal(off_s.cpu().numpy(), want_off)
    # one byte short: nothing is written and offsets[N] holds the true size, which the public call answers with a second run
    short = torch.full((total - 1,), 0xAB, dtype=torch.uint8, device="cuda")
    off_c, st_c, _ = U._encode_files_device_ragged_launch(*args, _cuda(K), _cuda(idx), S, bpr, short)
    assert int(off_c[-1]) == total and not st_c.any() and bool((short == 0xAB).all())
    blob_r, off_r = U.encode_files_device_ragged(*args, _cuda(K), _cuda(idx), S, bpr, out=short)
    assert blob_r.numel() == total and np.array_equal(blob_r.cpu().numpy(), want_blob) and bool((short == 0xAB).all())
    # exactly enough room, with a guard behind it: not one byte more is touched
    guard = torch.full((total + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    U._encode_files_device_ragged_launch(*args, Kv, iv, S, bpr, guard[:total])
    assert np.array_equal(guard[:total].cpu().numpy(), want_blob) and bool((guard[total:] == 0xAB).all())
    # and back: the host's files through the device reader, offsets on the host and on the device
    hdr_core, K_core, idx_core, st = C.core_decode(want_blob, want_off, bpr, mk)
    assert (st == 0).all() and np.array_equal(K_core, K) and np.array_equal(idx_core, idx_zeroed)
    hdr, Kd, idxd = U.decode_files_device_ragged(_cuda(want_blob), want_off, bpr, mk)
    assert hdr.is_cuda and Kd.is_cuda and idxd.is_cuda and Kd.shape == (n, T) and idxd.shape == (n, T, mk)
    assert np.array_equal(Kd.cpu().numpy(), K) and np.array_equal(idxd.cpu().numpy(), idx_zeroed)
    assert np.array_equal(hdr.cpu().numpy().astype(np.uint32), hdr_core)
    hdr2, K2, idx2, st2 = U._decode_files_device_ragged_launch(_cuda(want_blob), _cuda(want_off), bpr, mk, on_device=True)
    assert not st2.any() and torch.equal(K2, Kd) and torch.equal(idx2, idxd)


def _n3_cases():
    return [(i, name) for i, name in enumerate(C.case_names()) if "-N3-" in name]


@pytest.mark.parametrize("which", [i for i, _ in _n3_cases()], ids=[name for _, name in _n3_cases()])
def test_device_files_equal_the_host_coder_and_the_core(engine, which):
    c = C.cases()[which]
    _check_case(c["K"], c["idx"], c["bpr"], c["max_index"], c["blob"], c["offsets"], c["idx_zeroed"])


def test_more_lanes_than_a_wave_of_each_stream_kind(engine):
    """(1, 4) at N = 70: 140 index lanes and 140 count lanes, so the boundary between the two kinds falls inside a wave and each kind spans
    more than one."""
    from irec.io import utils as U
    rng = np.random.default_rng(70)
    bpr, mk, S, n = (1, 4), 7, 36, 70
    K = rng.integers(0, mk + 1, (n, 5)).astype(np.int32)
    K[3, 0], K[3, 1], K[69, 4] = 0, mk, mk
    idx = rng.integers(0, S, (n, 5, mk)).astype(np.int32)
    files = [C.file_of(l, S) for l in C.lists_of(K, idx, bpr)]                            # irec_rec_encode_file, image after image
    blob = np.frombuffer(b"".join(files), dtype=np.uint8)
    off = np.concatenate([[0], np.cumsum([len(f) for f in files])]).astype(np.int64)
    blob_h, off_h = U.encode_files_ragged(C.SEED, C.SHAPE, C.BLOCK_SIZE, K, idx, S, bpr)
    assert np.array_equal(blob_h, blob) and np.array_equal(off_h, off)
    _check_case(K, idx, bpr, S, blob, off, np.where(np.arange(mk)[None, None, :] < K[..., None], idx, 0).astype(np.int32))


def test_device_refuses_one_image_alone(engine):
    from irec.io import utils as U
    c = next(c for c in C.cases() if c["bpr"] == (3, 1, 5) and c["K"].shape[0] == 3 and c["max_index"] == 20)
    K, idx, bpr, mk = np.array(c["K"]), np.array(c["idx"]), c["bpr"], c["idx"].shape[2]
    K[1, 4] = max(K[1, 4], 1)
    idx[1, 4, 0] = 20
    out_c, off_c, st_c = C.core_encode(K, idx, 20, bpr)
    assert st_c.tolist() == [0, 2, 0]
    out = torch.full((int(off_c[-1]) + 16,), 0xAB, dtype=torch.uint8, device="cuda")
    off, st, _ = U._encode_files_device_ragged_launch(C.SEED, C.SHAPE, C.BLOCK_SIZE, _cuda(K), _cuda(idx), 20, bpr, out[:int(off_c[-1])])
    assert st.cpu().tolist() == [0, 2, 0] and np.array_equal(off.cpu().numpy(), off_c)
    assert np.array_equal(out.cpu().numpy(), out_c[:out.numel()])                         # the two good files, the guard untouched
    with pytest.raises(ValueError, match=r"max_index.*\(image 1\)"):
        U.encode_files_device_ragged(C.SEED, C.SHAPE, C.BLOCK_SIZE, _cuda(K), _cuda(idx), 20, bpr)
    K[2, 8] = mk + 1
    assert C.core_encode(K, idx, 20, bpr)[2].tolist() == [0, 2, 1]
    with pytest.raises(ValueError, match=r"max_index.*\(image 1\)"):                      # the first refused image is named
        U.encode_files_device_ragged(C.SEED, C.SHAPE, C.BLOCK_SIZE, _cuda(K), _cuda(idx), 20, bpr)


@pytest.mark.parametrize("offsets_on_device", [False, True], ids=["host_offsets", "device_offsets"])
def test_device_reader_on_damaged_files_equals_the_core(engine, offsets_on_device):
    """The ragged damaged set as ONE call.  Each file goes through the core hook on the CPU first (where it agrees with the host reader:
    tests/test_rec_ragged_host.py); the device's statuses, accepted outputs and zeroing are the hook's."""
    from irec.io import utils as U
    D = C.damaged_set()
    bpr, mk = C.DAMAGED_BPR, C.DAMAGED_MAX_K
    hdr_c, K_c, idx_c, st_c = C.core_decode(D["blob"], D["offsets"], bpr, mk)
    assert np.array_equal(st_c == 0, D["ok"]) and D["ok"].sum() >= 100 and (~D["ok"]).sum() >= 400
    assert (st_c[D["n_same"]:] == C.IREC_REC_E_STRUCTURE).all()
    offsets = _cuda(D["offsets"]) if offsets_on_device else D["offsets"]
    hdr, K, idx, st = U._decode_files_device_ragged_launch(_cuda(D["blob"]), offsets, bpr, mk, on_device=offsets_on_device)
    assert np.array_equal(st.cpu().numpy(), st_c)
    assert np.array_equal(hdr.cpu().numpy().view(np.uint32), hdr_c)
    assert np.array_equal(K.cpu().numpy(), K_c) and np.array_equal(idx.cpu().numpy(), idx_c)       # (zeroed where rejected, in both)
    ok = D["ok"]
    assert np.array_equal(K.cpu().numpy()[ok], D["K"][ok]) and np.array_equal(idx.cpu().numpy()[ok], D["idx"][ok])
    if not offsets_on_device:
        with pytest.raises(ValueError, match=r"\(image 0\)"):
            U.decode_files_device_ragged(_cuda(D["blob"]), offsets, bpr, mk)


def test_a_file_split_differently_is_another_structure(engine):
    from irec.io import utils as U
    rng = np.random.default_rng(5)
    K = rng.integers(0, 4, (2, 5)).astype(np.int32)
    idx = rng.integers(0, 36, (2, 5, 3)).astype(np.int32)
    blob, off = U.encode_files_ragged(1, (8, 8, 3), 10, K, idx, 36, (4, 1))
    assert (C.core_decode(blob, off, (1, 4), 3)[3] == C.IREC_REC_E_STRUCTURE).all()
    hdr, K2, idx2, st = U._decode_files_device_ragged_launch(_cuda(blob), off, (1, 4), 3)
    assert (st.cpu().numpy() == C.IREC_REC_E_STRUCTURE).all() and not hdr.any() and not K2.any() and not idx2.any()
    with pytest.raises(ValueError, match=r"structure.*\(image 0\)"):
        U.decode_files_device_ragged(_cuda(blob), off, (1, 4), 3)
    with pytest.raises(ValueError, match="offsets"):           # ranges outside the blob never reach a kernel
        U.decode_files_device_ragged(_cuda(blob), np.array([0, blob.size + 1]), (4, 1), 3)


def test_argument_errors(engine):
    """R = 65: IREC_E_INVALID with text, nothing launched, the outputs untouched.  R = 64 is accepted."""
    from irec import _lib
    from irec.io import utils as U
    lib = _lib.load()
    K, idx = np.ones((2, 65), dtype=np.int32), np.zeros((2, 65, 1), dtype=np.int32)
    Kd, idxd = _cuda(K), _cuda(idx)
    out = torch.full((4096,), 0xAB, dtype=torch.uint8, device="cuda")
    offsets = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    status = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.irec_rec_device_workspace_bytes(2, 65), dtype=torch.uint8, device="cuda")
    bpr = np.ones(65, dtype=np.int32)
    stream = torch.cuda.current_stream().cuda_stream
    st = lib.irec_rec_encode_files_device_ragged(C.SEED, C.BLOCK_SIZE, 36, *C.SHAPE, 2, 65, bpr.ctypes.data, 1, Kd.data_ptr(), 1, idxd.data_ptr(), 1,
                                                 out.data_ptr(), out.numel(), offsets.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), stream)
    assert st == _lib.IREC_E_INVALID and b"IREC_REC_RAGGED_MAX_RES" in lib.irec_last_error()
    torch.cuda.synchronize()
    assert bool((out == 0xAB).all()) and bool((offsets == -1).all()) and bool((status == -1).all())
    with pytest.raises(ValueError, match="IREC_REC_RAGGED_MAX_RES"):
        U.encode_files_device_ragged(C.SEED, C.SHAPE, C.BLOCK_SIZE, Kd, idxd, 36, (1,) * 65)
    blob, off = U.encode_files_device_ragged(C.SEED, C.SHAPE, C.BLOCK_SIZE, Kd[:, :64], idxd[:, :64], 36, (1,) * 64)
    want, want_off = U.encode_files_ragged(C.SEED, C.SHAPE, C.BLOCK_SIZE, K[:, :64], idx[:, :64], 36, (1,) * 64)
    assert np.array_equal(blob.cpu().numpy(), want) and np.array_equal(off.cpu().numpy(), want_off)
    hdr = torch.full((2, 9), -1, dtype=torch.int32, device="cuda")
    K2 = torch.full((2, 65), -1, dtype=torch.int32, device="cuda")
    st = lib.irec_rec_decode_files_device_ragged(blob.data_ptr(), off.data_ptr(), 2, 65, bpr.ctypes.data, 1, hdr.data_ptr(), K2.data_ptr(), idxd.data_ptr(),
                                                 status.data_ptr(), ws.data_ptr(), ws.numel(), stream)
    assert st == _lib.IREC_E_INVALID and b"IREC_REC_RAGGED_MAX_RES" in lib.irec_last_error()
    torch.cuda.synchronize()
    assert bool((hdr == -1).all()) and bool((K2 == -1).all()) and bool((status == -1).all())
    with pytest.raises(ValueError, match="IREC_REC_RAGGED_MAX_RES"):
        U.decode_files_device_ragged(blob, off, (1,) * 65, 1)
    hdr64, K64, idx64 = U.decode_files_device_ragged(blob, off, (1,) * 64, 1)
    assert np.array_equal(K64.cpu().numpy(), K[:, :64]) and not idx64.any()
    with pytest.raises(ValueError, match="blocks_per_res"):
        U.encode_files_device_ragged(C.SEED, C.SHAPE, C.BLOCK_SIZE, Kd[:, :3], idxd[:, :3], 36, (2, 0, 1))
