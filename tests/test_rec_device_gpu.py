"""GPU tests of the device .rec coder (csrc/irec_rec.hip through irec.io.encode_files_device / decode_files_device): device == host
coder (irec_io.cpp) == core hook, byte for byte, on the cases of tests/test_rec_device_host.py; every file the device is given has been
through the same core on the CPU first.  All comparisons are byte or integer equality."""
import numpy as np
import pytest
import torch

import rec_device_cases as C

pytestmark = pytest.mark.gpu


def _cuda(a):
    return torch.from_numpy(np.array(a)).cuda()          # (a copy: the cases are read-only)


@pytest.mark.parametrize("which", range(len(C.case_names())), ids=C.case_names())
def test_device_files_equal_the_host_coder_and_the_core(engine, which):
    from irec.io import utils as U
    c = C.cases()[which]
    K, idx = c["K"], c["idx"]
    n, R, bpt = K.shape
    mk = idx.shape[3]
    total = int(c["offsets"][-1])
    args = (c["seed"], c["shape"], c["block_size"])
    out_core, off_core, st_core = C.core_encode(*args, K, idx, c["max_index"])           # the core on the CPU first
    assert (st_core == 0).all() and np.array_equal(out_core[:total], c["blob"]) and np.array_equal(off_core, c["offsets"])
    blob, off = U.encode_files_device(*args, _cuda(K), _cuda(idx), c["max_index"])
    assert blob.is_cuda and off.is_cuda and blob.dtype == torch.uint8 and off.dtype == torch.int64
    assert np.array_equal(off.cpu().numpy(), c["offsets"])
    assert np.array_equal(blob.cpu().numpy(), c["blob"])
    if c["golden"]:
        host = blob.cpu().numpy()
        for i, want in enumerate(c["golden"]):
            assert host[c["offsets"][i]:c["offsets"][i + 1]].tobytes() == want
    # the strided input: the K / idx views of one joined [rows][1 + width] tensor, taken without a copy
    both = _cuda(C.joined(K, idx)).reshape(n, R, bpt, 1 + mk)
    Kv, iv = both[..., 0], both[..., 1:]
    K2, ks, i2, ist = U._block_strides(Kv, iv)
    assert (ks, ist) == (1 + mk, 1 + mk) and K2.data_ptr() == both.data_ptr() and i2.data_ptr() == both.data_ptr() + 4
    blob_s, off_s = U.encode_files_device(*args, Kv, iv, c["max_index"])
    assert np.array_equal(blob_s.cpu().numpy(), c["blob"]) and np.array_equal(off_s.cpu().numpy(), c["offsets"])
    # one byte short: nothing is written and offsets[N] holds the true size ...
    short = torch.full((total - 1,), 0xAB, dtype=torch.uint8, device="cuda")
    off_c, st_c, _ = U._encode_files_device_launch(*args, _cuda(K), _cuda(idx), c["max_index"], short)
    assert int(off_c[-1]) == total and not st_c.any() and bool((short == 0xAB).all())
    # ... which the public call answers by running once more with exactly that size
    blob_r, off_r = U.encode_files_device(*args, _cuda(K), _cuda(idx), c["max_index"], out=short)
    assert blob_r.numel() == total and np.array_equal(blob_r.cpu().numpy(), c["blob"]) and bool((short == 0xAB).all())
    # exactly enough room, with a guard behind it: not one byte more is touched
    guard = torch.full((total + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    off_e, st_e, _ = U._encode_files_device_launch(*args, _cuda(K), _cuda(idx), c["max_index"], guard[:total])
    assert np.array_equal(guard[:total].cpu().numpy(), c["blob"]) and bool((guard[total:] == 0xAB).all())
    # and back: the host's files (which the core hook decodes to the same on the CPU) through the device reader
    hdr_core, K_core, idx_core, st = C.core_decode(c["blob"], c["offsets"], R, bpt, mk)
    assert (st == 0).all() and np.array_equal(K_core, K) and np.array_equal(idx_core, c["idx_zeroed"])
    hdr, Kd, idxd = U.decode_files_device(_cuda(c["blob"]), _cuda(c["offsets"]), R, bpt, mk)
    assert hdr.is_cuda and Kd.is_cuda and idxd.is_cuda
    assert np.array_equal(Kd.cpu().numpy(), K) and np.array_equal(idxd.cpu().numpy(), c["idx_zeroed"])
    assert np.array_equal(hdr.cpu().numpy().astype(np.uint32), hdr_core)


def test_device_errors_name_the_image(engine):
    from irec.io import utils as U
    K = np.ones((3, 2, 2), dtype=np.int32)
    idx = np.zeros((3, 2, 2, 2), dtype=np.int32)
    bad = idx.copy()
    bad[1, 0, 0, 0] = 36
    assert C.core_encode(1, (8, 8, 3), 10, K, bad, 36)[2].tolist() == [0, 2, 0]
    with pytest.raises(ValueError, match=r"max_index.*\(image 1\)"):
        U.encode_files_device(1, (8, 8, 3), 10, _cuda(K), _cuda(bad), 36)
    Kbad = K.copy()
    Kbad[2, 1, 1] = 3
    assert C.core_encode(1, (8, 8, 3), 10, Kbad, idx, 36)[2].tolist() == [0, 0, 1]
    with pytest.raises(ValueError, match=r"K out of range \(image 2\)"):
        U.encode_files_device(1, (8, 8, 3), 10, _cuda(Kbad), _cuda(idx), 36)
    blob, off = U.encode_files(1, (8, 8, 3), 10, K, idx, 36)
    assert (C.core_decode(blob, off, 2, 3, 2)[3] == C.IREC_REC_E_STRUCTURE).all()
    hdr, K2, idx2, st = U._decode_files_device_launch(_cuda(blob), off, 2, 3, 2)
    assert (st.cpu().numpy() == C.IREC_REC_E_STRUCTURE).all() and not hdr.any() and not K2.any() and not idx2.any()
    with pytest.raises(ValueError, match=r"structure.*\(image 0\)"):
        U.decode_files_device(_cuda(blob), off, 2, 3, 2)
    with pytest.raises(ValueError, match="offsets"):           # ranges outside the blob never reach a kernel
        U.decode_files_device(_cuda(blob), np.array([0, blob.size + 1]), 2, 2, 2)


def test_one_layout_through_the_uniform_and_the_ragged_entries(engine):
    """N = 3, R = 2, bpt = 3 through irec_rec_*_files_device and, as R equal entries, through irec_rec_*_files_device_ragged; then both
    layouts with tables (irec_rec_*_files_device_tables either way): the same bytes, offsets and statuses, which without tables are the
    core hook's on the CPU.  Image 1 holds a K of 3 > max_K = 2: status 1 and an empty file."""
    from irec.io import SymbolTables, utils as U
    rng = np.random.default_rng(23)
    n, R, bpt, mk, S = 3, 2, 3, 2, 20
    K = rng.integers(0, mk + 1, (n, R, bpt)).astype(np.int32)
    K[1, 1, 2] = 3
    idx = rng.integers(0, S, (n, R, bpt, mk)).astype(np.int32)
    meta = (5, (8, 8, 3), 10)
    out_c, off_c, st_c = C.core_encode(*meta, K, idx, S)
    cap = C.first_allowance(n, R, bpt, mk)
    assert st_c.tolist() == [0, 1, 0] and 0 < off_c[1] == off_c[2] < off_c[3] <= cap
    Kd, idxd = _cuda(K), _cuda(idx)
    rows, uniform, ragged = (Kd.view(n, R * bpt), idxd.view(n, R * bpt, mk)), U._Layout(R, bpt), U._Layout.ragged([bpt] * R, "test")
    for tables in (None, SymbolTables(np.arange(1, S + 2), [np.arange(1, mk + 3)] * R)):
        got = []
        for launch in (lambda o: U._encode_rows_device_launch(*meta, *rows, S, uniform, o, tables, "test"),
                       lambda o: U._encode_rows_device_launch(*meta, *rows, S, ragged, o, tables, "test"),
                       lambda o: U._encode_files_device_ragged_launch(*meta, *rows, S, [bpt] * R, o, tables)):
            out = torch.full((cap,), 0xAB, dtype=torch.uint8, device="cuda")
            off, st, _ = launch(out)
            got.append((out.cpu().numpy(), off.cpu().numpy(), st.cpu().numpy()))
        if tables is None:                                     # the public-facing uniform launch, and the core on the CPU
            out = torch.full((cap,), 0xAB, dtype=torch.uint8, device="cuda")
            off, st, _ = U._encode_files_device_launch(*meta, Kd, idxd, S, out)
            got += [(out.cpu().numpy(), off.cpu().numpy(), st.cpu().numpy()), (out_c[:cap], off_c, st_c)]
        for blob, off, st in got[1:]:
            assert np.array_equal(blob, got[0][0]) and np.array_equal(off, got[0][1]) and np.array_equal(st, got[0][2])
        blob, off_d, st = got[0]
        assert st.tolist() == [0, 1, 0] and 0 < off_d[1] == off_d[2] < off_d[3] <= cap and (blob[off_d[3]:] == 0xAB).all()
        blob_d = torch.from_numpy(blob[:off_d[3]].copy()).cuda()
        back = [U._decode_rows_device_launch(blob_d, off_d, layout, mk, False, tables, "test") for layout in (uniform, ragged)]
        back.append(U._decode_files_device_ragged_launch(blob_d, off_d, [bpt] * R, mk, tables=tables))
        hdr, K3, idx4, st = U._decode_files_device_launch(blob_d, off_d, R, bpt, mk, tables=tables)
        assert K3.shape == (n, R, bpt) and idx4.shape == (n, R, bpt, mk)
        back.append((hdr, K3.view(n, -1), idx4.view(n, -1, mk), st))
        for hdr, K2, idx2, st in back:
            assert all(torch.equal(a, b) for a, b in zip((hdr, K2, idx2, st), back[0]))
        hdr, K2, idx2, st = (t.cpu().numpy() for t in back[0])
        assert st.tolist() == [0, 4, 0] and not hdr[1].any() and not K2[1].any() and not idx2[1].any()   # the empty file: a truncated header
        keep = [0, 2]
        assert np.array_equal(K2[keep], K.reshape(n, -1)[keep])
        assert np.array_equal(idx2[keep], np.where(np.arange(mk) < K[..., None], idx, 0).reshape(n, -1, mk)[keep])


def test_device_reader_on_damaged_files_equals_the_core(engine):
    """The damaged set as ONE call of 1746 files.  Each file goes through the core hook on the CPU first (where it agrees with the host
    reader: tests/test_rec_device_host.py); the device's statuses and accepted outputs are the hook's."""
    from irec.io import utils as U
    D = C.damaged_set()
    R, bpt, mk = C.DAMAGED_SHAPE
    hdr_c, K_c, idx_c, st_c = C.core_decode(D["blob"], D["offsets"], R, bpt, mk)
    assert np.array_equal(st_c == 0, D["ok"]) and D["ok"].sum() >= 200 and (~D["ok"]).sum() >= 1446
    hdr, K, idx, st = U._decode_files_device_launch(_cuda(D["blob"]), D["offsets"], R, bpt, mk)
    assert np.array_equal(st.cpu().numpy(), st_c)
    assert np.array_equal(hdr.cpu().numpy().view(np.uint32), hdr_c)
    assert np.array_equal(K.cpu().numpy(), K_c) and np.array_equal(idx.cpu().numpy(), idx_c)       # (zeroed where rejected, in both)
    ok = D["ok"]
    assert np.array_equal(K.cpu().numpy()[ok], D["K"][ok]) and np.array_equal(idx.cpu().numpy()[ok], D["idx"][ok])


def test_two_calls_in_flight_on_two_streams(engine):
    from irec.io import utils as U
    a, b = C.cases()[1], C.cases()[5]                          # (9, 5, 9, 12, 36) and (1500, 1, 1, 2, 36)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    ins = [(c, _cuda(c["K"]), _cuda(c["idx"]), torch.empty(int(c["offsets"][-1]), dtype=torch.uint8, device="cuda")) for c in (a, b)]
    torch.cuda.synchronize()
    outs = []
    for rounds in range(3):                                    # launches of the two calls interleaved, nothing read back in between
        for (c, K, idx, out), s in zip(ins, (s1, s2)):
            with torch.cuda.stream(s):
                outs.append((c, out, U._encode_files_device_launch(c["seed"], c["shape"], c["block_size"], K, idx, c["max_index"], out)))
    torch.cuda.synchronize()
    for c, out, (off, st, _) in outs:
        assert not st.any() and np.array_equal(off.cpu().numpy(), c["offsets"]) and np.array_equal(out.cpu().numpy(), c["blob"])
    decs = []
    for c, s in zip((a, b), (s1, s2)):
        with torch.cuda.stream(s):
            decs.append((c, U._decode_files_device_launch(_cuda(c["blob"]), c["offsets"], *c["K"].shape[1:], c["idx"].shape[3])))
    torch.cuda.synchronize()
    for c, (hdr, K, idx, st) in decs:
        assert not st.any() and np.array_equal(K.cpu().numpy(), c["K"]) and np.array_equal(idx.cpu().numpy(), c["idx_zeroed"])


def test_harness_with_the_files_built_on_the_device(engine, tmp_path):
    """compress -> .rec -> read back, end to end on the smallest model shape of tests/test_models_shim.py and four images: the rows of
    compress_images(..., rec_on_device=True) equal the default path's, and the files are byte-identical."""
    from irec import harness
    from test_models_shim import _model
    m = _model("cuda")
    torch.manual_seed(7)
    images = torch.rand(4, 3, 32, 32, device="cuda") - 0.5
    names_h, names_d = [f"host_{i}" for i in range(4)], [f"dev_{i}" for i in range(4)]
    rows_h = harness.compress_images(m, images, names_h, 42, 1000, str(tmp_path), batch=3)
    rows_d = harness.compress_images(m, images, names_d, 42, 1000, str(tmp_path), batch=3, rec_on_device=True)
    assert len(rows_h) == len(rows_d) == 4
    for a, b in zip(rows_h, rows_d):
        assert set(a) == set(b)
        assert (a["comp_codelength"], a["n_indices"], a["indices_recovered"]) == (b["comp_codelength"], b["n_indices"], b["indices_recovered"])
        assert b["indices_recovered"] is True and b["n_indices"] > 0
    for h, d in zip(names_h, names_d):
        assert (tmp_path / f"{h}.rec").read_bytes() == (tmp_path / f"{d}.rec").read_bytes()
    # compress_rec itself: the files of compress_packed's arrays
    from irec.io import encode_files
    K, idx, recon = m.compress_packed(images, seed=42)
    blob, off, recon_d = m.compress_rec(images, seed=42)
    want, want_off = encode_files(42, (32, 32, 3), 1000, K, idx, m.residual_blocks[0].coder.n_samples)
    assert np.array_equal(blob.cpu().numpy(), want) and np.array_equal(off.cpu().numpy(), want_off) and torch.equal(recon, recon_d)
