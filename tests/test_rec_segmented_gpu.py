"""GPU tests of the segmented .rec container (NAME.recs): the device pair (irec_rec_encode_files_device_segmented /
irec_rec_decode_files_device_segmented, csrc/irec_rec_seg.hip) against the host pair byte for byte and status for status, on the case
grid and the damaged set of tests/rec_segmented_cases.py -- every file the device reads here has been through the same lane functions
on the CPU first (tests/test_rec_segmented_host.py, and once more below before the upload) --, one run inside the canary arena of
tests/guarded.py, and the two models' compress_rec / decompress_rec with segment_blocks against their plain path."""
import functools

import numpy as np
import pytest
import torch

import guarded as G
import rec_ragged_cases as RC
import rec_segmented_cases as C

pytestmark = pytest.mark.gpu

CASES = range(len(C.case_names()))
I32, I64, U8 = torch.int32, torch.int64, torch.uint8


def _files(blob, off):
    blob, off = (blob.cpu().numpy(), off.cpu().numpy()) if hasattr(blob, "cpu") else (blob, off)
    return [blob[off[i]:off[i + 1]].tobytes() for i in range(len(off) - 1)]


@pytest.mark.parametrize("which", CASES, ids=C.case_names())
def test_device_files_and_rows_equal_the_hosts(engine, which):
    from irec.io import segmented as SG
    h, w, ch = C.SHAPE
    for g in C.SEGMENT_BLOCKS:
        c = C.case(which, g)
        K, idx, bpr, S, mk = c["K"], c["idx"], c["bpr"], c["max_index"], c["idx"].shape[2]
        host_blob, host_off = SG.encode_files_segmented(C.SEED, C.SHAPE, C.BLOCK_SIZE, K, idx, S, bpr, g, n_threads=16)
        assert np.array_equal(host_blob, c["blob"]) and np.array_equal(host_off, c["offsets"])
        Kd, Id = torch.from_numpy(np.array(K)).cuda(), torch.from_numpy(np.array(idx)).cuda()
        both = torch.from_numpy(RC.joined(K, idx)).cuda().view(K.shape[0], K.shape[1], 1 + mk)   # the views of one joined tensor: strided rows
        for Kv, Iv in ((Kd, Id), (both[..., 0], both[..., 1:])):
            if K.shape[0] == 0:                              # no images: an empty tensor has no address, which the device writer refuses
                with pytest.raises(ValueError, match="irec_rec_encode_files_device_segmented: bad arguments"):
                    SG.encode_files_device_segmented(C.SEED, C.SHAPE, C.BLOCK_SIZE, Kv, Iv, S, bpr, g)
                blob, off = torch.from_numpy(np.array(host_blob)).cuda(), host_off       # (the reader takes the host's no bytes)
                continue
            blob, off = SG.encode_files_device_segmented(C.SEED, C.SHAPE, C.BLOCK_SIZE, Kv, Iv, S, bpr, g)
            assert blob.is_cuda and np.array_equal(off.cpu().numpy(), host_off) and np.array_equal(blob.cpu().numpy(), host_blob), g
        if K.shape[0]:                                                                           # (no images: no byte to be short of)
            short = torch.full((int(host_off[-1]) - 1,), 0xAB, dtype=U8, device="cuda")          # one byte short: nothing written, then a second run
            blob, off = SG.encode_files_device_segmented(C.SEED, C.SHAPE, C.BLOCK_SIZE, Kd, Id, S, bpr, g, out=short)
            assert (short == 0xAB).all() and np.array_equal(blob.cpu().numpy(), host_blob)
        hdr, K2, idx2 = SG.decode_files_device_segmented(blob, off, bpr, mk)                     # g from the header
        assert np.array_equal(K2.cpu().numpy(), K) and np.array_equal(idx2.cpu().numpy(), c["idx_zeroed"])
        assert (hdr.cpu().numpy() == np.array([C.SEED, C.BLOCK_SIZE, S, h, w, ch, 0, 0, len(bpr)])).all()
        hdr, K2, idx2, st = SG._decode_files_device_segmented_launch(blob, off, bpr, g, mk + 3, on_device=True)
        assert not st.any() and np.array_equal(K2.cpu().numpy(), K) and not idx2[..., mk:].any()
        assert np.array_equal(idx2[..., :mk].cpu().numpy(), c["idx_zeroed"])


def test_device_reader_agrees_with_the_host_on_damaged_files(engine):
    """The damaged set goes to the GPU only after the host twin has been through it: every cause comes back as a status, the same one,
    and the rows are the host's -- zero for a refused image, intact beside it."""
    from irec.io import segmented as SG
    D = C.damaged_set()
    bpr, g, mk = C.DAMAGED_BPR, C.DAMAGED_G, C.DAMAGED_MAX_K
    hdr_h, K_h, idx_h, st_h = C.core_decode(D["blob"], D["offsets"], bpr, g, mk)                 # the same lane functions on the CPU, first
    assert st_h[:D["n_named"]].tolist() == D["want"]
    blob = torch.from_numpy(np.array(D["blob"])).cuda()
    hdr, K, idx, st = SG._decode_files_device_segmented_launch(blob, D["offsets"], bpr, g, mk)
    st = st.cpu().numpy()
    assert np.array_equal(st, st_h), [(D["names"][i], int(st[i]), int(st_h[i])) for i in np.flatnonzero(st != st_h)[:10]]
    assert np.array_equal(K.cpu().numpy(), K_h) and np.array_equal(idx.cpu().numpy(), idx_h)
    assert np.array_equal(hdr.cpu().numpy().view(np.uint32), hdr_h)
    bad = torch.from_numpy(st != 0).cuda()
    assert not K[bad].any() and not idx[bad].any() and not hdr[bad].any()
    one = torch.from_numpy(np.frombuffer(D["data"], dtype=np.uint8).copy()).cuda()
    off = np.array([0, one.numel()])
    for other_g, other_mk, want in ((2, mk, C.E_SEG_BLOCKS), (g, mk - 1, 18)):
        assert C.core_decode(one.cpu().numpy(), off, bpr, other_g, other_mk)[3].tolist() == [want]
        assert SG._decode_files_device_segmented_launch(one, off, bpr, other_g, other_mk)[3].tolist() == [want]
    with pytest.raises(ValueError, match=r"not the file's length \(image 0\)"):
        SG.decode_files_device_segmented(one[:-1].contiguous(), np.array([0, one.numel() - 1]), bpr, mk, g)


def _stream(engine):
    return torch.cuda.current_stream().cuda_stream


def test_one_run_in_the_arena(engine):
    """Outputs pre-filled, the workspace exactly the sized bytes and filled with 0xFF, inputs compared as bytes afterwards, the blob's
    capacity exact; then a capacity one byte short, which the call answers the way every writer of include/irec.h does -- offsets[N] above
    the capacity, the caller's sign to call again -- with no image's status set and the blob untouched."""
    from irec import _lib
    lib = engine.lib
    c = C.case(C.case_names().index("13_302-N3-S36"), 4)
    K, idx, bpr, g, S = c["K"], c["idx"], c["bpr"], 4, c["max_index"]
    n, T, mk, R = K.shape[0], K.shape[1], idx.shape[2], len(bpr)
    total = int(c["offsets"][-1])
    b = np.asarray(bpr, dtype=np.int32)
    need = lib.irec_rec_seg_workspace_bytes(n, R, b.ctypes.data, g)
    assert need > 0
    arena = G.Arena(G.slack(20) + 3 * need + 8 * (K.size + idx.size) + 4 * total + 256 * (n + 1), "cuda")
    Kd, Id = arena.put(K, name="K"), arena.put(idx, name="idx")
    out = arena.region(U8, (total,), "out", name="out")
    offsets = arena.region(I64, (n + 1,), "out", name="offsets")
    status = arena.region(I32, (n,), "out", name="status")
    ws = arena.workspace(need, 0xFFFFFFFF)
    arena.arm()
    _lib.check(lib.irec_rec_encode_files_device_segmented(C.SEED, C.BLOCK_SIZE, S, *C.SHAPE, n, R, b.ctypes.data, g, mk, Kd.data_ptr(), 1, Id.data_ptr(), mk,
                                                          out.data_ptr(), total, offsets.data_ptr(), status.data_ptr(), ws.data_ptr(), need, _stream(engine)),
               "irec_rec_encode_files_device_segmented")
    torch.cuda.synchronize()
    arena.check()
    assert not status.any() and np.array_equal(offsets.cpu().numpy(), c["offsets"]) and np.array_equal(out.cpu().numpy(), c["blob"])
    out_s = arena.region(U8, (total - 1,), "out", name="out (one byte short)")
    offsets_s = arena.region(I64, (n + 1,), "out", name="offsets (short)")
    status_s = arena.region(I32, (n,), "out", name="status (short)")
    ws_s = arena.workspace(need, 0xFFFFFFFF, name="workspace (short)")
    arena.arm()
    _lib.check(lib.irec_rec_encode_files_device_segmented(C.SEED, C.BLOCK_SIZE, S, *C.SHAPE, n, R, b.ctypes.data, g, mk, Kd.data_ptr(), 1, Id.data_ptr(), mk,
                                                          out_s.data_ptr(), total - 1, offsets_s.data_ptr(), status_s.data_ptr(), ws_s.data_ptr(), need,
                                                          _stream(engine)), "irec_rec_encode_files_device_segmented")
    torch.cuda.synchronize()
    arena.check()
    assert int(offsets_s[-1]) == total > total - 1 and np.array_equal(offsets_s.cpu().numpy(), c["offsets"])              # the error: the size it needs
    assert (out_s == G.PREFILL_U8).all() and not status_s.any()                                                              # and nothing written
    blob, off = arena.put(c["blob"], name="bytes"), arena.put(c["offsets"], name="offsets (in)")
    hdr = arena.region(I32, (n, 9), "out", name="headers")
    K2 = arena.region(I32, (n, T), "out", name="K (decoded)")
    idx2 = arena.region(I32, (n, T, mk), "out", name="idx (decoded)")
    st2 = arena.region(I32, (n,), "out", name="status (decoded)")
    ws2 = arena.workspace(need, 0xFFFFFFFF, name="workspace (decode)")
    arena.arm()
    _lib.check(lib.irec_rec_decode_files_device_segmented(blob.data_ptr(), off.data_ptr(), n, R, b.ctypes.data, g, mk, hdr.data_ptr(), K2.data_ptr(),
                                                          idx2.data_ptr(), st2.data_ptr(), ws2.data_ptr(), need, _stream(engine)),
               "irec_rec_decode_files_device_segmented")
    torch.cuda.synchronize()
    arena.check()
    assert not st2.any() and np.array_equal(K2.cpu().numpy(), K) and np.array_equal(idx2.cpu().numpy(), c["idx_zeroed"])
    h, w, ch = C.SHAPE
    assert (hdr.cpu().numpy().view(np.uint32) == np.array([C.SEED, C.BLOCK_SIZE, S, h, w, ch, 0, 0, R], dtype=np.uint32)).all()
    # a workspace one byte short, or a segment size of 0: an error before any launch, the outputs untouched
    assert lib.irec_rec_decode_files_device_segmented(blob.data_ptr(), off.data_ptr(), n, R, b.ctypes.data, g, mk, hdr.data_ptr(), K2.data_ptr(),
                                                      idx2.data_ptr(), st2.data_ptr(), ws2.data_ptr(), 7, _stream(engine)) == _lib.IREC_E_WORKSPACE
    assert lib.irec_rec_encode_files_device_segmented(C.SEED, C.BLOCK_SIZE, S, *C.SHAPE, n, R, b.ctypes.data, 0, mk, Kd.data_ptr(), 1, Id.data_ptr(), mk,
                                                      out_s.data_ptr(), total - 1, offsets_s.data_ptr(), status_s.data_ptr(), ws_s.data_ptr(), need,
                                                      _stream(engine)) == _lib.IREC_E_INVALID
    torch.cuda.synchronize()
    arena.check()
    assert (out_s == G.PREFILL_U8).all()


# ---- the models ---------------------------------------------------------------------------------------------------------------------------
SEED, SIZE, BLOCK = 42, 128, 5
LADDER = (16., 64., 256., 1024., 4096.)


@functools.lru_cache(maxsize=None)
def _lossy():
    """Large2LevelVAE(level_1_filters=8, level_2_filters=4) on 128 x 128 images: 16 dims at level 2 and 512 at level 1, blocks of 5 dims:
    blocks_per_res = [4, 103], tails of 1 and 2 dims.  The heads of both posteriors' locs scaled by the first step of LADDER at which a
    block takes K >= 3 (tests/test_lossy_packed_gpu.py's way of getting a K that is not constant), three images, and ONE plain pass
    over them: computed once, never changed."""
    import irec
    from irec.models import Large2LevelVAE
    torch.manual_seed(11)
    images = (torch.rand(3, 3, SIZE, SIZE) - 0.5).cuda()
    sampler = irec.BeamSearchCoder(kl_per_partition=3., n_beams=10, extra_samples=1., block_size=BLOCK)
    for scale in LADDER:
        torch.manual_seed(3)
        m = Large2LevelVAE(level_1_filters=8, level_2_filters=4).cuda().eval()
        with torch.no_grad():
            for mod in (m.hyper_analysis_transform[-1], m._level_1_posterior_loc_combiner):
                mod.weight.mul_(scale)
                mod.bias.mul_(scale)
        (blob, off, recon), (K, idx, bpr) = m.compress_rec(images, SEED, sampler, return_pendings=True)
        print(f"head scale {scale}: K {K.min()}..{K.max()}")
        if K.max() >= 3:
            break
    assert K.max() >= 3 and K.min() != K.max() and bpr == [4, 103] == m.blocks_per_res(images.shape, BLOCK)
    back = m.decompress_rec(blob, off, SEED, tuple(images.shape), sampler)
    return {"model": m, "sampler": sampler, "images": images, "K": K, "idx": idx, "recon": recon, "back": back, "files": _files(blob, off)}


@pytest.mark.parametrize("g", (1, 4))
def test_two_level_model_batch_of_three(engine, g):
    from irec.io import segmented as SG
    s = _lossy()
    m, sampler, images = s["model"], s["sampler"], s["images"]
    shape = tuple(images.shape)
    blob_d, off_d, recon_d = m.compress_rec(images, SEED, sampler, rec_on_device=True, segment_blocks=g)
    (blob_h, off_h, recon_h), (K_h, idx_h, bpr) = m.compress_rec(images, SEED, sampler, segment_blocks=g, return_pendings=True)
    assert blob_d.is_cuda and isinstance(blob_h, np.ndarray) and np.array_equal(K_h, s["K"])
    assert _files(blob_d, off_d) == _files(blob_h, off_h) and torch.equal(recon_d, s["recon"]) and torch.equal(recon_h, s["recon"])
    assert all(SG.is_segmented(f) and SG.segment_blocks_of(f) == g for f in _files(blob_h, off_h))
    assert _files(blob_h, off_h) == [C.file_of(s["K"][i], s["idx"][i], bpr, g, m._max_index(sampler), seed=SEED, shape=(SIZE, SIZE, 3), block_size=BLOCK)
                                     for i in range(3)]
    for on_device, blob, off in ((True, blob_d, off_d), (False, blob_h, off_h), (False, blob_d, off_d)):
        back = m.decompress_rec(blob, off, SEED, shape, sampler, rec_on_device=on_device, segment_blocks=g)
        assert torch.equal(back, s["back"])                                               # the same pixels as the plain path
    # another segment size, a plain file read as a segmented one and the other way round: a status per image, no rows
    from irec.models import resnet_vae as R
    _, status = m.decompress_rec(blob_d, off_d, SEED, shape, sampler, rec_on_device=True, segment_blocks=g + 1, strict=False)
    assert status.tolist() == [R.STATUS_SEGMENTED + 2] * 3
    plain = torch.from_numpy(np.frombuffer(b"".join(s["files"]), dtype=np.uint8).copy()).cuda()
    plain_off = np.concatenate([[0], np.cumsum([len(f) for f in s["files"]])])
    _, status = m.decompress_rec(plain, plain_off, SEED, shape, sampler, rec_on_device=True, segment_blocks=g, strict=False)
    assert status.tolist() == [R.STATUS_SEGMENTED] * 3
    for on_device in (True, False):
        _, status = m.decompress_rec(blob_d if on_device else blob_h, off_h, SEED, shape, sampler, rec_on_device=on_device, strict=False, max_K=8)
        assert (status != 0).all()
    from irec.io import SymbolTables
    tables = SymbolTables(index_counts=np.ones(1 + m._max_index(sampler), dtype=np.int64))
    with pytest.raises(ValueError, match="default symbol models"):
        m.compress_rec(images, SEED, sampler, tables=tables, segment_blocks=g)


@pytest.mark.parametrize("g", (1, 4))
def test_two_level_model_one_image(engine, g, tmp_path):
    from irec import harness
    s = _lossy()
    m, sampler = s["model"], s["sampler"]
    image = s["images"][1:2]
    shape = tuple(image.shape)
    blob_p, off_p, recon_p = m.compress_rec(image, SEED, sampler)
    want = m.decompress_rec(blob_p, off_p, SEED, shape, sampler)
    blob_d, off_d, recon_d = m.compress_rec(image, SEED, sampler, rec_on_device=True, segment_blocks=g)
    blob_h, off_h, recon_h = m.compress_rec(image, SEED, sampler, segment_blocks=g)
    assert _files(blob_d, off_d) == _files(blob_h, off_h) and torch.equal(recon_d, recon_p) and torch.equal(recon_h, recon_p)
    assert torch.equal(m.decompress_rec(blob_d, off_d, SEED, shape, sampler, rec_on_device=True, segment_blocks=g), want)
    assert torch.equal(m.decompress_rec(blob_h, off_h, SEED, shape, sampler, segment_blocks=g), want)
    # the harness: NAME.recs beside NAME.rec, told apart by magic and never decoded together
    for on_device in (False, True):
        out = str(tmp_path / f"dev{int(on_device)}")
        rows = harness.compress_images_lossy(m, sampler, image, ["seg"], SEED, BLOCK, out, rec_on_device=on_device, segment_blocks=g)
        rows += harness.compress_images_lossy(m, sampler, image, ["plain"], SEED, BLOCK, out, rec_on_device=on_device)
        assert all(r["indices_recovered"] for r in rows)
        assert open(f"{out}/seg.recs", "rb").read() == _files(blob_h, off_h)[0] and open(f"{out}/plain.rec", "rb").read() == _files(blob_p, off_p)[0]
        images, rows = harness.decompress_images_lossy(m, sampler, [f"{out}/seg.recs", f"{out}/plain.rec"], rec_on_device=on_device)
        assert [r["status"] for r in rows] == [0, 0] and torch.equal(images[0], want[0]) and torch.equal(images[1], want[0])
        datas = [open(f"{out}/seg.recs", "rb").read(), open(f"{out}/plain.rec", "rb").read()]
        infos, groups = harness.rec_file_groups(datas)
        assert sorted(groups.values()) == [[0], [1]] and infos[0]["segment_blocks"] == g and "segment_blocks" not in infos[1]


@pytest.mark.parametrize("g", (1, 4))
def test_resnet_vae_two_residual_blocks(engine, g):
    """BidirectionalResNetVAE, two residual blocks on 32 x 32 images, 2048-dim latents in blocks of 300: seven blocks per residual block."""
    from test_decompress_device_gpu import _images, _model
    from irec.io import segmented as SG
    from irec.models import resnet_vae as R
    m = _model(2, coder_args={"block_size": 300})
    images = _images(3, 5)
    (blob_p, off_p, recon_p), (K, idx) = m.compress_rec(images, seed=SEED, return_pendings=True)
    want = m.decompress_rec(blob_p, off_p, SEED, images.shape)
    assert K.shape[1:] == (2, 7)
    print("K", int(K.min()), "..", int(K.max()))
    blob, off, recon = m.compress_rec(images, seed=SEED, segment_blocks=g)
    assert torch.equal(recon, recon_p)
    Kh, ih = K.cpu().numpy().reshape(3, 14), idx.cpu().numpy().reshape(3, 14, -1)
    S = m.residual_blocks[0].coder.n_samples
    host_blob, host_off = SG.encode_files_segmented(SEED, (32, 32, 3), 300, Kh, ih, S, [7, 7], g)    # the host coder's files
    assert _files(blob, off) == _files(host_blob, host_off)
    assert _files(blob, off) == [C.file_of(Kh[i], ih[i], (7, 7), g, S, seed=SEED, shape=(32, 32, 3), block_size=300) for i in range(3)]
    for seg in (g, None):
        assert torch.equal(m.decompress_rec_segmented(blob, off, SEED, images.shape, segment_blocks=seg), want)
    _, status = m.decompress_rec_segmented(blob, off, SEED, images.shape, segment_blocks=g + 1, strict=False)
    assert status.tolist() == [R.STATUS_SEGMENTED + 2] * 3
    _, status = m.decompress_rec(blob, off, SEED, images.shape, strict=False)                         # the plain reader refuses the files
    assert (status != 0).all()
    _, status = m.decompress_rec_segmented(blob_p, off_p, SEED, images.shape, segment_blocks=g, strict=False)
    assert status.tolist() == [R.STATUS_SEGMENTED] * 3
