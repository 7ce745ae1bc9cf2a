"""GPU tests of the packed path of the two-level lossy model (Large2LevelVAE.compress_packed / compress_rec / decompress_packed /
decompress_rec, harness.compress_images_lossy / decompress_images_lossy) against the list path -- compress(file_path, ...) and
decompress(file_path, ...), the reference's surface -- on the smallest shapes where raggedness and tails are live:
Large2LevelVAE(level_1_filters=8, level_2_filters=4) on 128 x 64 images is 8 dims at level 2 and 256 at level 1, which a coder with
block_size = 5 cuts into blocks_per_res = [2, 52] with tails of 3 dims and 1 dim.  Files and indices are compared byte for byte and
integer for integer; pixels with torch.equal wherever the two sides run the same batch, and within 1e-5 between a batch of three and
images decompressed alone (the bound tests/test_decompress_device_gpu.py uses between two passes: batch size may change convolution
bits)."""
import functools
import math
import os

import numpy as np
import pytest
import torch

import rec_ragged_cases as C

pytestmark = pytest.mark.gpu

SEED, H, W, BLOCK = 42, 128, 64, 5
BPR = [2, 52]


def _beam():
    import irec
    return irec.BeamSearchCoder(kl_per_partition=3., n_beams=10, extra_samples=1., block_size=BLOCK)


def _importance():
    import irec
    return irec.GaussianCoder(kl_per_partition=3., sampler=irec.ImportanceSampler(coding_bits=3. / math.log(2.)), block_size=BLOCK)


CODERS = {"beam": _beam, "importance": _importance}


def _model(scale_2, scale_1):
    from irec.models import Large2LevelVAE
    torch.manual_seed(3)
    m = Large2LevelVAE(level_1_filters=8, level_2_filters=4).cuda().eval()
    with torch.no_grad():                         # the heads of the two posteriors' locs: a larger scale, a larger KL at that level
        for mod, scale in ((m.hyper_analysis_transform[-1], scale_2), (m._level_1_posterior_loc_combiner, scale_1)):
            mod.weight.mul_(scale)
            mod.bias.mul_(scale)
    return m


LADDER = (1., 4., 16., 64., 256., 1024., 4096.)


@functools.lru_cache(maxsize=None)
def _setup(kind):
    """The model with its head weights scaled until both levels hold a block with K >= 3 and K is not constant (level 2's head first,
    then level 1's: a step multiplies a KL by about 16, so the first scale that passes leaves K in the tens at most), the three images,
    and ONE packed pass over them (K, idx, reconstruction) with its files from the host coder: computed once, never changed."""
    from irec.io import encode_files_ragged
    torch.manual_seed(11)
    images = (torch.rand(3, 3, H, W) - 0.5).cuda()

    def attempt(scale_2, scale_1):
        m, sampler = _model(scale_2, scale_1), CODERS[kind]()
        K, idx, bpr, recon = m.compress_packed(images, SEED, sampler)
        print(f"{kind}: head scales {scale_2}, {scale_1}: level-2 K {K[:, :2].min()}..{K[:, :2].max()}, level-1 K {K[:, 2:].min()}..{K[:, 2:].max()}")
        return m, sampler, K, idx, bpr, recon

    scale_2 = next((s for s in LADDER if attempt(s, 1.)[2][:, :2].max() >= 3), None)
    assert scale_2 is not None, "no head scale gave level 2 a block with K >= 3"
    for scale_1 in LADDER:
        m, sampler, K, idx, bpr, recon = attempt(scale_2, scale_1)
        if K[:, 2:].max() >= 3:
            break
    assert K[:, :2].max() >= 3 and K[:, 2:].max() >= 3 and K.min() != K.max(), "no head scales gave both levels a block with K >= 3 and a K that is not constant"
    assert bpr == BPR == m.blocks_per_res(images.shape, BLOCK) and K.shape == (3, 54) and idx.shape[:2] == (3, 54)
    S = m._max_index(sampler)
    blob, off = encode_files_ragged(SEED, (H, W, 3), BLOCK, K, idx, S, bpr)
    for a in (K, idx, blob, off):
        a.setflags(write=False)
    return {"model": m, "sampler": sampler, "images": images, "K": K, "idx": idx, "recon": recon, "blob": blob, "off": off, "S": S}


def _files(blob, off):
    blob, off = (blob.cpu().numpy(), off.cpu().numpy()) if hasattr(blob, "cpu") else (blob, off)
    return [blob[off[i]:off[i + 1]].tobytes() for i in range(len(off) - 1)]


@pytest.mark.parametrize("kind", list(CODERS))
def test_compress_rec_files(engine, kind, tmp_path):
    """N = 3: the host coder's files equal the device coder's, byte for byte, and both equal write_compressed_code on the lists derived
    from compress_packed's arrays of the same pass."""
    from irec.io import write_compressed_code
    s = _setup(kind)
    m, sampler, images = s["model"], s["sampler"], s["images"]
    (blob_h, off_h, recon_h), (K_h, idx_h, bpr_h) = m.compress_rec(images, SEED, sampler, return_pendings=True)
    blob_d, off_d, recon_d = m.compress_rec(images, SEED, sampler, rec_on_device=True)
    assert isinstance(blob_h, np.ndarray) and blob_d.is_cuda and off_d.is_cuda
    assert np.array_equal(K_h, s["K"]) and bpr_h == BPR                                  # the same pass, coded again
    live = np.arange(idx_h.shape[2])[None, None, :] < K_h[..., None]
    assert np.array_equal(np.where(live, idx_h, 0), np.where(live, s["idx"], 0))
    assert torch.equal(recon_h, s["recon"]) and torch.equal(recon_d, s["recon"])
    want = []
    for i, lists in enumerate(C.lists_of(s["K"], s["idx"], BPR)):
        path = str(tmp_path / f"lists_{i}.rec")
        write_compressed_code(path, SEED, (H, W, 3), BLOCK, lists, s["S"])
        want.append(open(path, "rb").read())
        assert [len(rb) for rb in lists] == BPR
    assert _files(blob_h, off_h) == want and _files(blob_d, off_d) == want and _files(s["blob"], s["off"]) == want
    assert np.array_equal(off_d.cpu().numpy(), off_h)


def test_one_image_equals_the_list_path(engine, tmp_path):
    """N = 1: the file is the one compress(file_path, ...) writes and the reconstruction is its reconstruction; decompress_rec gives
    what decompress(file_path, sampler) gives."""
    s = _setup("beam")
    m, sampler = s["model"], s["sampler"]
    image = s["images"][1:2]
    path = str(tmp_path / "one.rec")
    recon_list = m.compress(path, image[0].permute(1, 2, 0).contiguous(), seed=SEED, sampler=sampler, block_size=BLOCK, max_index=s["S"])
    back_list = m.decompress(path, sampler)
    for on_device in (False, True):
        blob, off, recon = m.compress_rec(image, SEED, sampler, rec_on_device=on_device)
        assert _files(blob, off) == [open(path, "rb").read()]
        assert torch.equal(recon, recon_list)
        back = m.decompress_rec(blob, off, SEED, (1, 3, H, W), sampler, rec_on_device=on_device)
        assert torch.equal(back, back_list)
    K, idx, bpr, recon = m.compress_packed(image, SEED, sampler)
    assert torch.equal(recon, recon_list) and torch.equal(m.decompress_packed(K, idx, SEED, (1, 3, H, W), sampler), back_list)


@functools.lru_cache(maxsize=None)
def _decoded(kind):
    """decompress_rec on the host reader's rows, for the three images of _setup: computed once."""
    s = _setup(kind)
    return s["model"].decompress_rec(s["blob"], s["off"], SEED, (3, 3, H, W), s["sampler"])


@pytest.mark.parametrize("kind", list(CODERS))
def test_decompress_rec(engine, kind, tmp_path):
    s = _setup(kind)
    m, sampler = s["model"], s["sampler"]
    shape = (3, 3, H, W)
    host = _decoded(kind)
    dev = m.decompress_rec(torch.from_numpy(np.array(s["blob"])).cuda(), s["off"], SEED, shape, sampler, rec_on_device=True)
    dev_off = m.decompress_rec(torch.from_numpy(np.array(s["blob"])).cuda(), torch.from_numpy(np.array(s["off"])).cuda(), SEED, shape, sampler,
                               rec_on_device=True)
    packed = m.decompress_packed(s["K"], s["idx"], SEED, shape, sampler)
    assert host.shape == shape and torch.equal(host, dev) and torch.equal(host, dev_off) and torch.equal(host, packed)
    packed_dev, status = m.decompress_packed(torch.from_numpy(np.array(s["K"])).cuda(), torch.from_numpy(np.array(s["idx"])).cuda(), SEED, shape,
                                             sampler, strict=False)
    assert torch.equal(packed_dev, host) and not status.any()
    # each image alone through the list path
    for i, raw in enumerate(_files(s["blob"], s["off"])):
        path = str(tmp_path / f"alone_{i}.rec")
        with open(path, "wb") as fh:
            fh.write(raw)
        alone = m.decompress(path, sampler)
        err = float((alone[0] - host[i]).abs().max())
        print(f"{kind}: image {i}: max |alone - batch| = {err:.3g}")
        assert err <= 1e-5


def _damage(s, which):
    """The three files with file 1 damaged: (blob, offsets)."""
    files = _files(s["blob"], s["off"])
    if which == "truncated":
        files[1] = files[1][:len(files[1]) - 3]
    else:                                                       # the seed word
        files[1] = bytes([files[1][0] ^ 0x5A]) + files[1][1:]
    return np.frombuffer(b"".join(files), dtype=np.uint8), np.concatenate([[0], np.cumsum([len(f) for f in files])]).astype(np.int64)


@pytest.mark.parametrize("on_device", [False, True], ids=["host_reader", "device_reader"])
@pytest.mark.parametrize("which", ["truncated", "seed"])
def test_one_damaged_file_of_three(engine, which, on_device):
    from irec.coding import CodingError
    from irec.models.resnet_vae import STATUS_HEADER
    s = _setup("beam")
    m, sampler = s["model"], s["sampler"]
    good = _decoded("beam")
    blob, off = _damage(s, which)
    blob_in = torch.from_numpy(blob.copy()).cuda() if on_device else blob
    recon, status = m.decompress_rec(blob_in, off, SEED, (3, 3, H, W), sampler, strict=False, rec_on_device=on_device)
    assert status[0] == 0 and status[2] == 0
    if which == "truncated":
        assert 1 <= status[1] <= 18                             # an irec_rec_status: the reader's verdict
        assert status[1] in (8, 14, 15, 16)                     # truncated streams, or an index stream that no longer decodes
    else:
        assert status[1] == STATUS_HEADER
    assert torch.equal(recon[0], good[0]) and torch.equal(recon[2], good[2])
    with pytest.raises(CodingError, match=r"\(image 1\)"):
        m.decompress_rec(blob_in, off, SEED, (3, 3, H, W), sampler, strict=True, rec_on_device=on_device)


def test_an_index_out_of_range_in_one_image(engine):
    from irec import _lib
    from irec.coding import CodingError
    from irec.models.resnet_vae import STATUS_ROWS
    s = _setup("beam")
    m, sampler = s["model"], s["sampler"]
    good = _decoded("beam")
    K, idx = np.array(s["K"]), np.array(s["idx"])
    row = 2 + int(np.argmax(K[1, 2:]))                          # a level-1 row of image 1 that holds indices
    assert K[1, row] >= 1
    idx[1, row, 0] = s["S"]
    recon, status = m.decompress_packed(K, idx, SEED, (3, 3, H, W), sampler, strict=False)
    assert status.tolist() == [0, STATUS_ROWS + _lib.IREC_ROWS_E_INDEX_RANGE, 0]
    assert torch.equal(recon[0], good[0]) and torch.equal(recon[2], good[2])
    with pytest.raises(CodingError, match=r"index out of range.*\(image 1\)"):
        m.decompress_packed(K, idx, SEED, (3, 3, H, W), sampler)


def test_harness_round_trip(engine, tmp_path):
    import irec
    from irec import harness
    s = _setup("beam")
    m, sampler, images = s["model"], s["sampler"], s["images"]
    good = _decoded("beam")
    want = _files(s["blob"], s["off"])
    for on_device in (False, True):
        names = [f"{'dev' if on_device else 'host'}_{i}" for i in range(3)]
        rows = harness.compress_images_lossy(m, sampler, images, names, SEED, BLOCK, str(tmp_path), rec_on_device=on_device)
        assert [r["name"] for r in rows] == names and all(r["indices_recovered"] is True and r["n_indices"] > 0 for r in rows)
        assert [r["n_indices"] for r in rows] == s["K"].sum(axis=1).tolist()
        paths = [str(tmp_path / f"{nm}.rec") for nm in names]
        lists = C.lists_of(s["K"], s["idx"], BPR)
        for i, path in enumerate(paths):
            seed, shape, bs, blocks = irec.io.read_compressed_code(path)
            assert (seed, tuple(shape), bs) == (SEED, (H, W, 3), BLOCK) and blocks == lists[i]
            assert open(path, "rb").read() == want[i]
        pixels, drows = harness.decompress_images_lossy(m, sampler, paths, rec_on_device=on_device)
        assert torch.equal(pixels, good) and all(r["status"] == 0 for r in drows)
        # (batches of 2 and 1 against one batch of 3: convolution bits may differ with the batch size)
        pixels_b, _ = harness.decompress_images_lossy(m, sampler, paths, batch=2, rec_on_device=on_device)
        assert float((pixels_b - good).abs().max()) <= 1e-5
    # a truncated file among them: named, the others untouched
    with open(paths[1], "r+b") as fh:
        fh.truncate(os.path.getsize(paths[1]) - 3)
    pixels, drows = harness.decompress_images_lossy(m, sampler, paths, strict=False)
    assert [r["status"] != 0 for r in drows] == [False, True, False] and "error" in drows[1]
    assert torch.equal(pixels[0], good[0]) and torch.equal(pixels[2], good[2]) and not pixels[1].any()
    with pytest.raises(irec.coding.CodingError, match=r"\(image 1\)"):
        harness.decompress_images_lossy(m, sampler, paths)
