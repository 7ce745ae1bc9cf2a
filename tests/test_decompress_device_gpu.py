"""GPU tests of the device decompress path: .rec files -> irec.io's device reader -> every coder's row check and decode on rows that
never leave the device -> pixels, with one read-back (the per-image status).  The referee is the list path that stays
(read-back lists through model.decompress): same convolutions, bit-identical latents, so the comparisons are torch.equal; against
the compress pass the project's own bound for batched convolutions (1e-5, tests/test_models_shim.py) applies."""
import ctypes

import numpy as np
import pytest
import torch

import rec_device_cases as RC
import rows_status_cases as C

pytestmark = pytest.mark.gpu

SEED = 42


def _model(blocks=3, sampler="beam_search", sampler_args=None, coder_args=None, sto=8):
    """tests/test_models_shim.py's _model("cuda", blocks) with the sampler and the coder's arguments open: 32 x 32 images give
    2048-dim latents, blocks of 1000 + 1000 + 48 at block_size 1000."""
    from irec.models import BidirectionalResNetVAE
    torch.manual_seed(0)
    m = BidirectionalResNetVAE(num_res_blocks=blocks, sampler=sampler,
                               sampler_args=sampler_args or {"n_beams": 20, "extra_samples": 1.2},
                               coder_args={"block_size": 1000} if coder_args is None else coder_args,
                               deterministic_filters=16, stochastic_filters=sto, kl_per_partition=3.)
    with torch.no_grad():
        for b in m.residual_blocks:
            for head in (b.gen_posterior_loc_head, b.gen_posterior_log_scale_head, b.infer_posterior_loc_head,
                         b.infer_posterior_log_scale_head, b.prior_loc_head, b.prior_log_scale_head):
                head.weight.mul_(0.3)
        m._generative_base.normal_(0, 0.5)
    return m.cuda().eval()


def _images(n, seed, size=32):
    torch.manual_seed(seed)
    return torch.rand(n, 3, size, size, device="cuda") - 0.5


def _lists(K, idx, flat=False):
    """Packed arrays (numpy or device) as the nested lists model.decompress takes: [image][res_block][coder_block] (flat: no block
    level, the form of a coder without block_size)."""
    K, idx = (a.cpu().numpy() if hasattr(a, "cpu") else a for a in (K, idx))
    out = [[[idx[i, r, j, :K[i, r, j]].tolist() for j in range(K.shape[2])] for r in range(K.shape[1])] for i in range(K.shape[0])]
    if flat:
        out = [[blk[0] for blk in img] for img in out]
    return out[0] if K.shape[0] == 1 else out


def _round_trip(m, images, header_block_size=None, flat=False, host_files=None):
    """compress_rec -> decompress_rec against the list path and the compress pass; returns what the later checks reuse.
    host_files = S: the files come from compress_packed and the host writer instead (compress_rec is the beam-search coder's)."""
    if host_files:
        from irec.io import encode_files
        K, idx, recon = m.compress_packed(images, seed=SEED)
        blob, off = encode_files(SEED, (images.shape[2], images.shape[3], 3), 1000, K, idx, max_index=host_files)
        blob, K, idx = torch.from_numpy(np.array(blob)).cuda(), torch.from_numpy(K).cuda(), torch.from_numpy(idx).cuda()
    else:
        (blob, off, recon), (K, idx) = m.compress_rec(images, seed=SEED, block_size=header_block_size, return_pendings=True)
    out = m.decompress_rec(blob, off, SEED, images.shape)
    assert out.shape == images.shape and out.is_cuda
    assert torch.equal(out, m.decompress(_lists(K, idx, flat), seed=SEED, image_shape=images.shape))
    assert torch.allclose(out, recon, atol=1e-5, rtol=0)
    return blob, off, recon, K, idx, out


def test_round_trip_equals_the_list_path_and_the_compress_pass(engine):
    m = _model(3)
    images = _images(3, 1)
    blob, off, recon, K, idx, out = _round_trip(m, images)
    assert K.shape == (3, 3, 3) and int(K.sum()) > 0
    # strict=False: the same pixels and a clean status; max_K given or taken from the headers alike
    out2, status = m.decompress_rec(blob, off.cpu().numpy(), SEED, images.shape, max_K=int(K.max()), strict=False)
    assert torch.equal(out2, out) and status.dtype == np.int32 and status.tolist() == [0, 0, 0]
    # N = 1: the compress pass's own reconstruction, bit for bit (tests/test_models_shim.py:75)
    one = images[1:2]
    blob1, off1, recon1 = m.compress_rec(one, seed=SEED)
    assert torch.equal(m.decompress_rec(blob1, off1, SEED, one.shape), recon1)
    # a header that differs from the arguments is its own status, per image
    from irec.coding import CodingError
    from irec.models import resnet_vae as R
    _, status = m.decompress_rec(blob, off, SEED + 1, images.shape, strict=False)
    assert status.tolist() == [R.STATUS_HEADER] * 3
    with pytest.raises(CodingError, match=r"header.*\(image 0\)"):
        m.decompress_rec(blob, off, SEED + 1, images.shape)


def test_joined_views_give_the_bits_of_the_contiguous_form(engine):
    m = _model(3)
    images = _images(3, 2)
    (blob, off, recon), (Kv, iv) = m.compress_rec(images, seed=SEED, return_pendings=True)
    width = iv.shape[3]
    assert not iv.is_contiguous() and Kv.stride(2) == 1 + width and iv.stride(2) == 1 + width        # the views of the one joined tensor
    from irec.coding import GaussianCoder
    Kf, ks, If, ist = GaussianCoder._flat_rows(Kv, iv)
    assert (ks, ist) == (1 + width, 1 + width) and Kf.data_ptr() == Kv.data_ptr() and If.data_ptr() == iv.data_ptr()   # no copy for the check
    a = m.decompress_packed(Kv, iv, SEED, images.shape)
    b = m.decompress_packed(Kv.contiguous(), iv.contiguous(), SEED, images.shape)
    assert torch.equal(a, b) and torch.equal(a, m.decompress_rec(blob, off, SEED, images.shape))
    assert torch.allclose(a, recon, atol=1e-5, rtol=0)


def test_one_block_per_tensor(engine):
    m = _model(3, coder_args={"block_size": None})
    images = _images(2, 3)
    assert m.blocks_per_tensor(images.shape) == 1
    _, _, _, K, _, _ = _round_trip(m, images, header_block_size=2048, flat=True)
    assert K.shape == (2, 3, 1)


def test_block_wise_gather_where_whole_tensors_do_not_fit(engine):
    m = _model(3, coder_args={"block_size": 7})
    coder = m.residual_blocks[0].coder
    assert engine.lib.irec_decode_tensors_supported(ctypes.byref(coder._params()), 2048, 7) == 0      # 293 blocks a tensor: block-wise
    assert engine.lib.irec_decode_tensors_supported(ctypes.byref(coder._params()), 2048, 1000) == 1
    images = _images(2, 4)
    _, _, _, K, _, _ = _round_trip(m, images)
    assert K.shape == (2, 3, 293)


def test_importance_sampler_with_a_zero_kl_block(engine):
    m = _model(3, sampler="importance", sampler_args={"coding_bits": 3. / np.log(2.), "alpha": np.inf})
    b0 = m.residual_blocks[0]
    with torch.no_grad():       # block 0: posterior == prior, bit for bit (equal weights in one fused convolution, no inference share)
        for post, prior in ((b0.gen_posterior_loc_head, b0.prior_loc_head), (b0.gen_posterior_log_scale_head, b0.prior_log_scale_head)):
            post.weight.copy_(prior.weight); post.bias.copy_(prior.bias)
        for head in (b0.infer_posterior_loc_head, b0.infer_posterior_log_scale_head):
            head.weight.zero_(); head.bias.zero_()
    images = _images(2, 5)
    pendings, _ = m._compress_device(images, SEED)
    assert int(pendings[0].K.max()) == 0 and int(pendings[1].K.max()) >= 1        # zero KL in block 0: K = 0, and still one index each
    _, _, _, K, idx, _ = _round_trip(m, images, host_files=m.residual_blocks[0].coder.sampler.n_samples())
    assert (K[:, 0] == 1).all() and int(K.min()) == 1
    assert m.residual_blocks[0].coder.MIN_INDICES == 1 and m.residual_blocks[0].coder.last_path == "device"
    # a row without an index is refused by this coder (min_K = 1), where the beam-search coder decodes it
    from irec.models import resnet_vae as R
    K2 = K.contiguous().clone()
    K2[1, 2, 0] = 0
    _, status = m.decompress_packed(K2, idx.contiguous(), SEED, images.shape, strict=False)
    assert status.tolist() == [0, R.STATUS_ROWS + C.K_RANGE]


def _flip_that_the_reader_refuses(data, R, bpt, mk):
    """A byte of the index streams (the file's tail) whose flip the .rec reader refuses -- found with the reader's core on the CPU."""
    for at in range(len(data) - 1, 28 + 16 * R, -1):
        bad = data.copy()
        bad[at] ^= 0xFF
        st = int(RC.core_decode(bad, np.array([0, bad.size], dtype=np.int64), R, bpt, mk)[3][0])
        if st:
            return bad, st
    raise AssertionError("no byte flip of the index streams is refused")


def test_damaged_files_are_named_and_leave_the_others_alone(engine):
    from irec.coding import CodingError
    m = _model(3)
    images = _images(3, 6)
    blob, off, recon, K, idx, healthy = _round_trip(m, images)
    host, o = blob.cpu().numpy(), off.cpu().numpy()
    mk = int(K.max())
    files = [host[o[i]:o[i + 1]].copy() for i in range(3)]
    files[0] = files[0][:40]                                                       # truncated inside the dynamic header
    files[1], want1 = _flip_that_the_reader_refuses(files[1], 3, 3, mk)
    want0 = int(RC.core_decode(files[0], np.array([0, 40], dtype=np.int64), 3, 3, mk)[3][0])
    assert want0 == 4 and want1 != 0                                               # IREC_REC_E_TRUNCATED_HEADER
    off2 = np.concatenate([[0], np.cumsum([f.size for f in files])]).astype(np.int64)
    blob2 = torch.from_numpy(np.concatenate(files)).cuda()
    out, status = m.decompress_rec(blob2, off2, SEED, images.shape, max_K=mk, strict=False)
    assert status.tolist() == [want0, want1, 0]
    assert torch.equal(out[2], healthy[2])
    with pytest.raises(CodingError, match=r"truncated header \(image 0\)"):
        m.decompress_rec(blob2, off2, SEED, images.shape, max_K=mk)
    # offsets on the device that point outside the blob are clamped there: a refused file, no read outside
    wild = torch.tensor([0, int(off2[1]), 10 ** 12, -5], dtype=torch.int64, device="cuda")
    _, status = m.decompress_rec(blob2, wild, SEED, images.shape, max_K=mk, strict=False)
    assert status[0] == want0 and status[1] != 0 and status[2] != 0


def test_bad_rows_planted_on_the_device(engine):
    from irec.coding import CodingError
    from irec.models import resnet_vae as R
    m = _model(4)
    images = _images(3, 7)
    K, idx, _ = m.compress_packed(images, seed=SEED)
    S = m.residual_blocks[0].coder.n_samples
    Kd, idxd = torch.from_numpy(K).cuda(), torch.from_numpy(idx).cuda()
    healthy = m.decompress_packed(Kd, idxd, SEED, images.shape)
    Kb, ib = Kd.clone(), idxd.clone()
    Kb[1, 2, 0] = max(1, int(K[1, 2, 0]))
    ib[1, 2, 0, 0] = S                                                             # an index = S in image 1, residual block 2
    Kb[2, 0, 1] = idx.shape[3] + 1                                                 # K = max_K + 1 in image 2
    out, status = m.decompress_packed(Kb, ib, SEED, images.shape, strict=False)
    assert status.tolist() == [0, R.STATUS_ROWS + C.INDEX_RANGE, R.STATUS_ROWS + C.K_RANGE]
    assert torch.equal(out[0], healthy[0])
    with pytest.raises(CodingError, match=r"index out of range \[0, n_samples\) \(image 1\)"):
        m.decompress_packed(Kb, ib, SEED, images.shape)
    # fitted ratios and a short table: a count beyond it is the reference's error, not a K_RANGE
    from irec.coding.coder import AUX_RATIO_POWER_LAW
    mf = _model(4, coder_args={"block_size": 1000, "extrapolate_auxiliary_ratios": False})
    for b in mf.residual_blocks:
        b.coder.set_auxiliary_variance_ratios(np.power(np.arange(1., 5.), AUX_RATIO_POWER_LAW))
    Kf = torch.ones((3, 4, 3), dtype=torch.int32, device="cuda")
    If = torch.zeros((3, 4, 3, 8), dtype=torch.int32, device="cuda")
    ok, status = mf.decompress_packed(Kf, If, SEED, images.shape, strict=False)
    assert status.tolist() == [0, 0, 0]
    Kf[1, 1, 2] = 6                                                                # beyond the table of four ...
    Kf[1, 3, 0] = 9                                                                # ... and a later, larger count that is a K_RANGE
    out, status = mf.decompress_packed(Kf, If, SEED, images.shape, strict=False)
    assert status.tolist() == [0, R.STATUS_ROWS + C.RATIO_TABLE, 0] and torch.equal(out[0], ok[0]) and torch.equal(out[2], ok[2])
    with pytest.raises(CodingError, match=r"Maximum possible number of partitions is 4.Requested 6 \(image 1\)"):
        mf.decompress_packed(Kf, If, SEED, images.shape)


    # rows without an index slot are refused before any launch
    with pytest.raises(CodingError, match="no index slot"):
        mf.decompress_packed(Kf, If[..., :0], SEED, images.shape)


def test_device_row_check_equals_the_host_twin(engine):
    lib = engine.lib
    nonzero = 0
    for case in C.cases():
        got, want = C.device_status(lib, case, torch), C.host_status(lib, case)
        assert np.array_equal(got, want), (case["name"], case["plants"], got.tolist(), want.tolist())
        nonzero += int((want != 0).sum())
    assert nonzero > 1000


def test_graphed_decompress_replays_and_recaptures(engine):
    from irec.io import encode_files, rec_files_max_K
    from irec.models import GraphedDecompress
    m = _model(3)
    shape = (2, 3, 32, 32)
    batches = []
    for s in (11, 12, 13):
        blob, off, _ = m.compress_rec(_images(2, s), seed=SEED)
        batches.append((blob, off.cpu().numpy()))
    max_K = max(rec_files_max_K(b.cpu().numpy(), o) for b, o in batches)
    gd = GraphedDecompress(m, shape, SEED, R=3, bpt=3, max_K=max_K, blob_bytes=max(b.numel() for b, _ in batches))
    for blob, off in batches:
        eager = m.decompress_rec(blob, off, SEED, shape, max_K=max_K)
        assert torch.equal(gd(blob, off), eager)
    assert gd.captures == 1 and gd.graph is not None          # (the capture itself: no host synchronisation, no allocation outside the graph's pool)
    out, status = gd(batches[0][0], batches[0][1], strict=False)
    assert status.tolist() == [0, 0] and gd.captures == 1
    # a fourth batch with a longer row than the captured buffers hold: the eager path answers, and the next call captures again
    S = m.residual_blocks[0].coder.n_samples
    rng = np.random.default_rng(3)
    K4 = np.ones((2, 3, 3), dtype=np.int32)
    K4[1, 1, 0] = max_K + 3
    idx4 = rng.integers(0, S, size=(2, 3, 3, max_K + 3)).astype(np.int32)
    host4, off4 = encode_files(SEED, (32, 32, 3), 1000, K4, idx4, max_index=S)
    blob4 = torch.from_numpy(np.array(host4)).cuda()
    want4 = m.decompress_rec(blob4, off4, SEED, shape)
    assert torch.equal(gd(blob4, off4), want4)
    assert gd.graph is None and gd.max_K == max_K + 3 and gd.blob_bytes >= blob4.numel()
    assert torch.equal(gd(blob4, off4), want4) and gd.captures == 2
    # a damaged file that reports IREC_REC_E_MAX_K while its header asks for no more than the graph holds: eager, the graph is kept
    bad = np.array(host4)
    first = 28 + 12 * 3                                                            # file 0's max_partitions words: 1, 1, 1 -> 0, 0, 0
    assert bad[first:first + 12].view("<u4").tolist() == [1, 1, 1]
    bad[first:first + 12] = 0
    _, status = gd(torch.from_numpy(bad).cuda(), off4, strict=False)
    assert status[0] != 0 and status[1] == 0 and gd.graph is not None and gd.captures == 2
    assert torch.equal(gd(*batches[1]), m.decompress_rec(batches[1][0], batches[1][1], SEED, shape, max_K=max_K))


def test_driver_reads_what_the_driver_wrote(engine, tmp_path):
    from irec import harness
    m = _model(3)
    small, large = _images(3, 21), _images(2, 22, size=64)
    names_s, names_l = [f"s{i}" for i in range(3)], [f"l{i}" for i in range(2)]
    for images, names in ((small, names_s), (large, names_l)):
        rows = harness.compress_images(m, images, names, SEED, 1000, str(tmp_path), rec_on_device=True)
        assert all(r["indices_recovered"] for r in rows)
    recon_s, recon_l = m.compress_rec(small, seed=SEED)[2], m.compress_rec(large, seed=SEED)[2]
    paths = [str(tmp_path / f"{n}.rec") for n in names_s]
    out, rows = harness.decompress_images(m, paths)
    assert out.shape == (3, 3, 32, 32) and torch.allclose(out, recon_s, atol=1e-5, rtol=0)
    assert [r["name"] for r in rows] == [f"{n}.rec" for n in names_s] and all(r["status"] == 0 and r["seed"] == SEED for r in rows)
    # a file too short for its header: its own row, no image; strict names it by its place in the list
    short = tmp_path / "short.rec"
    short.write_bytes((tmp_path / "s0.rec").read_bytes()[:40])
    outs, rows = harness.decompress_images(m, [paths[0], str(short), paths[1]], strict=False)
    assert [r["status"] for r in rows] == [0, 4, 0] and outs[1] is None and "truncated header" in rows[1]["error"]
    assert torch.allclose(torch.stack([outs[0], outs[2]]), recon_s[:2], atol=1e-5, rtol=0)
    from irec.coding import CodingError
    with pytest.raises(CodingError, match=r"truncated header \(image 1\)"):
        harness.decompress_images(m, [paths[0], str(short), paths[1]])
    # a mixed list: grouped by shape, answered in the order given
    order = [("s", 0), ("l", 0), ("s", 1), ("l", 1), ("s", 2)]
    mixed = [str(tmp_path / f"{k}{i}.rec") for k, i in order]
    outs, rows = harness.decompress_images(m, mixed, batch=2)
    assert len(outs) == len(rows) == 5
    for (k, i), im, row in zip(order, outs, rows):
        want = (recon_s if k == "s" else recon_l)[i]
        assert im.shape == want.shape and torch.allclose(im, want, atol=1e-5, rtol=0), (k, i)
        assert row["name"] == f"{k}{i}.rec" and row["image_shape"] == ((32, 32, 3) if k == "s" else (64, 64, 3)) and row["status"] == 0
