"""Model call-surface shim: constructor surface on CPU; on the GPU the sequential res-block <->
coder hand-off, checked in situ against the oracle and by a compress -> decompress round trip."""
import inspect

import numpy as np
import pytest
import torch
import torch.nn.functional as F


def _model(device="cpu", blocks=3, det=16, sto=8):
    from irec.models import BidirectionalResNetVAE
    torch.manual_seed(0)
    m = BidirectionalResNetVAE(num_res_blocks=blocks, sampler="beam_search",
                               sampler_args={"n_beams": 20, "extra_samples": 1.2}, coder_args={"block_size": 1000},
                               deterministic_filters=det, stochastic_filters=sto, kl_per_partition=3.)
    with torch.no_grad():   # random-init weights (no checkpoints exist); keep posteriors close to priors so K stays small
        for b in m.residual_blocks:
            for head in (b.gen_posterior_loc_head, b.gen_posterior_log_scale_head, b.infer_posterior_loc_head,
                         b.infer_posterior_log_scale_head, b.prior_loc_head, b.prior_log_scale_head):
                head.weight.mul_(0.3)
        m._generative_base.normal_(0, 0.5)
    return m.to(device).eval()


def test_constructor_surface_matches_reference():
    from irec.models import BidirectionalResNetVAE, BidirectionalResidualBlock, ModelError
    blk = list(inspect.signature(BidirectionalResidualBlock.__init__).parameters)
    assert blk[1:6] == ["stochastic_filters", "deterministic_filters", "sampler", "sampler_args", "coder_args"]
    assert {"kernel_size", "is_last", "kl_per_partition", "name"} <= set(blk)
    vae = list(inspect.signature(BidirectionalResNetVAE.__init__).parameters)
    assert vae[1:5] == ["num_res_blocks", "sampler", "sampler_args", "coder_args"]
    assert {"first_kernel_size", "first_strides", "deterministic_filters", "stochastic_filters", "kl_per_partition"} <= set(vae)
    assert list(inspect.signature(BidirectionalResNetVAE.compress).parameters) == ["self", "image", "seed", "update_sampler"]
    m = _model()
    assert [b.is_last for b in m.residual_blocks] == [True, False, False]
    assert m.residual_blocks[0].coder.n_samples == 36 and m.residual_blocks[0].coder.block_size == 1000
    assert m.residual_blocks[2].coder.name == "encoder_for_resnet_block_2"
    with pytest.raises(ModelError, match="Sampler must be one of"):
        BidirectionalResNetVAE(num_res_blocks=1, sampler="nope")
    with pytest.raises(ModelError):
        BidirectionalResNetVAE(num_res_blocks=1, sampler="rejection")


@pytest.mark.gpu
def test_compress_decompress_round_trip_and_in_situ_parity(engine, oracle):
    m = _model("cuda")
    torch.manual_seed(1)
    image = (torch.rand(1, 3, 32, 32, device="cuda") - 0.5)
    # capture what each residual block hands to its coder
    seen = []
    for b in m.residual_blocks:
        orig = b.coder.encode

        def spy(target_dist, coding_dist, seed, _orig=orig, **kw):
            out = _orig(target_dist, coding_dist, seed, **kw)
            seen.append((target_dist.loc.clone(), target_dist.scale.clone(), coding_dist.loc.clone(),
                         coding_dist.scale.clone(), out))
            return out
        b.coder.encode = spy
    block_indices, recon = m.compress(image, seed=42)
    assert len(block_indices) == 3 and all(len(bi) == 3 for bi in block_indices)      # 2048 dims -> 1000 + 1000 + 48
    assert recon.shape == image.shape and torch.isfinite(recon).all()
    assert len(seen) == 3
    for ql, qs, pl, ps, (pending, sample) in seen:                                     # NHWC, batch 1, as in the reference
        assert ql.shape == (1, 16, 16, 8)
        idx = pending.to_lists()[0]                                                    # compress defers the host copy
        ridx, rs = oracle.encode_tensor(ql.cpu().numpy(), qs.cpu().numpy(), pl.cpu().numpy(), ps.cpu().numpy(), 42, 3.0,
                                        36, 20, block_size=1000)
        assert idx == ridx
        assert np.array_equal(sample.cpu().numpy(), rs)
    for b in m.residual_blocks:
        del b.coder.encode
    recon2 = m.decompress(block_indices, seed=42, image_shape=image.shape)
    assert torch.equal(recon2, recon)                                                   # decoder reproduces the encoder's pass
    # sequential dependence: a different latent in block 0 changes the prior block 1 sees
    alt = [[list(ix) for ix in bi] for bi in block_indices]
    alt[0][0][0] = (alt[0][0][0] + 1) % 36
    assert not torch.equal(m.decompress(alt, seed=42, image_shape=image.shape), recon)


@pytest.mark.gpu
def test_lossy_two_level_compress_file_decompress(engine, tmp_path):
    # BASELINE config 4 settings (B = 10, Omega = 3, eps = 0 -> S = 20, block_size 1000, max_index 20) on a 128 x 192 crop:
    # level 2 = [1, 2, 3, 128] (768 dims, 1 block), level 1 = [1, 8, 12, 196] (18 816 dims, 19 blocks)
    import irec
    from irec.models import Large2LevelVAE
    torch.manual_seed(3)
    m = Large2LevelVAE().cuda().eval()
    with torch.no_grad():
        for mod in (m.analysis_transform[-1], m.hyper_analysis_transform[-1], m.hyper_synthesis_transform[-1],
                    m._prior_loc_head, m._prior_log_scale_head, m._level_1_posterior_loc_combiner,
                    m._level_1_posterior_log_scale_combiner):
            mod.weight.mul_(0.2)
    sampler = irec.BeamSearchCoder(kl_per_partition=3., n_beams=10, extra_samples=1., block_size=1000)
    image = torch.rand(128, 192, 3, device="cuda") - 0.5
    path = str(tmp_path / "kodak_crop.rec")
    seen = []                                     # what each of the two sequential sampler.encode calls was handed, and returned
    orig = sampler.encode

    def spy(target, coder, seed, **kw):
        out = orig(target, coder, seed, **kw)
        seen.append((target.loc.clone(), target.scale.clone(), coder.loc.clone(), coder.scale.clone(), out))
        return out
    sampler.encode = spy
    recon = m.compress(path, image, seed=42, sampler=sampler, block_size=1000, max_index=20)
    del sampler.encode
    from oracle import oracle as O
    assert [tuple(t[0].shape) for t in seen] == [(1, 2, 3, 128), (1, 8, 12, 196)]       # level 2 first, then level 1 (:359,394)
    for ql, qs, pl, ps, (idx, sample) in seen:                                            # in-situ parity with the oracle
        ridx, rs = O.encode_tensor(ql.cpu().numpy(), qs.cpu().numpy(), pl.cpu().numpy(), ps.cpu().numpy(), 42, 3.0, 20, 10,
                                   block_size=1000)
        assert idx == ridx and np.array_equal(sample.cpu().numpy(), rs)
    assert recon.shape == (1, 3, 128, 192) and torch.isfinite(recon).all()
    seed, shape, bs, block_indices = irec.io.read_compressed_code(path)
    assert (seed, shape, bs) == (42, (128, 192, 3), 1000)
    assert block_indices == [seen[0][4][0], seen[1][4][0]]                               # the file holds what the coder emitted
    assert [len(b) for b in block_indices] == [1, 19]
    assert m.level_1_posterior.loc.shape == (1, 8, 12, 196) and m.level_2_posterior.loc.shape == (1, 2, 3, 128)
    recon2 = m.decompress(path, sampler)
    assert torch.equal(recon2, recon)
    import os
    assert os.path.getsize(path) < 4000          # a few hundred indices, arithmetic coded


@pytest.mark.gpu
def test_batched_compress_equals_one_by_one_and_writes_rec(engine, oracle, tmp_path):
    """N images through every residual block together == the N = 1 path image by image (indices and reconstruction),
    each block's hand-off still the oracle's; the harness writes one .rec per image, reads it back and gathers the bits
    (compression_performance.py:350-375)."""
    import irec
    from irec import harness
    m = _model("cuda", blocks=4)
    torch.manual_seed(5)
    images = torch.rand(5, 3, 32, 32, device="cuda") - 0.5
    seen = []
    blk = m.residual_blocks[2]
    orig = blk.coder.encode

    def spy(target_dist, coding_dist, seed, **kw):
        out = orig(target_dist, coding_dist, seed, **kw)
        seen.append((target_dist.loc.clone(), target_dist.scale.clone(), coding_dist.loc.clone(), coding_dist.scale.clone(), out))
        return out
    blk.coder.encode = spy
    bi_batch, recon_batch = m.compress(images, seed=42)
    del blk.coder.encode
    assert len(bi_batch) == 5 and len(bi_batch[0]) == 4 and len(bi_batch[0][0]) == 3
    ql, qs, pl, ps, (pending, sample) = seen[0]
    assert ql.shape == (5, 16, 16, 8)
    lists = pending.to_lists()
    for i in (0, 3):                                                                   # in-situ oracle parity inside the batch
        ridx, rs = oracle.encode_tensor(ql[i].cpu().numpy(), qs[i].cpu().numpy(), pl[i].cpu().numpy(), ps[i].cpu().numpy(),
                                        42, 3.0, 36, 20, block_size=1000)
        assert lists[i] == ridx and np.array_equal(sample[i].cpu().numpy(), rs)
    for i in range(5):
        bi_one, recon_one = m.compress(images[i:i + 1], seed=42)
        assert bi_one == bi_batch[i]
        assert torch.allclose(recon_one[0], recon_batch[i], atol=1e-5, rtol=0)   # convolutions at batch 1 vs 5 may pick other kernels
    assert torch.allclose(m.decompress(bi_batch, seed=42, image_shape=images.shape), recon_batch, atol=1e-5, rtol=0)
    rows, all_bits, all_nats = harness.compress_sharded(m, images.cpu(), 42, 1000, str(tmp_path), batch=3)
    assert len(rows) == 5 and all(r["indices_recovered"] for r in rows)
    assert all_bits.tolist() == [r["comp_codelength"] for r in rows] and all(b > 0 for b in all_bits.tolist())
    s, shape, bs, bi_file = irec.io.read_compressed_code(str(tmp_path / "img_00003.rec"))
    assert (s, shape, bs) == (42, (32, 32, 3), 1000) and bi_file == bi_batch[3]
    assert rows[3]["n_indices"] == sum(len(ix) for b in bi_batch[3] for ix in b)
    # the per-image form of the driver (reference's write_compressed_code / read_compressed_code on nested lists): same rows
    rows_py = harness.compress_images(m, images, [f"py_{i}" for i in range(5)], 42, 1000, str(tmp_path), batch=3, packed=False)
    for a, b in zip(rows, rows_py):
        assert (a["comp_codelength"], a["n_indices"], a["indices_recovered"]) == (b["comp_codelength"], b["n_indices"], b["indices_recovered"])
    assert (tmp_path / "py_3.rec").read_bytes() == (tmp_path / "img_00003.rec").read_bytes()
    # the packed read-back itself
    K, idx, recon_p = m.compress_packed(images, seed=42)
    assert K.shape == (5, 4, 3) and torch.equal(recon_p, recon_batch)
    for i in range(5):
        assert [[idx[i, r, j, :K[i, r, j]].tolist() for j in range(3)] for r in range(4)] == bi_batch[i]


@pytest.mark.gpu
def test_handoff_kernels_against_plain_pytorch(engine):
    """csrc/irec_shim.hip (statistics + exp in NHWC, concat + ELU, residual + ELU, each with the producing convolution's bias
    folded in) against the plain PyTorch float32 ops they replace (rec/models/resnet_vae.py:385-496); tolerance 2e-6 relative:
    HIP's expf / expm1f and PyTorch's differ in the last place, everything else is the same IEEE operation."""
    from irec.models.resnet_vae import _HandOff
    g = torch.Generator(device="cuda"); g.manual_seed(5)
    n, s, d, h, w = 3, 8, 20, 16, 16
    y = torch.randn((n, 4 * s + d, h, w), generator=g, device="cuda")
    yi = torch.randn((n, 2 * s + d, h, w), generator=g, device="cuda")
    by, bi = torch.randn(4 * s + d, generator=g, device="cuda"), torch.randn(2 * s + d, generator=g, device="cuda")
    lat = torch.randn((n, h, w, s), generator=g, device="cuda")
    yb, yib = y + by.reshape(1, -1, 1, 1), yi + bi.reshape(1, -1, 1, 1)

    def close(a, b):
        return torch.allclose(a, b, rtol=2e-6, atol=1e-7)
    want = yb[:, :4 * s].clone()
    want[:, 2 * s:] += yib[:, :2 * s]
    want = want.view(n, 4, s, h, w).permute(1, 0, 3, 4, 2).contiguous()
    want[1::2] = want[1::2].exp()
    got = _HandOff.stats(y, yi, s, 4, by, bi)
    assert got.shape == (4, n, h, w, s) and close(got, want)
    assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2])          # the locs are exact
    assert torch.equal(_HandOff.stats(y, None, s, 2, by), got[:2])                # the decoder's prior: the encoder's bits
    assert close(_HandOff.stats(y, yi, s, 4), (lambda t: torch.cat([t[:1], t[1:2].exp(), t[2:3], t[3:4].exp()]))(
        (torch.cat([y[:, :2 * s], y[:, 2 * s:4 * s] + yi[:, :2 * s]], 1)).view(n, 4, s, h, w).permute(1, 0, 3, 4, 2).contiguous()))
    want = F.elu(torch.cat([yb[:, 4 * s:], lat.permute(0, 3, 1, 2)], dim=1))
    assert close(_HandOff.cat_elu(y, 4 * s, d, lat, by), want)
    assert close(_HandOff.cat_elu(yi, 2 * s, d, None, bi), F.elu(yib[:, 2 * s:]))
    inp, t, bt = torch.randn((n, d, h, w), generator=g, device="cuda"), torch.randn((n, d, h, w), generator=g, device="cuda"), torch.randn(d, generator=g, device="cuda")
    out, out_elu = _HandOff.residual_elu(inp, t, 0.1, bt)
    want = torch.add(inp, t + bt.reshape(1, -1, 1, 1), alpha=0.1)
    assert close(out, want) and close(out_elu, F.elu(want))
    out2, _ = _HandOff.residual_elu(inp, t, 0.1)
    assert close(out2, torch.add(inp, t, alpha=0.1))


# ---- the hand-off kernels at the shapes and values the test above leaves out ---------------------------------------------------------------
SHIM_VALUES = [0.0, -0.0, -1e-8, -1e-4, -20.0, -100.0, np.inf, -np.inf, np.nan]
SHIM_LOG_SCALE_VALUES = [88.0, 89.0]          # expf is finite / overflows
SHIM_GRID_CAP = 4096 * 256                    # shim_grid (csrc/irec_shim.hip:81): at most 4096 workgroups of 256 threads, then the loop strides
# smallest n at s = 8, d = 20, hw = 4096 whose element count exceeds the cap: 4 * n * hw * s (four statistics), n * (d + s) * hw, n * d * hw
SHIM_WRAP_N = {"stats": 9, "cat_elu": 10, "residual_elu": 13}


def _plant(rng, arr, values, where=None):
    """Plant `values` at distinct random positions of arr (where: boolean mask of the positions allowed); -> boolean mask of the plants."""
    flat = arr.reshape(-1)
    allowed = np.flatnonzero(np.ones(flat.size, bool) if where is None else np.broadcast_to(where, arr.shape).reshape(-1))
    at = rng.permutation(allowed)[:len(values)]
    flat[at] = np.asarray(values[:at.size], dtype=np.float32)
    mask = np.zeros(flat.size, bool)
    mask[at] = True
    return mask.reshape(arr.shape)


def _ref_elu(v):
    """tf.nn.elu of float32 values: expm1 in float64, rounded once."""
    with np.errstate(all="ignore"):
        return np.where(v > 0, v, np.expm1(v.astype(np.float64)).astype(np.float32)).astype(np.float32)


def _ref_exp(v):
    with np.errstate(all="ignore"):
        return np.exp(v.astype(np.float64)).astype(np.float32)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def _shim_close(got, want, planted, what):
    """rtol 2e-6 (the tolerance of the test above: expf / expm1f differ from the float64 function in the last places), atol 1e-7 as
    there -- but atol 0 where a planted value went in: at x = -1e-8 an atol of 1e-7 would accept exp(x) - 1 in place of expm1(x).
    NaN and infinities must match in kind and sign."""
    assert got.shape == want.shape == planted.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN positions")
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf]), (what, "infinities")
    fin = ~(nan | inf)
    assert np.isfinite(got[fin]).all(), (what, "an infinity where the reference is finite")
    g, w = got[fin].astype(np.float64), want[fin].astype(np.float64)
    err, tol = np.abs(g - w), 2e-6 * np.abs(w) + np.where(planted[fin], 0.0, 1e-7)
    rel = err / np.maximum(np.abs(w), np.finfo(np.float32).tiny)
    print(f"{what}: {int(fin.sum())} finite, max rel err {rel.max() if rel.size else 0:.3e}, on planted {rel[planted[fin]].max() if planted[fin].any() else 0:.3e}")
    bad = np.flatnonzero(err > tol)
    assert not bad.size, (what, bad.size, g[bad[:5]].tolist(), w[bad[:5]].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("biased", [False, True], ids=["bias NULL", "bias set"])
@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (3, 8, 20, 255), "wrap"], ids=["1x1x1x1", "3x8x20x255", "grid-stride wrap"])
def test_handoff_kernels_shapes_and_planted_values(engine, shape, biased):
    """csrc/irec_shim.hip through the C ABI, operands and outputs in a canary arena (tests/guarded.py), against a float64 reference on the
    CPU: the float32 additions are the kernels' own IEEE operations in the kernels' order (an exp of a sum that was formed in float64
    would differ from one formed in float32 by |x| * 6e-8, more than the tolerance at x = 88), the transcendental -- expm1 for the ELU,
    exp for the scales -- is evaluated in float64 and rounded to float32 once.  `out` of the residual kernel is one multiply-add: either
    IEEE evaluation of it (fused or not) is accepted, bit for bit."""
    import ctypes
    import guarded as G
    from irec import _lib
    lib, F32 = engine.lib, torch.float32
    rng = np.random.default_rng(77)
    wrap = shape == "wrap"
    n0, s, d, hw = (None, 8, 20, 4096) if wrap else shape
    if wrap:
        for per_n, n_w in ((4 * hw * s, SHIM_WRAP_N["stats"]), ((d + s) * hw, SHIM_WRAP_N["cat_elu"]), (d * hw, SHIM_WRAP_N["residual_elu"])):
            assert (n_w - 1) * per_n <= SHIM_GRID_CAP < n_w * per_n
    f32 = lambda *sh: rng.standard_normal(sh).astype(np.float32)
    P = lambda t: t.data_ptr() if t is not None else None
    stream = engine._stream()

    # ---- irec_shim_stats: four statistics, and two with infer_heads = NULL
    n = SHIM_WRAP_N["stats"] if wrap else n0
    Cy, Ci = 4 * s + d, 2 * s + d
    y, yi, by, bi = f32(n, Cy, hw), f32(n, Ci, hw), f32(Cy), f32(Ci)
    log_y = np.zeros((1, Cy, 1), bool); log_y[:, s:2 * s] = True; log_y[:, 3 * s:4 * s] = True
    log_i = np.zeros((1, Ci, 1), bool); log_i[:, s:2 * s] = True
    my = _plant(rng, y, SHIM_VALUES) | _plant(rng, y, SHIM_LOG_SCALE_VALUES, log_y)
    mi = _plant(rng, yi, SHIM_VALUES) | _plant(rng, yi, SHIM_LOG_SCALE_VALUES, log_i)
    pair = my[:, 2 * s:4 * s] & (rng.random((n, 2 * s, hw)) < 0.5)          # half of y's plants meet a zero on the inference side
    yi[:, :2 * s][pair] = 0.0
    mi[:, :2 * s] |= pair
    mby, mbi = _plant(rng, by, SHIM_VALUES), _plant(rng, bi, SHIM_VALUES)
    if not biased:
        by = bi = None
    with np.errstate(all="ignore"):
        vy = y + by.reshape(1, -1, 1) if biased else y.copy()
        vi = yi + bi.reshape(1, -1, 1) if biased else yi.copy()
    py = my | (mby.reshape(1, -1, 1) if biased else False)
    pi = mi | (mbi.reshape(1, -1, 1) if biased else False)

    def stats_ref(n_stats):
        v, p = vy[:, :n_stats * s].copy(), py[:, :n_stats * s].copy()
        if n_stats == 4:
            with np.errstate(all="ignore"):
                v[:, 2 * s:] = v[:, 2 * s:] + vi[:, :2 * s]
            p[:, 2 * s:] |= pi[:, :2 * s]
        v = np.ascontiguousarray(v.reshape(n, n_stats, s, hw).transpose(1, 0, 3, 2))      # [k][n][hw][c]
        p = np.ascontiguousarray(p.reshape(n, n_stats, s, hw).transpose(1, 0, 3, 2))
        v[1::2] = _ref_exp(v[1::2])
        return v, p

    arena = G.Arena(G.slack(8) + 4 * (y.size + yi.size + Cy + Ci + 6 * n * hw * s), "cuda")
    dy, dyi = arena.put(y, name="y"), arena.put(yi, name="infer_heads")
    dby, dbi = (arena.put(by, name="bias_y"), arena.put(bi, name="bias_infer")) if biased else (None, None)
    out4 = arena.region(F32, (4, n, hw, s), "out", name="out (4 statistics)")
    out2 = arena.region(F32, (2, n, hw, s), "out", name="out (2 statistics)")
    arena.arm()
    _lib.check(lib.irec_shim_stats(engine.ctx, P(dy), P(dyi), P(out4), 4, n, Cy, Ci, s, hw, P(dby), P(dbi), stream), "irec_shim_stats")
    _lib.check(lib.irec_shim_stats(engine.ctx, P(dy), None, P(out2), 2, n, Cy, 0, s, hw, P(dby), None, stream), "irec_shim_stats (2)")
    torch.cuda.synchronize()
    arena.check()
    for out, n_stats in ((out4, 4), (out2, 2)):
        got, (want, planted) = out.cpu().numpy(), stats_ref(n_stats)
        _shim_close(got, want, planted, f"stats x{n_stats}")
        assert _same_bits(got[0::2], want[0::2]), n_stats                             # the locs are exact
    del arena

    # ---- irec_shim_cat_elu: slice + latent, and the slice alone
    n = SHIM_WRAP_N["cat_elu"] if wrap else n0
    y, by, lat = f32(n, Cy, hw), f32(Cy), f32(n, hw, s)
    my, mby, ml = _plant(rng, y, SHIM_VALUES, np.arange(Cy).reshape(1, -1, 1) >= 4 * s), _plant(rng, by[4 * s:], SHIM_VALUES), _plant(rng, lat, SHIM_VALUES)
    if not biased:
        by = None
    with np.errstate(all="ignore"):
        v = y[:, 4 * s:] + by[4 * s:].reshape(1, -1, 1) if biased else y[:, 4 * s:].copy()
    p = my[:, 4 * s:] | (mby.reshape(1, -1, 1) if biased else False)
    want_cat = _ref_elu(np.concatenate([v, lat.transpose(0, 2, 1)], axis=1))
    plant_cat = np.concatenate([np.broadcast_to(p, v.shape), ml.transpose(0, 2, 1)], axis=1)
    arena = G.Arena(G.slack(8) + 4 * (y.size + Cy + lat.size + 2 * n * (d + s) * hw), "cuda")
    dy, dlat = arena.put(y, name="y"), arena.put(lat, name="latent")
    dby = arena.put(by, name="bias_y") if biased else None
    out_cat = arena.region(F32, (n, d + s, hw), "out", name="out (cat)")
    out_slice = arena.region(F32, (n, d, hw), "out", name="out (slice)")
    arena.arm()
    _lib.check(lib.irec_shim_cat_elu(engine.ctx, P(dy), P(dlat), P(out_cat), n, Cy, 4 * s, d, s, hw, P(dby), stream), "irec_shim_cat_elu")
    _lib.check(lib.irec_shim_cat_elu(engine.ctx, P(dy), None, P(out_slice), n, Cy, 4 * s, d, 0, hw, P(dby), stream), "irec_shim_cat_elu (slice)")
    torch.cuda.synchronize()
    arena.check()
    _shim_close(out_cat.cpu().numpy(), want_cat, plant_cat, "cat_elu")
    _shim_close(out_slice.cpu().numpy(), want_cat[:, :d], plant_cat[:, :d], "cat_elu (slice)")
    del arena

    # ---- irec_shim_residual_elu
    n = SHIM_WRAP_N["residual_elu"] if wrap else n0
    inp, t, bt = f32(n, d, hw), f32(n, d, hw), f32(d)
    minp, mt, mbt = _plant(rng, inp, SHIM_VALUES), _plant(rng, t, SHIM_VALUES), _plant(rng, bt, SHIM_VALUES)
    t[minp] = 0.0                                                                     # inp's plants reach the ELU as they are (bias NULL)
    mt |= minp
    if not biased:
        bt = None
    alpha = np.float32(0.1)
    with np.errstate(all="ignore"):
        tv = t + bt.reshape(1, -1, 1) if biased else t.copy()
        unfused = (inp + (alpha * tv).astype(np.float32)).astype(np.float32)
        fused = (inp.astype(np.float64) + np.float64(alpha) * tv.astype(np.float64)).astype(np.float32)
    planted = minp | mt | (mbt.reshape(1, -1, 1) if biased else False)
    arena = G.Arena(G.slack(8) + 4 * (4 * inp.size + d), "cuda")
    dinp, dt = arena.put(inp, name="input"), arena.put(t, name="tensor")
    dbt = arena.put(bt, name="bias_tensor") if biased else None
    out, out_elu = arena.region(F32, (n, d, hw), "out", name="out"), arena.region(F32, (n, d, hw), "out", name="out_elu")
    arena.arm()
    _lib.check(lib.irec_shim_residual_elu(engine.ctx, P(dinp), P(dt), float(alpha), P(out), P(out_elu), n, d, hw, P(dbt), stream), "irec_shim_residual_elu")
    torch.cuda.synchronize()
    arena.check()
    got = out.cpu().numpy()
    which = [name for name, ref in (("fused", fused), ("unfused", unfused)) if _same_bits(got, ref)]
    print("residual_elu: out is the", which, "multiply-add;", int((fused != unfused).sum()), "elements tell them apart")
    assert which, "out is neither IEEE evaluation of inp + alpha * t"
    _shim_close(out_elu.cpu().numpy(), _ref_elu(got), np.broadcast_to(planted, got.shape), "residual_elu")


@pytest.mark.gpu
def test_graphed_compress_replays_the_whole_pass(engine):
    """The device side of compress (convolutions + 4 sequential coder launches, no host sync) captured as one HIP graph:
    same indices and reconstruction as the eager pass, for the capture image and for others replayed through it."""
    from irec.models import GraphedCompress
    m = _model("cuda", blocks=4)
    torch.manual_seed(9)
    images = torch.rand(3, 1, 3, 32, 32, device="cuda") - 0.5
    graphed = GraphedCompress(m, (1, 3, 32, 32), seed=42)
    for k in range(3):
        idx_e, rec_e = m.compress(images[k], seed=42)
        idx_g, rec_g = graphed(images[k])
        assert idx_g == idx_e and torch.equal(rec_g, rec_e), k
    assert graphed.graph is not None
    assert torch.equal(m.decompress(idx_g, seed=42, image_shape=images[2].shape), rec_g)


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [2, 3])
def test_graphed_compress_lanes_code_a_batch_side_by_side(engine, lanes):
    """A batch cut into independent sub-batches, each its own captured graph on its own stream with its own scratch (round
    3: a mid-size coder call is latency-bound, a second lane fills the device meanwhile): same indices and reconstruction,
    image for image, as the eager batched pass -- also for a second batch replayed through the same graphs."""
    from irec.models import GraphedCompress
    m = _model("cuda", blocks=4)
    torch.manual_seed(19)
    batches = torch.rand(2, 7, 3, 32, 32, device="cuda") - 0.5
    graphed = GraphedCompress(m, (7, 3, 32, 32), seed=42, lanes=lanes)
    assert graphed.lanes == lanes
    for k in range(2):
        idx_e, rec_e = m.compress(batches[k], seed=42)
        idx_g, rec_g = graphed(batches[k])
        assert idx_g == idx_e and torch.equal(rec_g, rec_e), k


@pytest.mark.gpu
def test_config3_harness_two_ranks_share_images(tmp_path):
    """scripts/config3_harness.py under torch.distributed.run with two ranks (gloo: both on the one GPU of the test box):
    image i goes to rank i mod 2, every rank compresses its share as one batch, writes / reads back its .rec files, and the
    per-image bits of ALL images are gathered on every rank."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env.update(IREC_DIST_BACKEND="gloo", TMPDIR=str(tmp_path))
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29617", os.path.join(root, "scripts", "config3_harness.py"),
                        "--images", "10", "--blocks", "3", "--singles", "1", "--no-graph"],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert res["images_this_rank"] == 5 and res["gathered_items"] == 10 and res["all_indices_recovered"] and res["errors"] == 0
    assert res["mean_bits_per_image"] > 0
