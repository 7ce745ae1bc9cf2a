"""The sequential importance coder on the GPU (csrc/irec_gc.hip behind irec_gc_importance_encode / _decode) against the numpy
referee of its arithmetic contract (tests/gc_referee.py; tests/test_gc_importance_host.py pins that referee to the reference's
own outputs): indices and samples bit for bit -- NaN positions equal, finite values equal."""
import functools
import os

import numpy as np
import pytest
import torch

import gc_referee as R
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(GOLDEN_DIR, "refpy_gc_importance.npz"))
CELLS = [str(c) for c in GOLD["cells"]]
LN2 = np.log(2)


def _normal(oracle):
    @functools.lru_cache(maxsize=64)
    def normal(seed, count):
        return oracle.tf_random_normal(seed, count)
    return normal


def _coder(omega, bits, **kw):
    import irec
    return irec.GaussianCoder(kl_per_partition=omega, sampler=irec.ImportanceSampler(coding_bits=bits), **kw)


def _bits_for(S):
    return float(np.log2(S - 0.5))     # ceil(exp(bits * ln 2)) = S whatever the float32 rounding of the product


class _D:
    def __init__(self, loc, scale):
        self.loc, self.scale = loc, scale


def _cuda(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _same(a, b):
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def _referee_blocks(oracle, host, seed, S, omega, ratio=R.power_law):
    """One block per row of the [n, D] arrays -> (indices per row, samples [n, D])."""
    normal, idx, out = _normal(oracle), [], []
    for mq, sq, mp, sp in zip(*host):
        K = oracle.num_aux(oracle.block_kl(mq, sq, mp, sp), omega)
        i, z = R.encode_block(mq, sq, mp, sp, seed, S, K, normal, ratio)
        idx.append(i)
        out.append(z)
    return idx, np.stack(out)


@pytest.mark.parametrize("cell", CELLS)
def test_every_fixture_cell(engine, oracle, cell):
    g = np.load(os.path.join(GOLDEN_DIR, cell.split("__")[0] + ".npz"))
    omega, seed, bits = float(g["kl_per_partition"]), int(g["seed"]), float(GOLD[f"{cell}_bits"])
    coder = _coder(omega, bits)
    coder.table_steps = coder._max_K_hint = 16
    S = coder.sampler.n_samples()
    ql, qs, pl, ps = _cuda(*(g[k][None] for k in ("q_loc", "q_scale", "p_loc", "p_scale")))
    idx, z = coder.encode_block(_D(ql, qs), _D(pl, ps), seed)
    ridx, rz = _referee_blocks(oracle, [g[k][None] for k in ("q_loc", "q_scale", "p_loc", "p_scale")], seed, S, omega)
    assert z.is_cuda and z.shape == ql.shape
    assert [int(i) for i in idx] == ridx[0] == GOLD[f"{cell}_indices"].tolist()
    assert _same(z.cpu().numpy(), rz[0]) and _same(rz[0], GOLD[f"{cell}_sample"])
    keep = list(idx)
    dec = coder.decode_block(_D(pl, ps), idx, seed)
    assert idx == keep and dec.is_cuda and torch.equal(dec, z)


@pytest.mark.parametrize("D", [1000, 192])
def test_model_shaped_latents_in_one_call(engine, oracle, D):
    import latent_families as lf
    host = lf.stack(lf.mixed(D, 5, 3.0, max_K=24))
    coder = _coder(3., 3. / LN2)
    S = coder.sampler.n_samples()
    assert S == 21
    ql, qs, pl, ps = _cuda(*host)
    idx, z = coder.encode(_D(ql, qs), _D(pl, ps), 17, batched=True)
    ridx, rz = _referee_blocks(oracle, host, 17, S, 3.0)
    assert len({len(i) for i in ridx}) > 3                   # the call mixes partition counts
    assert [[int(v) for v in ix] for ix in idx] == ridx
    assert _same(z.cpu().numpy(), rz)
    assert torch.equal(coder.decode(_D(pl, ps), idx, 17, batched=True), z)


def _rvae_batch(oracle, n):
    stats = [oracle.synthetic_latent(500 + i, 8192) for i in range(n)]
    return [np.stack([s[j] for s in stats]).reshape(n, 16, 16, 32) for j in range(4)]


def test_batch_of_64_rvae_shaped_tensors(engine, oracle):
    """576 blocks of two dims (1000 and 192) in one launch."""
    host = _rvae_batch(oracle, 64)
    coder = _coder(3., 3. / LN2, block_size=1000)
    ql, qs, pl, ps = _cuda(*host)
    idx, z = coder.encode(_D(ql, qs), _D(pl, ps), 42, batched=True)
    assert len(idx) == 64 and all(len(b) == 9 for b in idx) and z.shape == ql.shape
    zh = z.cpu().numpy()
    for i in range(64):
        ridx, rz = R.encode_tensor(*(h[i] for h in host), 42, 21, 3.0, 1000, _Cached(oracle))
        assert [[int(v) for v in ix] for ix in idx[i]] == ridx, i
        assert _same(zh[i], rz), i
    assert torch.equal(coder.decode(_D(pl, ps), idx, 42, batched=True), z)


class _Cached:
    """The oracle with its normal stream memoised (every block of a call reads the same draws)."""

    def __init__(self, oracle):
        self._o, self.tf_random_normal = oracle, _normal(oracle)

    def __getattr__(self, name):
        return getattr(self._o, name)


def _tensor_fixture():
    g = np.load(os.path.join(GOLDEN_DIR, "tensor_rvae_cfg2.npz"))
    return g, [g[k] for k in ("q_loc", "q_scale", "p_loc", "p_scale")], float(g["kl_per_partition"]), int(g["seed"]), int(g["block_size"])


def test_tensor_fixture_is_the_reference(engine):
    """GaussianCoder(.., block_size=1000).encode on GPU tensors returns the reference's committed outputs."""
    g, host, omega, seed, bs = _tensor_fixture()
    coder = _coder(omega, omega / LN2, block_size=bs)
    ql, qs, pl, ps = _cuda(*host)
    idx, z = coder.encode(_D(ql, qs), _D(pl, ps), seed)
    assert [[int(v) for v in ix] for ix in idx] == [GOLD["tensor_indices"][r, :k].tolist() for r, k in enumerate(GOLD["tensor_K"])]
    assert _same(z.cpu().numpy(), GOLD["tensor_sample"])
    dec = coder.decode(_D(pl, ps), idx, seed)
    assert torch.equal(dec, z) and _same(dec.cpu().numpy(), GOLD["tensor_decoded"])
    assert sum(coder.get_codelength(ix) for ix in idx) == pytest.approx(198.0, rel=1e-6)


@pytest.mark.parametrize("S", [5, 21, 64, 149, 404, 1024])
def test_every_sizing_of_the_kernel(engine, oracle, S):
    """One wave (S <= 64), several waves (S <= 1024) per block; 1024: the largest workgroup."""
    g, host, omega, seed, bs = _tensor_fixture()
    coder = _coder(omega, _bits_for(S), block_size=bs)
    coder.table_steps = coder._max_K_hint = 16
    assert coder.sampler.n_samples() == S
    ql, qs, pl, ps = _cuda(*host)
    idx, z = coder.encode(_D(ql, qs), _D(pl, ps), seed)
    ridx, rz = R.encode_tensor(*host, seed, S, omega, bs, _Cached(oracle))
    assert [[int(v) for v in ix] for ix in idx] == ridx
    assert _same(z.cpu().numpy(), rz)
    assert torch.equal(coder.decode(_D(pl, ps), idx, seed), z)


def test_more_samples_than_lanes(engine, oracle):
    """S = 1500 > 1024: a lane owns two samples."""
    g = np.load(os.path.join(GOLDEN_DIR, "block_D192_cfg2.npz"))
    host = [g[k][None] for k in ("q_loc", "q_scale", "p_loc", "p_scale")]
    coder = _coder(float(g["kl_per_partition"]), _bits_for(1500))
    coder.table_steps = coder._max_K_hint = 8
    ql, qs, pl, ps = _cuda(*host)
    idx, z = coder.encode_block(_D(ql, qs), _D(pl, ps), 3)
    ridx, rz = _referee_blocks(oracle, host, 3, 1500, float(g["kl_per_partition"]))
    assert [int(i) for i in idx] == ridx[0] and _same(z.cpu().numpy(), rz[0])


def test_window_smaller_than_K_is_coded_again(engine):
    from irec.coding.beam_search_coder import MorePartitionsNeeded
    g, host, omega, seed, bs = _tensor_fixture()
    coder = _coder(omega, omega / LN2, block_size=bs)
    coder.table_steps = coder._max_K_hint = 4
    ql, qs, pl, ps = _cuda(*host)
    pending, _ = coder.encode(_D(ql, qs), _D(pl, ps), seed, defer=True)
    with pytest.raises(MorePartitionsNeeded) as e:
        pending.to_lists()
    assert e.value.need == 9 and coder._max_K_hint == 9
    coder._max_K_hint = 4
    idx, z = coder.encode(_D(ql, qs), _D(pl, ps), seed)
    assert [[int(v) for v in ix] for ix in idx] == [GOLD["tensor_indices"][r, :k].tolist() for r, k in enumerate(GOLD["tensor_K"])]
    assert _same(z.cpu().numpy(), GOLD["tensor_sample"])


def test_zero_kl_block_and_mixed_rows(engine, oracle):
    """q == p in one tensor of a batch: K = 0 reads back as one index, 0 for this seed (the reference's output)."""
    g = np.load(os.path.join(GOLDEN_DIR, "block_D192_cfg0.npz"))
    ql = np.stack([g["p_loc"], g["q_loc"]]); qs = np.stack([g["p_scale"], g["q_scale"]])
    pl = np.stack([g["p_loc"], g["p_loc"]]); ps = np.stack([g["p_scale"], g["p_scale"]])
    coder = _coder(3., 3. / LN2)
    t = _cuda(ql, qs, pl, ps)
    idx, z = coder.encode(_D(t[0], t[1]), _D(t[2], t[3]), 42, batched=True)
    assert [int(v) for v in idx[0]] == GOLD["zero_kl_indices"].tolist() == [0]
    assert _same(z[0].cpu().numpy(), GOLD["zero_kl_sample"])
    ridx, rz = _referee_blocks(oracle, [ql, qs, pl, ps], 42, 21, 3.0)
    assert [[int(v) for v in ix] for ix in idx] == ridx and _same(z.cpu().numpy(), rz)
    assert torch.equal(coder.decode(_D(t[2], t[3]), idx, 42, batched=True), z)
    pending, _ = coder.encode(_D(t[0], t[1]), _D(t[2], t[3]), 42, batched=True, defer=True)
    from irec.coding.beam_search_coder import PendingCode
    K, packed = PendingCode.gather_packed([pending])
    assert K.shape == (2, 1, 1) and K[0, 0, 0] == 1 and packed[0, 0, 0, 0] == 0


def test_damaged_rows_decode_to_p_loc(engine):
    g, host, omega, seed, bs = _tensor_fixture()
    coder = _coder(omega, omega / LN2, block_size=bs)
    S = coder.sampler.n_samples()
    ql, qs, pl, ps = (t.reshape(1, -1) for t in _cuda(*host))
    lay = engine.layout(1, ql.numel(), bs, seed)
    K, idx, z = engine.gc_encode_blocks(lay, ql, qs, pl, ps, seed, omega, S, 12)
    good = engine.gc_decode_blocks(lay, pl, ps, seed, S, K, idx)
    assert torch.equal(good, z) and _same(z.cpu().numpy(), GOLD["tensor_sample"])
    Kb, ib = K.clone(), idx.clone()
    Kb[0], Kb[1], Kb[2] = -1, 13, 1000000
    ib[3, 1], ib[4, 0] = S, -1
    bad = engine.gc_decode_blocks(lay, pl, ps, seed, S, Kb, ib).cpu().numpy().reshape(-1)
    at = lay.element_index(np.arange(lay.n_blocks), 1000)
    want, plh = z.cpu().numpy().reshape(-1), pl.cpu().numpy().reshape(-1)
    for row in range(lay.n_blocks):
        e = at[row][at[row] >= 0]
        assert np.array_equal(bad[e], plh[e] if row < 5 else want[e]), row


def test_fitted_ratios_on_the_device(engine, oracle):
    from irec.coding.utils import CodingError
    g, host, omega, seed, bs = _tensor_fixture()
    ratios = np.array([1.0, 0.6, 0.45, 0.4, 0.33, 0.3, 0.25, 0.22, 0.2, 0.18], np.float32)
    coder = _coder(omega, omega / LN2, block_size=bs, extrapolate_auxiliary_ratios=False)
    coder.set_auxiliary_variance_ratios(ratios)
    ql, qs, pl, ps = _cuda(*host)
    idx, z = coder.encode(_D(ql, qs), _D(pl, ps), seed)
    ridx, rz = R.encode_tensor(*host, seed, 21, omega, bs, _Cached(oracle), ratio=lambda i: ratios[i])
    assert [[int(v) for v in ix] for ix in idx] == ridx and _same(z.cpu().numpy(), rz)
    assert torch.equal(coder.decode(_D(pl, ps), idx, seed), z)
    coder.set_auxiliary_variance_ratios(ratios[:8])                       # one block needs 9 partitions
    with pytest.raises(CodingError, match="KL divergence higher than auxiliary variables can account for.*Requested 9"):
        coder.encode(_D(ql, qs), _D(pl, ps), seed)


def test_cpu_tensors_and_other_samplers_take_the_host_path(engine):
    """Same outputs from both paths on the fixture: the device path is not a different coder."""
    g, host, omega, seed, bs = _tensor_fixture()
    coder = _coder(omega, omega / LN2, block_size=bs)
    cpu = [torch.from_numpy(h) for h in host]
    idx_h, z_h = coder.encode(_D(cpu[0], cpu[1]), _D(cpu[2], cpu[3]), seed)
    dev = _cuda(*host)
    idx_d, z_d = coder.encode(_D(dev[0], dev[1]), _D(dev[2], dev[3]), seed)
    assert not z_h.is_cuda and z_d.is_cuda
    assert [[int(v) for v in ix] for ix in idx_h] == [[int(v) for v in ix] for ix in idx_d]
    assert torch.equal(z_h, z_d.cpu())


def test_model_shim_with_the_importance_sampler(engine, tmp_path):
    import irec.io
    from irec.models import BidirectionalResNetVAE
    torch.manual_seed(0)
    m = BidirectionalResNetVAE(num_res_blocks=3, sampler="importance", sampler_args={"coding_bits": 3. / LN2, "alpha": np.inf},
                               coder_args={"block_size": 1000}, deterministic_filters=16, stochastic_filters=8, kl_per_partition=3.)
    with torch.no_grad():
        for b in m.residual_blocks:
            for head in (b.gen_posterior_loc_head, b.gen_posterior_log_scale_head, b.infer_posterior_loc_head,
                         b.infer_posterior_log_scale_head, b.prior_loc_head, b.prior_log_scale_head):
                head.weight.mul_(0.3)
        m._generative_base.normal_(0, 0.5)
    m = m.cuda().eval()
    S = m.residual_blocks[0].coder.sampler.n_samples()
    torch.manual_seed(1)
    image = torch.rand(1, 3, 64, 64, device="cuda") - 0.5
    block_indices, recon = m.compress(image, seed=42)
    assert len(block_indices) == 3 and all(len(ix) >= 1 for b in block_indices for ix in b)
    assert recon.shape == image.shape and torch.isfinite(recon).all()
    path = str(tmp_path / "image.rec")
    irec.io.write_compressed_code(path, 42, (64, 64, 3), 1000, block_indices, max_index=S)
    seed, shape, bs, read_back = irec.io.read_compressed_code(path)
    assert (seed, shape, bs) == (42, (64, 64, 3), 1000)
    assert read_back == [[[int(v) for v in ix] for ix in b] for b in block_indices]
    assert torch.equal(m.decompress(read_back, 42, image.shape), recon)
    # a batch, packed: the same indices for the same image
    images = torch.cat([image, torch.rand(2, 3, 64, 64, device="cuda") - 0.5])
    K, idx, _ = m.compress_packed(images, seed=42)
    assert K.shape[:2] == (3, 3) and K.min() >= 1
    assert [[idx[0, r, j, :K[0, r, j]].tolist() for j in range(K.shape[2])] for r in range(3)] == read_back


def test_tables_that_do_not_fit_send_gpu_tensors_to_the_host_loop(engine):
    """S = 4096 over a 4096-step window at 192 dims is 12 GB of tables, more than the library builds: the call runs the host loop
    on the GPU tensors (split / merge included), hands the sample back on the device, and says which path it took."""
    from irec.engine import NormalTableTooLarge, build_normal_table
    with pytest.raises(NormalTableTooLarge):
        build_normal_table(1, 4096, 192, 4096)
    g = np.load(os.path.join(GOLDEN_DIR, "block_D192_cfg0.npz"))
    host = [g[k][None] for k in ("q_loc", "q_scale", "p_loc", "p_scale")]
    cpu = [torch.from_numpy(h) for h in host]
    for block_size in (None, 100):
        coder = _coder(float(g["kl_per_partition"]), 12.0, block_size=block_size)
        coder.table_steps = coder._max_K_hint = 4096
        ql, qs, pl, ps = _cuda(*host)
        idx, z = coder.encode(_D(ql, qs), _D(pl, ps), 5)
        assert coder.last_path == "host" and z.is_cuda and z.shape == ql.shape
        dec = coder.decode(_D(pl, ps), idx, 5)
        assert coder.last_path == "host" and dec.is_cuda and torch.equal(dec, z)
        idx_h, z_h = coder.encode(_D(cpu[0], cpu[1]), _D(cpu[2], cpu[3]), 5)
        assert idx == idx_h and torch.equal(z.cpu(), z_h)
        coder.table_steps = coder._max_K_hint = 16              # the same call within the limit: the kernels, same outputs
        idx_d, z_d = coder.encode(_D(ql, qs), _D(pl, ps), 5)
        assert coder.last_path == "device"
        assert [[int(v) for v in ix] for ix in ([idx_d] if block_size is None else idx_d)] == \
               [[int(v) for v in ix] for ix in ([idx] if block_size is None else idx)]
        assert torch.equal(z_d, z)


def test_a_block_beyond_the_table_window_takes_the_host_loop(engine, oracle):
    """K = 5000 > IREC_TABLE_STEPS_MAX: the device call is not repeated for ever; the host loop codes the block."""
    mp = np.zeros((1, 3), np.float32)
    sp = np.ones((1, 3), np.float32)
    mq = np.full((1, 3), 100.0, np.float32)                 # 0.5 * 100^2 nats a dim: 15 000 nats, K = 5000 at Omega = 3
    K = oracle.num_aux(oracle.block_kl(mq[0], sp[0], mp[0], sp[0]), 3.0)
    assert K == 5000
    coder = _coder(3., 3. / LN2)
    ql, qs, pl, ps = _cuda(mq, sp, mp, sp)
    idx, z = coder.encode_block(_D(ql, qs), _D(pl, ps), 9)
    assert coder.last_path == "host" and len(idx) == K and z.is_cuda and coder._max_K_hint <= coder.DEVICE_MAX_K
    idx_h, z_h = coder.encode_block(_D(*map(torch.from_numpy, (mq, sp))), _D(*map(torch.from_numpy, (mp, sp))), 9)
    assert idx == idx_h and _same(z.cpu().numpy(), z_h.numpy())
    g = np.load(os.path.join(GOLDEN_DIR, "block_D192_cfg0.npz"))     # and the coder is back on the kernels for the next block
    t = _cuda(*(g[k][None] for k in ("q_loc", "q_scale", "p_loc", "p_scale")))
    idx2, _ = coder.encode_block(_D(t[0], t[1]), _D(t[2], t[3]), int(g["seed"]))
    assert coder.last_path == "device" and [int(i) for i in idx2] == GOLD["block_D192_cfg0__omega_indices"].tolist()
