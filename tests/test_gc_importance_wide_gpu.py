"""The sequential importance coder on the GPU for blocks of MORE than 1024 dims (gc_importance_encode_wide_kernel of
csrc/irec_gc.hip behind irec_gc_importance_encode_ws): against the reference's own outputs (tests/golden/refpy_gc_importance_wide.npz)
and the numpy referee of the arithmetic contract (tests/gc_referee.py; tests/test_gc_importance_wide_host.py pins that referee to
the reference on these blocks).  Indices and samples bit for bit -- NaN positions equal, finite values equal.

The kernel walks a block in chunks of 1024 dims and, up to S_pad = 1024, in LDS tiles of 8192 / S_pad dims; beyond that it takes
the plain lane-per-sample walk.  The shapes below sit on those edges: D = 1025, 1280 (one tile past the chunk at S_pad = 32), 2048,
2049; S = 1024 (the last tiled sizing, 8 dims a tile) and S = 1500 (plain walk, a lane owns two samples)."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import gc_referee as R
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(GOLDEN_DIR, "refpy_gc_importance_wide.npz"))
CELLS = [str(c) for c in GOLD["cells"]]
BLOCK_SIZES = [None if b < 0 else int(b) for b in GOLD["tensor_block_sizes"]]
KEYS = ("q_loc", "q_scale", "p_loc", "p_scale")
LN2 = np.log(2)


@functools.lru_cache(maxsize=8)
def _normal_of(seed, count):
    from oracle import oracle as O
    return O.tf_random_normal(seed, count)


class _Cached:
    """The oracle with its normal stream memoised (every block of a call reads the same draws)."""

    def __init__(self, oracle):
        self._o, self.tf_random_normal = oracle, _normal_of

    def __getattr__(self, name):
        return getattr(self._o, name)


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


def _lists(idx):
    return [[int(v) for v in ix] for ix in idx]


def _referee_blocks(oracle, host, seed, S, omega, ratio=R.power_law):
    """One block per row of the [n, D] arrays -> (indices per row, samples [n, D])."""
    idx, out = [], []
    for mq, sq, mp, sp in zip(*host):
        K = oracle.num_aux(oracle.block_kl(mq, sq, mp, sp), omega)
        i, z = R.encode_block(mq, sq, mp, sp, seed, S, K, _normal_of, ratio)
        idx.append(i)
        out.append(z)
    return idx, np.stack(out)


def _block(name, D=None):
    g = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    return [g[k][:D][None] for k in KEYS], float(g["kl_per_partition"]), int(g["seed"])


def _tensor_fixture():
    g = np.load(os.path.join(GOLDEN_DIR, "tensor_rvae_cfg2.npz"))
    return [g[k] for k in KEYS], float(g["kl_per_partition"]), int(g["seed"])


def _tensor_want(bs):
    tag = f"tensor_bs{bs}"
    return [GOLD[f"{tag}_indices"][r, :k].tolist() for r, k in enumerate(GOLD[f"{tag}_K"])], GOLD[f"{tag}_sample"], GOLD[f"{tag}_decoded"]


# 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", CELLS)
def test_every_wide_golden_cell(engine, oracle, cell):
    host, omega, seed = _block(cell.split("__")[0])
    coder = _coder(omega, float(GOLD[f"{cell}_bits"]))
    coder.table_steps = coder._max_K_hint = 26           # (K <= 25 on these cells: no longer a table than the cell reads)
    S = coder.sampler.n_samples()
    ql, qs, pl, ps = _cuda(*host)
    idx, z = coder.encode_block(_D(ql, qs), _D(pl, ps), seed)
    assert coder.last_path == "device"
    ridx, rz = _referee_blocks(oracle, host, seed, S, omega)
    assert z.is_cuda and z.shape == ql.shape
    assert [int(i) for i in idx] == ridx[0] == GOLD[f"{cell}_indices"].tolist()
    assert _same(z.cpu().numpy(), rz[0]) and _same(rz[0], GOLD[f"{cell}_sample"])
    keep = list(idx)
    dec = coder.decode_block(_D(pl, ps), idx, seed)
    assert coder.last_path == "device" and idx == keep and dec.is_cuda and torch.equal(dec, z)
    assert _same(dec.cpu().numpy(), GOLD[f"{cell}_decoded"])


# 2 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,K", [(1025, 8), (1280, 10), (2048, 16), (2049, 16)])
def test_chunk_and_tile_edges(engine, oracle, D, K):
    host, omega, seed = _block("block_D2500_large", D)
    coder = _coder(omega, _bits_for(21))
    coder.table_steps = coder._max_K_hint = 16
    ql, qs, pl, ps = _cuda(*host)
    idx, z = coder.encode_block(_D(ql, qs), _D(pl, ps), seed)
    assert coder.last_path == "device"
    ridx, rz = _referee_blocks(oracle, host, seed, 21, omega)
    assert len(ridx[0]) == K
    assert [int(i) for i in idx] == ridx[0] and _same(z.cpu().numpy(), rz[0])
    assert torch.equal(coder.decode_block(_D(pl, ps), idx, seed), z) and coder.last_path == "device"


# 3 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [5, 64, 149, 404, 1024, 1500])
def test_every_sizing_at_1025_dims(engine, oracle, S):
    """S <= 1024 (S_pad <= 1024): the tile form, 8192 / S_pad dims a tile -- 1024 is its last sizing.  S = 1500: the plain walk, and a
    lane owns two samples."""
    host, omega, seed = _block("block_D2500_large", 1025)
    coder = _coder(omega, _bits_for(S))
    coder.table_steps = coder._max_K_hint = 8
    assert coder.sampler.n_samples() == S
    ql, qs, pl, ps = _cuda(*host)
    idx, z = coder.encode_block(_D(ql, qs), _D(pl, ps), seed)
    assert coder.last_path == "device" and len(idx) == 8
    ridx, rz = _referee_blocks(oracle, host, seed, S, omega)
    assert [int(i) for i in idx] == ridx[0] and _same(z.cpu().numpy(), rz[0])
    assert torch.equal(coder.decode_block(_D(pl, ps), idx, seed), z)


# 4 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bs", BLOCK_SIZES)
def test_tensor_fixture_is_the_reference(engine, bs):
    """None: ONE block of 8192 dims, K = 62.  1500: five wide blocks and one of 692 dims in one call."""
    host, omega, seed = _tensor_fixture()
    want, sample, decoded = _tensor_want(bs)
    coder = _coder(omega, omega / LN2, block_size=bs)
    coder.table_steps = coder._max_K_hint = 64
    ql, qs, pl, ps = _cuda(*host)
    idx, z = coder.encode(_D(ql, qs), _D(pl, ps), seed)
    assert coder.last_path == "device"
    assert _lists([idx] if bs is None else idx) == want
    assert _same(z.cpu().numpy(), sample)
    dec = coder.decode(_D(pl, ps), idx, seed)
    assert coder.last_path == "device" and torch.equal(dec, z) and _same(dec.cpu().numpy(), decoded)


def test_tensor_fixture_batched(engine):
    """The fixture stacked three times at block_size 1500: 15 wide blocks and 3 narrow ones in one launch."""
    host, omega, seed = _tensor_fixture()
    want, sample, _ = _tensor_want(1500)
    coder = _coder(omega, omega / LN2, block_size=1500)
    ql, qs, pl, ps = _cuda(*(np.concatenate([h, h, h]) for h in host))
    idx, z = coder.encode(_D(ql, qs), _D(pl, ps), seed, batched=True)
    assert coder.last_path == "device" and len(idx) == 3
    for i in range(3):
        assert _lists(idx[i]) == want, i
        assert _same(z[i:i + 1].cpu().numpy(), sample), i
    assert torch.equal(coder.decode(_D(pl, ps), idx, seed, batched=True), z) and coder.last_path == "device"


# 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_model_shaped_latents_in_one_call(engine, oracle):
    import latent_families as lf
    host = lf.stack(lf.mixed(1500, 5, 3.0, max_K=24))
    coder = _coder(3., 3. / LN2)
    S = coder.sampler.n_samples()
    assert S == 21
    ql, qs, pl, ps = _cuda(*host)
    idx, z = coder.encode(_D(ql, qs), _D(pl, ps), 17, batched=True)
    assert coder.last_path == "device"
    ridx, rz = _referee_blocks(oracle, host, 17, S, 3.0)
    assert min(len(i) for i in ridx) == 1 and max(len(i) for i in ridx) >= 20        # the call mixes partition counts
    assert _lists(idx) == ridx
    assert _same(z.cpu().numpy(), rz)
    assert torch.equal(coder.decode(_D(pl, ps), idx, 17, batched=True), z)


# 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_window_smaller_than_K_is_coded_again(engine):
    from irec.coding.beam_search_coder import MorePartitionsNeeded
    cell = "block_D1500_large_b10__omega"
    host, omega, seed = _block("block_D1500_large_b10")
    coder = _coder(omega, omega / LN2)
    coder.table_steps = coder._max_K_hint = 4
    ql, qs, pl, ps = _cuda(*host)
    pending, _ = coder.encode(_D(ql, qs), _D(pl, ps), seed, defer=True)
    assert coder.last_path == "device"
    with pytest.raises(MorePartitionsNeeded) as e:
        pending.to_lists()
    assert e.value.need == 12 and coder._max_K_hint == 12
    coder._max_K_hint = 4
    idx, z = coder.encode(_D(ql, qs), _D(pl, ps), seed)
    assert coder.last_path == "device"
    assert [int(v) for v in idx] == GOLD[f"{cell}_indices"].tolist() and _same(z.cpu().numpy(), GOLD[f"{cell}_sample"])


def test_zero_kl_wide_block(engine, oracle):
    host, omega, seed = _block("block_D1500_large_b10")
    pl, ps = _cuda(host[2], host[3])
    coder = _coder(3., 3. / LN2)
    idx, z = coder.encode_block(_D(pl, ps), _D(pl, ps), 42)
    assert coder.last_path == "device" and len(idx) == 1
    ridx, rz = R.encode_block(host[2], host[3], host[2], host[3], 42, 21, 0, _normal_of)
    assert [int(v) for v in idx] == ridx and _same(z.cpu().numpy(), rz)
    assert torch.equal(coder.decode_block(_D(pl, ps), idx, 42), z)


def test_fitted_ratios_on_a_wide_call(engine, oracle):
    host, omega, seed = _tensor_fixture()
    ratios = np.power(np.arange(1, 17), -0.75).astype(np.float32)         # 16 partitions; the 1500-dim blocks need at most 12
    coder = _coder(omega, omega / LN2, block_size=1500, extrapolate_auxiliary_ratios=False)
    coder.set_auxiliary_variance_ratios(ratios)
    ql, qs, pl, ps = _cuda(*host)
    idx, z = coder.encode(_D(ql, qs), _D(pl, ps), seed)
    assert coder.last_path == "device"
    ridx, rz = R.encode_tensor(*host, seed, 21, omega, 1500, _Cached(oracle), ratio=lambda i: ratios[i])
    assert _lists(idx) == ridx and _same(z.cpu().numpy(), rz)
    assert ridx != _tensor_want(1500)[0]                                   # (not the power law's answer)
    assert torch.equal(coder.decode(_D(pl, ps), idx, seed), z)


def test_damaged_rows_decode_to_p_loc(engine):
    host, omega, seed = _tensor_fixture()
    S = 21
    ql, qs, pl, ps = (t.reshape(1, -1) for t in _cuda(*host))
    lay = engine.layout(1, ql.numel(), 1500, seed)
    assert lay.n_blocks == 6 and lay.distinct_dims == [1500, 692]
    K, idx, z = engine.gc_encode_blocks(lay, ql, qs, pl, ps, seed, omega, S, 12)
    good = engine.gc_decode_blocks(lay, pl, ps, seed, S, K, idx)
    assert torch.equal(good, z) and _same(z.cpu().numpy(), GOLD["tensor_bs1500_sample"])
    Kb, ib = K.clone(), idx.clone()
    Kb[0], Kb[1] = -1, 13
    ib[2, 1], ib[3, 0] = S, -1
    bad = engine.gc_decode_blocks(lay, pl, ps, seed, S, Kb, ib).cpu().numpy().reshape(-1)
    at = lay.element_index(np.arange(lay.n_blocks), 1500)
    want, plh = z.cpu().numpy().reshape(-1), pl.cpu().numpy().reshape(-1)
    for row in range(lay.n_blocks):
        e = at[row][at[row] >= 0]
        assert np.array_equal(bad[e], plh[e] if row < 4 else want[e]), row


# 7, 8 ------------------------------------------------------------------------------------------------------------------------------
def _abi_call(engine, entry, ws_short=None):
    """One 1025-dim block through `entry` of the C ABI; -> (status, out_K on the host, needed workspace bytes)."""
    from irec.engine import _ptr
    host, omega, seed = _block("block_D2500_large", 1025)
    ql, qs, pl, ps = (t.reshape(-1) for t in _cuda(*host))
    lay = engine.layout(1, 1025, None, seed)
    tables, keep = engine.normal_tables(seed, 21, [1025], 8)
    out_K = torch.full((1,), -77, dtype=torch.int32, device="cuda")
    out_idx = torch.zeros((1, 8), dtype=torch.int32, device="cuda")
    sample = torch.empty_like(ql)
    args = [engine.ctx, 1, _ptr(lay.block_base), _ptr(lay.block_pos), _ptr(lay.block_dim), _ptr(lay.perm), _ptr(ql), _ptr(qs), _ptr(pl),
            _ptr(ps), ctypes.byref(tables), 3.0, 8, _ptr(out_K), _ptr(out_idx), _ptr(sample)]
    need = engine.lib.irec_gc_encode_workspace_bytes(engine.ctx, 1, 1025)
    if ws_short is not None:
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        args += [_ptr(ws), need - ws_short]
    st = getattr(engine.lib, entry)(*args, engine._stream())
    torch.cuda.synchronize()
    del keep
    return st, int(out_K.cpu()[0]), need, out_idx.cpu().numpy()[0].tolist()


def test_workspace_abi(engine, oracle):
    from irec import _lib
    lib = engine.lib
    assert lib.irec_gc_encode_workspace_bytes(engine.ctx, 1, 1024) == 0
    assert lib.irec_gc_encode_workspace_bytes(engine.ctx, 64, 1024) == 0
    one = lib.irec_gc_encode_workspace_bytes(engine.ctx, 1, 1025)
    assert one >= 4 * 2048 * 4                     # one slab: four float arrays of 1025 dims rounded up to 1024s
    assert lib.irec_gc_encode_workspace_bytes(engine.ctx, 2, 1025) >= 2 * 4 * 2048 * 4
    assert lib.irec_gc_encode_workspace_bytes(engine.ctx, 1 << 20, 1025) == lib.irec_gc_encode_workspace_bytes(engine.ctx, 1 << 21, 1025)
    st, K, need, _ = _abi_call(engine, "irec_gc_importance_encode_ws", ws_short=1)
    assert st == _lib.IREC_E_WORKSPACE and K == -77, "a short workspace: nothing launched, the outputs untouched"
    assert str(need).encode() in lib.irec_last_error()
    st, K, _, idx = _abi_call(engine, "irec_gc_importance_encode_ws", ws_short=0)
    host, omega, seed = _block("block_D2500_large", 1025)
    ridx, _ = _referee_blocks(oracle, host, seed, 21, 3.0)
    assert st == _lib.IREC_OK and K == 8 == len(ridx[0]) and idx == ridx[0]


def test_legacy_entry_still_refuses_a_wide_block(engine):
    from irec import _lib
    st, K, _, _ = _abi_call(engine, "irec_gc_importance_encode")
    assert st == _lib.IREC_OK and K == -1


# 9 ---------------------------------------------------------------------------------------------------------------------------------
def test_model_with_the_default_coder_args(engine, tmp_path):
    """coder_args={}: block_size None, every latent ONE block of 8192 dims (1 x 8 x 32 x 32)."""
    import irec.io
    from irec.models import BidirectionalResNetVAE
    torch.manual_seed(0)
    m = BidirectionalResNetVAE(num_res_blocks=3, sampler="importance", sampler_args={"coding_bits": 3. / LN2, "alpha": np.inf},
                               coder_args={}, deterministic_filters=16, stochastic_filters=8, kl_per_partition=3.)
    with torch.no_grad():
        for b in m.residual_blocks:
            for head in (b.gen_posterior_loc_head, b.gen_posterior_log_scale_head, b.infer_posterior_loc_head,
                         b.infer_posterior_log_scale_head, b.prior_loc_head, b.prior_log_scale_head):
                head.weight.mul_(0.3)
        m._generative_base.normal_(0, 0.5)
    m = m.cuda().eval()
    S = m.residual_blocks[0].coder.sampler.n_samples()
    assert all(b.coder.block_size is None for b in m.residual_blocks)
    torch.manual_seed(1)
    image = torch.rand(1, 3, 64, 64, device="cuda") - 0.5
    block_indices, recon = m.compress(image, seed=42)
    assert len(block_indices) == 3 and all(len(ix) >= 1 for ix in block_indices)
    assert all(b.coder.last_path == "device" for b in m.residual_blocks)
    assert recon.shape == image.shape and torch.isfinite(recon).all()
    path = str(tmp_path / "image.rec")
    as_blocks = [[ix] for ix in block_indices]                       # the file's form: [res_block][coder_block] -> indices
    irec.io.write_compressed_code(path, 42, (64, 64, 3), 8192, as_blocks, max_index=S)
    seed, shape, bs, read_back = irec.io.read_compressed_code(path)
    assert (seed, shape, bs) == (42, (64, 64, 3), 8192)
    assert read_back == [[[int(v) for v in ix]] for ix in block_indices]
    assert torch.equal(m.decompress([b[0] for b in read_back], 42, image.shape), recon)
    assert all(b.coder.last_path == "device" for b in m.residual_blocks)
