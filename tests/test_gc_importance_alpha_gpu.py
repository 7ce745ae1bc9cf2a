"""The sequential importance coder at FINITE alpha on the GPU (csrc/irec_gc.hip: gc_gumbel_encode_kernel / gc_gumbel_encode_wide_kernel
behind irec_gc_importance_encode_gumbel): against the reference's own outputs (tests/golden/refpy_gc_importance_alpha.npz) and the
numpy referee with alpha (tests/gc_referee_alpha.py, pinned to those outputs by tests/test_gc_importance_alpha_host.py) -- indices and
samples bit for bit; crafted Gumbel tables (NaN rows, +inf, -inf) through the C entry; the entry's argument checks; the model shim."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import gc_referee_alpha as RA
from conftest import GOLDEN_DIR
from gc_alpha_cases import CELLS, GOLD, WIDE_CELLS, cell_inputs, coder_of, same

pytestmark = pytest.mark.gpu

LN2 = np.log(2)
ENTRY = "irec_gc_importance_encode_gumbel"


@functools.lru_cache(maxsize=16)
def _normal_of(seed, count):
    from oracle import oracle as O
    return O.tf_random_normal(seed, count)


class _D:
    def __init__(self, loc, scale):
        self.loc, self.scale = loc, scale


def _cuda(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _bits_for(S):
    return float(np.log2(S - 0.5))     # ceil(exp(bits * ln 2)) = S whatever the float32 rounding of the product


def _lists(idx):
    return [[int(v) for v in ix] for ix in idx]


def _block_of(D, seed, nats=11.0):
    """One block of D dims whose KL is about `nats` (K = 4 or 5 at Omega = 3), spread evenly: float32 (mq, sq, mp, sp)."""
    rng = np.random.default_rng(4000 + 31 * seed + D)
    mp = rng.normal(0.0, 1.0, D)
    sp = np.exp(rng.normal(0.0, 0.25, D))
    mq = mp + sp * np.sqrt(2.0 * nats / D) * rng.choice([-1.0, 1.0], D)
    sq = sp * np.exp(-np.abs(rng.normal(0.0, 0.02, D)))
    return tuple(np.asarray(v, np.float32) for v in (mq, sq, mp, sp))


def _referee(oracle, blocks, seed, S, omega, alpha, gumbel=RA.reference_gumbel):
    idx, out = [], []
    for b in blocks:
        K = oracle.num_aux(oracle.block_kl(*b), omega)
        i, z = RA.encode_block(*b, seed, S, K, _normal_of, alpha, gumbel)
        idx.append(i)
        out.append(z)
    return idx, out


# 1 -- the reference's own outputs ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", CELLS + WIDE_CELLS)
def test_every_golden_cell(engine, cell):
    stats, omega, seed = cell_inputs(cell)
    bits, alpha = float(GOLD[f"{cell}_bits"]), float(GOLD[f"{cell}_alpha"])
    coder = coder_of(omega, bits, alpha)
    coder.table_steps = coder._max_K_hint = 16
    ql, qs, pl, ps = _cuda(*(s[None] for s in stats))
    idx, z = coder.encode_block(_D(ql, qs), _D(pl, ps), seed)
    assert coder.last_path == "device" and z.is_cuda and z.shape == ql.shape
    assert [int(i) for i in idx] == GOLD[f"{cell}_indices"].tolist()
    assert same(z.cpu().numpy(), GOLD[f"{cell}_sample"])
    keep = list(idx)
    dec = coder.decode_block(_D(pl, ps), idx, seed)
    assert coder.last_path == "device" and idx == keep and torch.equal(dec, z) and same(dec.cpu().numpy(), GOLD[f"{cell}_decoded"])
    for other_alpha in (np.inf, 7.0):                     # the decoder never looks at alpha
        other = coder_of(omega, bits, other_alpha)
        other.table_steps = 16
        assert torch.equal(other.decode_block(_D(pl, ps), idx, seed), z) and other.last_path == "device"


def test_tensor_fixture_is_the_reference(engine):
    g = np.load(os.path.join(GOLDEN_DIR, "tensor_rvae_cfg2.npz"))
    omega, seed, bs = float(g["kl_per_partition"]), int(g["seed"]), int(g["block_size"])
    want = [GOLD["tensor_indices"][r, :k].tolist() for r, k in enumerate(GOLD["tensor_K"])]
    coder = coder_of(omega, omega / LN2, 1.0, block_size=bs)
    ql, qs, pl, ps = _cuda(*(g[k] for k in ("q_loc", "q_scale", "p_loc", "p_scale")))
    idx, z = coder.encode(_D(ql, qs), _D(pl, ps), seed)
    assert coder.last_path == "device" and _lists(idx) == want and same(z.cpu().numpy(), GOLD["tensor_sample"])
    assert want != [GOLD["tensor_inf_indices"][r, :k].tolist() for r, k in enumerate(GOLD["tensor_inf_K"])]
    dec = coder_of(omega, omega / LN2, np.inf, block_size=bs).decode(_D(pl, ps), idx, seed)
    assert torch.equal(dec, z) and same(dec.cpu().numpy(), GOLD["tensor_decoded"])
    # defer=True and the packed decode: rows that never leave the device
    from irec.coding.beam_search_coder import PendingCode
    pending, z2 = coder.encode(_D(ql, qs), _D(pl, ps), seed, defer=True, max_K=12)
    assert isinstance(pending, PendingCode) and torch.equal(z2, z) and _lists(pending.to_lists()[0]) == want


# 2 -- the referee ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [21, 256, 1177])
@pytest.mark.parametrize("D", [1, 3, 255, 1000])
def test_narrow_kernel_against_the_referee(engine, oracle, D, S):
    """S = 21: 21 live lanes of one wave.  256: the arg-max crosses four waves.  1177: a lane owns two samples."""
    blocks = [_block_of(D, s) for s in (1, 2)]
    alpha = 1.0 if D != 255 else 2.5
    coder = coder_of(3., _bits_for(S), alpha)
    coder.table_steps = coder._max_K_hint = 8
    assert coder.sampler.n_samples() == S
    ql, qs, pl, ps = _cuda(*(np.stack([b[j] for b in blocks]) for j in range(4)))
    idx, z = coder.encode(_D(ql, qs), _D(pl, ps), 17, batched=True)
    assert coder.last_path == "device"
    ridx, rz = _referee(oracle, blocks, 17, S, 3.0, alpha)
    assert _lists(idx) == ridx and same(z.cpu().numpy(), np.stack(rz))
    assert torch.equal(coder.decode(_D(pl, ps), idx, 17, batched=True), z)


def _abi_encode(engine, blocks, S, seed, omega, max_K, entry=ENTRY, gumbel=None, steps=None):
    """The blocks (any dims, at most four distinct) in ONE call of `entry`, straight through the C ABI.  gumbel: None (NULL), or
    (table float32 [steps, S_pad] host or CUDA, n_samples, steps, alpha).  Outputs are prefilled (-77 / -5 / -9): what a refused call
    must leave.  -> (status, K, idx, sample per block)."""
    from irec import _lib
    from irec.engine import _ptr
    steps = max_K if steps is None else steps
    dims = [int(b[0].size) for b in blocks]
    n = len(blocks)
    ql, qs, pl, ps = _cuda(*(np.concatenate([b[j].reshape(-1) for b in blocks]).astype(np.float32) for j in range(4)))
    pos = np.concatenate([[0], np.cumsum(dims)[:-1]]).astype(np.int32)
    base, pos_d, dim_d = _cuda(np.zeros(n, np.int64), pos, np.asarray(dims, np.int32))
    tables, keep = engine.normal_tables(seed, S, sorted(set(dims), reverse=True), steps)
    out_K = torch.full((n,), -77, dtype=torch.int32, device="cuda")
    out_idx = torch.full((n, max_K), -5, dtype=torch.int32, device="cuda")
    sample = torch.full_like(ql, -9.0)
    need = engine.lib.irec_gc_encode_workspace_bytes(engine.ctx, n, max(dims))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda") if need else None
    args = [engine.ctx, n, _ptr(base), _ptr(pos_d), _ptr(dim_d), None, _ptr(ql), _ptr(qs), _ptr(pl), _ptr(ps), ctypes.byref(tables),
            float(np.float32(omega)), max_K, _ptr(out_K), _ptr(out_idx), _ptr(sample), _ptr(ws), need]
    if entry == ENTRY:
        g = None
        if gumbel is not None:
            tab = gumbel[0] if torch.is_tensor(gumbel[0]) else torch.from_numpy(np.ascontiguousarray(gumbel[0], np.float32)).cuda()
            g = _lib.IrecGumbelTable(tab.data_ptr(), int(gumbel[1]), int(gumbel[2]), float(gumbel[3]))
        args.append(ctypes.byref(g) if g is not None else None)
    st = getattr(engine.lib, entry)(*args, engine._stream())
    torch.cuda.synchronize()
    del keep
    zs = sample.cpu().numpy()
    return st, out_K.cpu().numpy(), out_idx.cpu().numpy(), [zs[p:p + d] for p, d in zip(pos, dims)]


def _check_call(oracle, blocks, got, seed, S, omega, alpha, gumbel=RA.reference_gumbel):
    st, K, idx, zs = got
    assert st == 0
    ridx, rz = _referee(oracle, blocks, seed, S, omega, alpha, gumbel)
    for r, (ri, z) in enumerate(zip(ridx, rz)):
        assert max(int(K[r]), 1) == len(ri) and idx[r, :len(ri)].tolist() == ri, r
        assert same(zs[r], z), r
    return ridx


def test_wide_tile_form_with_narrow_blocks_in_the_same_call(engine, oracle):
    """One 1500-dim block (S_pad = 32: the tile form) and narrow blocks of 255 and 3 dims: the wide kernel codes all of them."""
    S, seed, steps = 21, 17, 8
    blocks = [_block_of(1500, 1), _block_of(255, 1), _block_of(255, 2), _block_of(3, 1), _block_of(3, 2)]
    g, keep = engine.gumbel_table(seed, S, steps, 1.0)
    got = _abi_encode(engine, blocks, S, seed, 3.0, steps, gumbel=(keep, S, steps, 1.0))
    ridx = _check_call(oracle, blocks, got, seed, S, 3.0, 1.0)
    inf = _abi_encode(engine, blocks, S, seed, 3.0, steps, gumbel=None)
    assert any(inf[2][r, :len(ri)].tolist() != ri for r, ri in enumerate(ridx))      # the perturbation decided somewhere


def test_wide_plain_walk(engine, oracle):
    """1100 dims at S = 1177 (S_pad = 1184 > 1024): the plain walk, a lane owns two samples."""
    S, seed, steps = 1177, 17, 6
    blocks = [_block_of(1100, 3)]
    g, keep = engine.gumbel_table(seed, S, steps, 1.0)
    _check_call(oracle, blocks, _abi_encode(engine, blocks, S, seed, 3.0, steps, gumbel=(keep, S, steps, 1.0)), seed, S, 3.0, 1.0)


# 3 -- crafted tables: the table is the caller's data ---------------------------------------------------------------------------------
def _crafted_case(engine, oracle, craft, alpha=1.0, wide=False):
    """3-dim blocks (and, wide: one of 1025 dims, so that the wide kernel takes the call) under the Gumbel table `craft(w0)` builds from
    zeros: checked against the referee; -> (indices per block, table)."""
    S, seed, steps = 21, 5, 6
    blocks = [_block_of(3, s) for s in (1, 2, 3)] + ([_block_of(1025, 1)] if wide else [])
    tab = np.zeros((steps, 32), np.float32)
    craft(tab)
    gumbel = lambda step_seed, n: tab[step_seed - seed, :n]                      # noqa: E731
    got = _abi_encode(engine, blocks, S, seed, 3.0, steps, gumbel=(tab, S, steps, alpha))
    return _check_call(oracle, blocks, got, seed, S, 3.0, alpha, gumbel), tab


@pytest.mark.parametrize("wide", [False, True])
def test_crafted_gumbel_tables(engine, oracle, wide):
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    base, _ = _crafted_case(engine, oracle, lambda t: None, wide=wide)        # zeros: the arg-max of alpha * w
    assert all(len(ix) >= 2 for ix in base)

    def all_nan_first_step(t):
        t[0, :] = nan
    idx, _ = _crafted_case(engine, oracle, all_nan_first_step, wide=wide)
    assert all(ix[0] == 0 for ix in idx)                                       # no candidate: the accumulator's start, index 0

    def one_inf(t):
        t[:, 13] = inf
    idx, _ = _crafted_case(engine, oracle, one_inf, wide=wide)
    assert all(v == 13 for ix in idx for v in ix)                              # +inf wins over any weight

    def two_inf(t):
        t[:, 17] = inf
        t[:, 6] = inf
    idx, _ = _crafted_case(engine, oracle, two_inf, wide=wide)
    assert all(v == 6 for ix in idx for v in ix)                               # the lower index of equals

    def all_minus_inf_but_one(t):
        t[:, :] = -inf
        t[:, 9] = 0.0
        t[1, :] = -inf
    idx, _ = _crafted_case(engine, oracle, all_minus_inf_but_one, wide=wide)
    assert all(ix[0] == 9 and ix[1] == 0 and all(v == 9 for v in ix[2:]) for ix in idx)   # -inf is never chosen (step 1: nobody is)

    def nan_at_the_winner(t):                                                  # block 0's step-0 winner under zeros
        t[0, base[0][0]] = nan
    idx, _ = _crafted_case(engine, oracle, nan_at_the_winner, wide=wide)
    assert idx[0][0] != base[0][0]                                             # the choice passes to the next (the referee says which)


# 4 -- the entry's contract -------------------------------------------------------------------------------------------------------------
def test_null_gumbel_is_the_ws_entry_bit_for_bit(engine):
    S, seed, steps = 21, 17, 8
    for blocks in ([_block_of(1500, 1), _block_of(255, 1), _block_of(3, 1)], [_block_of(255, 1), _block_of(3, 1), _block_of(3, 2)]):
        a = _abi_encode(engine, blocks, S, seed, 3.0, steps, entry="irec_gc_importance_encode_ws")
        b = _abi_encode(engine, blocks, S, seed, 3.0, steps, gumbel=None)
        assert a[0] == b[0] == 0 and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
        assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a[3], b[3]))
        assert int(a[1].min()) >= 1 and not (a[2][:, 0] == -5).any()


def test_bad_gumbel_arguments_are_refused_before_any_launch(engine):
    from irec import _lib
    S, seed, steps = 21, 17, 8
    blocks = [_block_of(255, 1), _block_of(3, 1)]
    tab = np.zeros((steps, 32), np.float32)
    for bad in ((tab, S + 1, steps, 1.0), (tab, S, steps - 1, 1.0), (tab, S, steps + 1, 1.0), (tab, S, steps, 0.5),
                (tab, S, steps, float("nan")), (tab, S, steps, float("inf"))):
        st, K, idx, zs = _abi_encode(engine, blocks, S, seed, 3.0, steps, gumbel=bad)
        assert st == _lib.IREC_E_INVALID, bad[1:]
        assert (K == -77).all() and (idx == -5).all() and all((z == -9.0).all() for z in zs), bad[1:]
    assert b"Alpha must be in the range [1, inf)" in engine.lib.irec_last_error()
    st, K, _, _ = _abi_encode(engine, blocks, S, seed, 3.0, steps, gumbel=(tab, S, steps, 1.0))
    assert st == 0 and (K >= 1).all()


# 5 -- the model shim -------------------------------------------------------------------------------------------------------------------
SEED = 42


def _model(alpha):
    """tests/test_decompress_device_gpu.py's importance model: 32 x 32 images, 2048-dim latents, blocks of 1000 + 1000 + 48."""
    from irec.models import BidirectionalResNetVAE
    torch.manual_seed(0)
    m = BidirectionalResNetVAE(num_res_blocks=3, sampler="importance", sampler_args={"coding_bits": 3. / LN2, "alpha": alpha},
                               coder_args={"block_size": 1000}, deterministic_filters=16, stochastic_filters=8, kl_per_partition=3.)
    with torch.no_grad():
        for b in m.residual_blocks:
            for head in (b.gen_posterior_loc_head, b.gen_posterior_log_scale_head, b.infer_posterior_loc_head,
                         b.infer_posterior_log_scale_head, b.prior_loc_head, b.prior_log_scale_head):
                head.weight.mul_(0.3)
        m._generative_base.normal_(0, 0.5)
    return m.cuda().eval()


def _packed_lists(K, idx):
    K, idx = K.cpu().numpy(), idx.cpu().numpy()
    return [[[idx[i, r, j, :K[i, r, j]].tolist() for j in range(K.shape[2])] for r in range(K.shape[1])] for i in range(K.shape[0])]


def test_model_at_alpha_one(engine):
    from irec.io import rec_files_max_K
    from irec.models import GraphedCompress, GraphedDecompress
    m, m_inf = _model(1.0), _model(np.inf)
    torch.manual_seed(7)
    images = torch.rand(2, 3, 32, 32, device="cuda") - 0.5
    (blob, off, recon), (K, idx) = m.compress_rec(images, seed=SEED, return_pendings=True)
    assert all(b.coder.last_path == "device" for b in m.residual_blocks)
    lists = _packed_lists(K, idx)
    out = m.decompress_rec(blob, off, SEED, images.shape)
    assert torch.equal(out, m.decompress(lists, seed=SEED, image_shape=images.shape))       # the list path's pixels
    assert torch.allclose(out, recon, atol=1e-5, rtol=0)
    assert torch.equal(m.decompress_packed(K, idx, SEED, images.shape), out)
    # compress and compress_packed code the same indices
    block_indices, _ = m.compress(images, seed=SEED)
    assert [[_lists(b) for b in img] for img in block_indices] == lists
    Kp, idxp, _ = m.compress_packed(images, seed=SEED)
    assert np.array_equal(Kp, K.cpu().numpy()) and _packed_lists(torch.from_numpy(Kp), torch.from_numpy(idxp)) == lists
    # the graphs replay to the same
    off_h = off.cpu().numpy()
    gd = GraphedDecompress(m, images.shape, SEED, R=3, bpt=3, max_K=rec_files_max_K(blob.cpu().numpy(), off_h), blob_bytes=blob.numel())
    assert torch.equal(gd(blob, off_h), out) and torch.equal(gd(blob, off_h), out) and gd.captures == 1
    gc = GraphedCompress(m, images.shape, SEED)
    g_idx, g_rec = gc(images)
    assert [[_lists(b) for b in img] for img in g_idx] == lists and gc.graph is not None
    # another coder than alpha = inf: other files
    blob_inf, off_inf, _ = m_inf.compress_rec(images, seed=SEED)
    assert not (blob_inf.numel() == blob.numel() and torch.equal(blob_inf, blob))
    # ... which the alpha = 1 model's decoder reads all the same (the decoder never looks at alpha)
    assert torch.equal(m.decompress_rec(blob_inf, off_inf, SEED, images.shape), m_inf.decompress_rec(blob_inf, off_inf, SEED, images.shape))


# 6 -- the limits -----------------------------------------------------------------------------------------------------------------------
def test_tables_that_do_not_fit_still_take_the_host_loop(engine):
    """S = 4096 over a 4096-step window: the normal tables exceed what the library builds; the call runs the host loop on the GPU
    tensors, at finite alpha as at alpha = inf, and returns what the CPU tensors return."""
    g = np.load(os.path.join(GOLDEN_DIR, "block_D192_cfg0.npz"))
    host = [g[k][None] for k in ("q_loc", "q_scale", "p_loc", "p_scale")]
    cpu = [torch.from_numpy(h) for h in host]
    coder = coder_of(float(g["kl_per_partition"]), 12.0, 1.0)
    coder.table_steps = coder._max_K_hint = 4096
    ql, qs, pl, ps = _cuda(*host)
    idx, z = coder.encode(_D(ql, qs), _D(pl, ps), 5)
    assert coder.last_path == "host" and z.is_cuda and z.shape == ql.shape
    dec = coder.decode(_D(pl, ps), idx, 5)
    assert coder.last_path == "host" and torch.equal(dec, z)
    idx_h, z_h = coder.encode(_D(cpu[0], cpu[1]), _D(cpu[2], cpu[3]), 5)
    assert idx == idx_h and torch.equal(z.cpu(), z_h)
    coder.table_steps = coder._max_K_hint = 16                  # the same call within the limit: the kernels, same outputs
    idx_d, z_d = coder.encode(_D(ql, qs), _D(pl, ps), 5)
    assert coder.last_path == "device" and [int(v) for v in idx_d] == [int(v) for v in idx] and torch.equal(z_d, z)


def test_window_smaller_than_K_is_coded_again(engine):
    g = np.load(os.path.join(GOLDEN_DIR, "tensor_rvae_cfg2.npz"))
    omega, seed, bs = float(g["kl_per_partition"]), int(g["seed"]), int(g["block_size"])
    coder = coder_of(omega, omega / LN2, 1.0, block_size=bs)
    coder.table_steps = coder._max_K_hint = 4
    ql, qs, pl, ps = _cuda(*(g[k] for k in ("q_loc", "q_scale", "p_loc", "p_scale")))
    idx, z = coder.encode(_D(ql, qs), _D(pl, ps), seed)
    assert coder.last_path == "device" and coder._max_K_hint == 9
    assert _lists(idx) == [GOLD["tensor_indices"][r, :k].tolist() for r, k in enumerate(GOLD["tensor_K"])]
    assert same(z.cpu().numpy(), GOLD["tensor_sample"])


@pytest.mark.parametrize("alpha", [0.5, float("nan")])
def test_alpha_below_one_raises_before_any_device_work(engine, alpha):
    from irec.coding.utils import CodingError
    stats, omega, seed = cell_inputs(CELLS[0])
    coder = coder_of(omega, 8.0, alpha)
    ql, qs, pl, ps = _cuda(*(s[None] for s in stats))
    coder.last_path = None
    for call in (lambda: coder.encode_block(_D(ql, qs), _D(pl, ps), seed), lambda: coder.encode(_D(ql, qs), _D(pl, ps), seed),
                 lambda: coder.encode(_D(ql, qs), _D(pl, ps), seed, defer=True)):
        with pytest.raises(CodingError, match=r"Alpha must be in the range \[1, inf\), but (0\.5|nan) was given!"):
            call()
    assert coder.last_path is None
