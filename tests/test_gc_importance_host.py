"""The sequential importance coder without a GPU: GaussianCoder(sampler=ImportanceSampler(..)) (rec/coding/coder.py:412-587).

  * the numpy referee of the arithmetic contract (tests/gc_referee.py) returns the REFERENCE'S OWN outputs
    (tests/golden/refpy_gc_importance.npz: its unmodified GaussianCoder run over oracle/tfshim) bit for bit, on every cell;
  * irec.GaussianCoder's host path -- the reference's loop over `sampler.coded_sample` -- returns the same outputs;
  * decode(encode) is exact, a zero-KL block emits one index, fitted ratios shorter than K raise the reference's text,
    decode_block leaves the caller's list alone;
  * irec_normal_table_build is oracle.tf_random_normal rearranged.
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import gc_referee as R
from conftest import GOLDEN_DIR

pytestmark = [pytest.mark.both_suites, pytest.mark.usefixtures("suite")]

GOLD = np.load(os.path.join(GOLDEN_DIR, "refpy_gc_importance.npz"))
CELLS = [str(c) for c in GOLD["cells"]]
N = torch.distributions.Normal


def _fixture(cell):
    return np.load(os.path.join(GOLDEN_DIR, cell.split("__")[0] + ".npz"))


def _coder(omega, bits, **kw):
    import irec
    return irec.GaussianCoder(kl_per_partition=omega, sampler=irec.ImportanceSampler(coding_bits=bits), **kw)


def _dists(g, lead=True):
    a = [torch.from_numpy(np.asarray(g[k])[None] if lead else np.asarray(g[k])) for k in ("q_loc", "q_scale", "p_loc", "p_scale")]
    return N(a[0], a[1], validate_args=False), N(a[2], a[3], validate_args=False)


def test_the_golden_file_holds_every_cell():
    """Both settings of every block fixture of at most 1024 dims: no cell left out."""
    import glob
    names = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "block_*.npz"))
                   if np.load(p)["q_loc"].size <= 1024)
    assert len(names) == 18
    assert CELLS == [f"{n}__{m}" for n in names for m in ("omega", "bits8")]


@pytest.mark.parametrize("cell", CELLS)
def test_referee_is_the_reference(oracle, cell):
    g = _fixture(cell)
    ref_idx = GOLD[f"{cell}_indices"].tolist()
    S = oracle.importance_n_samples(float(GOLD[f"{cell}_bits"]))
    K = oracle.num_aux(oracle.block_kl(g["q_loc"], g["q_scale"], g["p_loc"], g["p_scale"]), float(g["kl_per_partition"]))
    assert max(K, 1) == len(ref_idx)          # the canonical K (irec_block_kl) is the reference's
    idx, z = R.encode_block(g["q_loc"], g["q_scale"], g["p_loc"], g["p_scale"], int(g["seed"]), S, K, oracle.tf_random_normal)
    assert idx == ref_idx
    assert np.array_equal(z, GOLD[f"{cell}_sample"])
    dec = R.decode_block(g["p_loc"], g["p_scale"], idx, int(g["seed"]), S, oracle.tf_random_normal)
    assert np.array_equal(dec, GOLD[f"{cell}_decoded"]) and np.array_equal(dec, z)


@pytest.mark.parametrize("cell", CELLS)
def test_host_path_is_the_reference(cell):
    g = _fixture(cell)
    coder = _coder(float(g["kl_per_partition"]), float(GOLD[f"{cell}_bits"]))
    q, p = _dists(g)
    idx, z = coder.encode_block(q, p, int(g["seed"]))
    assert [int(i) for i in idx] == GOLD[f"{cell}_indices"].tolist()
    assert z.shape == q.loc.shape and np.array_equal(z.numpy().reshape(-1), GOLD[f"{cell}_sample"])
    keep = list(idx)
    dec = coder.decode_block(p, idx, int(g["seed"]))
    assert idx == keep, "decode_block must not reverse the caller's list (the reference does, coder.py:564)"
    assert torch.equal(dec, z) and np.array_equal(dec.numpy().reshape(-1), GOLD[f"{cell}_decoded"])
    assert coder.get_codelength(idx) == pytest.approx(float(GOLD[f"{cell}_codelength"]), rel=1e-6)


def test_tensor_through_split_and_merge(oracle):
    g = np.load(os.path.join(GOLDEN_DIR, "tensor_rvae_cfg2.npz"))
    omega, seed, bs = float(g["kl_per_partition"]), int(g["seed"]), int(g["block_size"])
    want = [GOLD["tensor_indices"][r, :k].tolist() for r, k in enumerate(GOLD["tensor_K"])]
    assert GOLD["tensor_K"].tolist() == [8, 9, 8, 8, 7, 8, 8, 8, 2]
    S = oracle.importance_n_samples(omega / np.log(2))
    ridx, rz = R.encode_tensor(g["q_loc"], g["q_scale"], g["p_loc"], g["p_scale"], seed, S, omega, bs, oracle)
    assert ridx == want and np.array_equal(rz, GOLD["tensor_sample"])
    coder = _coder(omega, omega / np.log(2), block_size=bs)
    q, p = _dists(g, lead=False)
    idx, z = coder.encode(q, p, seed)
    assert [[int(v) for v in ix] for ix in idx] == want
    assert np.array_equal(z.numpy(), GOLD["tensor_sample"])
    dec = coder.decode(p, idx, seed)
    assert torch.equal(dec, z) and np.array_equal(dec.numpy(), GOLD["tensor_decoded"])
    assert sum(coder.get_codelength(ix) for ix in idx) == pytest.approx(float(GOLD["tensor_codelength"]), rel=1e-6)
    assert float(GOLD["tensor_codelength"]) == pytest.approx(198.0, rel=1e-6)       # 66 indices x 3 nats


def test_zero_kl_block_emits_one_index(oracle):
    g = np.load(os.path.join(GOLDEN_DIR, "block_D192_cfg0.npz"))
    coder = _coder(3., 3. / np.log(2))
    p = N(torch.from_numpy(g["p_loc"][None]), torch.from_numpy(g["p_scale"][None]))
    idx, z = coder.encode_block(p, p, 42)
    assert [int(i) for i in idx] == GOLD["zero_kl_indices"].tolist() == [0]
    assert np.array_equal(z.numpy().reshape(-1), GOLD["zero_kl_sample"])
    ridx, rz = R.encode_block(g["p_loc"], g["p_scale"], g["p_loc"], g["p_scale"], 42, 21, 0, oracle.tf_random_normal)
    assert ridx == [0] and np.array_equal(rz, GOLD["zero_kl_sample"])
    assert torch.equal(coder.decode_block(p, idx, 42), z)


def test_errors_are_the_references():
    import irec
    from irec.coding.utils import CodingError
    g = np.load(os.path.join(GOLDEN_DIR, "block_D192_cfg0.npz"))          # K = 2 at Omega = 3 ... pick ratios shorter than K
    q, p = _dists(g)
    K = len(GOLD["block_D192_cfg0__omega_indices"])
    assert K >= 2
    coder = _coder(float(g["kl_per_partition"]), 4., extrapolate_auxiliary_ratios=False)
    with pytest.raises(CodingError, match="has not been initialized yet"):
        coder.encode_block(q, p, 1)
    coder.set_auxiliary_variance_ratios([1.0] + [0.5] * (K - 2))           # covers K - 1 partitions
    with pytest.raises(CodingError, match=f"KL divergence higher than auxiliary variables can account for.*Requested {K}"):
        coder.encode_block(q, p, 1)
    coder.set_auxiliary_variance_ratios([1.0] + [0.5] * (K - 1))
    idx, z = coder.encode_block(q, p, 1)
    assert len(idx) == K and torch.equal(coder.decode_block(p, idx, 1), z)
    with pytest.raises(CodingError, match="KL divergence higher than auxiliary variables can account for"):
        coder.decode_block(p, idx + [0], 1)
    two = N(torch.zeros(2, 4), torch.ones(2, 4))
    with pytest.raises(CodingError, match="For encoding, batch size must be 1."):
        _coder(3., 4.).encode_block(two, two, 1)
    with pytest.raises(CodingError, match="For encoding, batch size must be 1."):
        _coder(3., 4., block_size=2).encode(two, two, 1)
    with pytest.raises(CodingError, match="update_sampler"):
        _coder(3., 4.).encode_block(N(torch.zeros(1, 4), torch.ones(1, 4)), N(torch.zeros(1, 4), torch.ones(1, 4)), 1, update_sampler=True)
    assert isinstance(irec.BeamSearchCoder(3., 5), irec.GaussianCoder)


def test_host_path_takes_any_sampler_object():
    """What a user's own Sampler (a rejection sampler, say) runs through: the loop only calls coded_sample / decode_sample."""
    import irec
    from irec.coding.samplers import Sampler

    class Recording(Sampler):
        def __init__(self):
            super().__init__()
            self.inner, self.seeds = irec.ImportanceSampler(coding_bits=5.), []

        def coded_sample(self, target, coder, seed):
            self.seeds.append(seed)
            return self.inner.coded_sample(target, coder, seed)

        def decode_sample(self, coder, sample_index, seed):
            return self.inner.decode_sample(coder, sample_index, seed)

        def get_codelength(self, index):
            return 1.0

        def update(self, target, coder):
            pass

    g = np.load(os.path.join(GOLDEN_DIR, "block_D192_cfg2.npz"))
    q, p = _dists(g)
    rec = irec.GaussianCoder(kl_per_partition=float(g["kl_per_partition"]), sampler=Recording())
    idx, z = rec.encode_block(q, p, 7)
    assert rec.sampler.seeds == list(range(7, 7 + len(idx)))
    plain = _coder(float(g["kl_per_partition"]), 5.)
    idx2, z2 = plain.encode_block(q, p, 7)
    assert idx == idx2 and torch.equal(z, z2) and torch.equal(rec.decode_block(p, idx, 7), z)
    assert rec.get_codelength(idx) == len(idx)


@pytest.mark.parametrize("S,dim,steps", [(21, 37, 3), (5, 192, 2), (149, 8, 1), (32, 3, 2)])
def test_normal_table_is_the_stream_rearranged(oracle, S, dim, steps):
    from irec import _lib
    from irec.engine import build_normal_table
    pad = _lib.IREC_NORMAL_TABLE_PAD
    s_pad = -(-S // pad) * pad
    for n_threads in (0, 1, 3):
        tab = build_normal_table(1234, S, dim, steps, n_threads)
        assert tab.shape == (steps, dim, s_pad) and tab.dtype == np.float32
        for j in range(steps):
            x = oracle.tf_random_normal(1234 + j, S * dim).reshape(S, dim)
            assert np.array_equal(tab[j, :, :S], x.T)
            assert not tab[j, :, S:].any()
    lib = _lib.load()
    assert lib.irec_normal_table_floats(S, dim, steps) == steps * dim * s_pad
    assert lib.irec_normal_table_floats(1 << 20, 1024, 32) == 0 and b"IREC_TABLE_BYTES_HARD" in lib.irec_last_error()
    assert lib.irec_normal_table_floats(0, 4, 1) == 0
    assert lib.irec_normal_table_build(1, S, dim, steps, ctypes.c_void_p(0), 1) == _lib.IREC_E_INVALID


@functools.lru_cache(maxsize=None)
def _families_cells():
    return [(f, D) for f in ("benign", "sharp", "collapsed", "eqvar", "tiny", "wide", "offset") for D in (1000, 192, 37)]


@pytest.mark.parametrize("family,D", _families_cells())
def test_host_path_and_referee_agree_on_model_shaped_latents(oracle, family, D):
    """The host path weighs with libm's logf, the contract with the deterministic log rounded to float32: every emitted index
    and every sample agree on the model-shaped families too (a disagreement would need two weights closer than one ulp of log)."""
    import latent_families as lf
    mq, sq, mp, sp = lf.block(family, D, 3, 3.0, max_K=12)
    K = oracle.num_aux(oracle.block_kl(mq, sq, mp, sp), 3.0)
    ridx, rz = R.encode_block(mq, sq, mp, sp, 11, 21, K, oracle.tf_random_normal)
    assert np.isfinite(rz).all()
    coder = _coder(3., 3. / np.log(2))
    q = N(torch.from_numpy(mq[None]), torch.from_numpy(sq[None]), validate_args=False)
    p = N(torch.from_numpy(mp[None]), torch.from_numpy(sp[None]), validate_args=False)
    idx, z = coder.encode_block(q, p, 11)
    assert [int(i) for i in idx] == ridx and np.array_equal(z.numpy().reshape(-1), rz)
    assert np.array_equal(R.decode_block(mp, sp, ridx, 11, 21, oracle.tf_random_normal), rz)


def test_model_shim_builds_the_importance_coder():
    import irec
    from irec.models import BidirectionalResNetVAE, ModelError
    m = BidirectionalResNetVAE(num_res_blocks=2, sampler="importance", sampler_args={"coding_bits": 3. / np.log(2), "alpha": np.inf},
                               coder_args={"block_size": 1000}, deterministic_filters=8, stochastic_filters=4, kl_per_partition=3.)
    for r, blk in enumerate(m.residual_blocks):
        assert type(blk.coder) is irec.GaussianCoder and type(blk.coder.sampler) is irec.ImportanceSampler
        assert blk.coder.block_size == 1000 and blk.coder.sampler.n_samples() == 21 and blk.coder.sampler.alpha == np.inf
        assert blk.coder.name == f"encoder_for_resnet_block_{r}" and blk.coder.kl_per_partition == np.float32(3.)
    with pytest.raises(ModelError):
        BidirectionalResNetVAE(num_res_blocks=1, sampler="rejection")


@pytest.mark.parametrize("D", [1000, 192, 37, 1])
def test_host_K_is_the_canonical_K(oracle, D):
    """One coder, one K: the host path counts partitions as block_kl_kernel does (float64 KL, canonical tree, float32 ceil) -- also
    where KL / Omega sits on an integer."""
    import latent_families as lf
    from irec.coding.coder import canonical_partitions
    from irec.coding.utils import CodingError
    blocks = lf.mixed(D, 2, 3.0) + [lf.block(f, D, s, 3.0) for f in ("benign", "sharp", "collapsed", "wide") for s in range(4)]
    for mq, sq, mp, sp in blocks:
        for omega in (3.0, 0.37):
            assert canonical_partitions(mq, sq, mp, sp, np.float32(omega)) == oracle.num_aux(oracle.block_kl(mq, sq, mp, sp), omega)
    mq, sq, mp, sp = blocks[0]
    assert canonical_partitions(mp, sp, mp, sp, np.float32(3.)) == 0
    bad = sp.copy()
    bad[0] = 0.0                                            # an infinite KL: the device reports 10^9 partitions and the mirror raises
    assert canonical_partitions(mq, sq, mp, bad, np.float32(3.)) == 1000000000
    coder = _coder(3., 4.)
    with pytest.raises(CodingError, match="KL divergence needs 1000000000 partitions"):
        coder.encode_block(N(torch.from_numpy(mq[None]), torch.from_numpy(sq[None]), validate_args=False),
                           N(torch.from_numpy(mp[None]), torch.from_numpy(bad[None]), validate_args=False), 1)


def test_device_retries_are_bounded_and_fall_back_to_the_host(monkeypatch):
    """A block that needs more partitions than the tables can cover is not coded again for ever: the call takes the host loop."""
    from irec import _lib
    from irec.coding.beam_search_coder import MorePartitionsNeeded
    from irec.coding.coder import DeviceWindowExceeded
    from irec.engine import NormalTableTooLarge
    g = np.load(os.path.join(GOLDEN_DIR, "block_D192_cfg0.npz"))
    q, p = _dists(g)
    coder = _coder(float(g["kl_per_partition"]), float(g["kl_per_partition"]) / np.log(2))
    calls = []

    class Pending:
        sample = None

        def __init__(self, need):
            self.need = need

        def to_lists(self):
            coder._max_K_hint = max(coder._max_K_hint, self.need)      # what PendingCode._check does before it raises
            raise MorePartitionsNeeded(self.need)

    def device(need):
        def call(q_loc, q_scale, p_loc, p_scale, seed, block_size, max_K=None, table_steps=None):
            calls.append(max_K)
            return Pending(need)
        return call

    assert coder.DEVICE_MAX_K == _lib.IREC_TABLE_STEPS_MAX and issubclass(DeviceWindowExceeded, NormalTableTooLarge)
    monkeypatch.setattr(coder, "encode_tensors_device", device(5000))           # beyond the tables: one attempt, no retry
    with pytest.raises(DeviceWindowExceeded, match="5000 partitions"):
        coder.encode_tensors(q.loc, q.scale, p.loc, p.scale, 1, None)
    assert calls == [None] and coder._max_K_hint <= coder.DEVICE_MAX_K
    del calls[:]
    monkeypatch.setattr(coder, "encode_tensors_device", device(100))            # a device that never satisfies: bounded
    with pytest.raises(DeviceWindowExceeded):
        coder.encode_tensors(q.loc, q.scale, p.loc, p.scale, 1, None)
    assert calls == [None] + [100] * (coder.DEVICE_ATTEMPTS - 1)
    # through the public methods: the host loop's (= the reference's) outputs, and the coder says which path it took
    monkeypatch.setattr(coder, "_on_device", lambda loc, block_size: True)
    monkeypatch.setattr(coder, "encode_tensors_device", device(5000))
    cell = "block_D192_cfg0__omega"
    idx, z = coder.encode_block(q, p, int(g["seed"]))
    assert coder.last_path == "host" and [int(i) for i in idx] == GOLD[f"{cell}_indices"].tolist()
    assert np.array_equal(z.numpy().reshape(-1), GOLD[f"{cell}_sample"])
    idx2, z2 = coder.encode(q, p, int(g["seed"]))
    assert idx2 == idx and torch.equal(z2, z)
