"""The sequential importance coder on blocks of MORE than 1024 dims, without a GPU: the numpy referee of the arithmetic contract
(tests/gc_referee.py) and irec.GaussianCoder's host loop return the REFERENCE'S OWN outputs
(tests/golden/refpy_gc_importance_wide.npz: its unmodified GaussianCoder run over oracle/tfshim) bit for bit, on every cell -- the
four wide block fixtures at two sample counts, and tensor_rvae_cfg2 at block_size None (one block of 8192 dims), 3000 and 1500.
These pin the referee that tests/test_gc_importance_wide_gpu.py holds the wide kernel to; they pass with or without that kernel.
"""
import functools
import glob
import os

import numpy as np
import pytest
import torch

import gc_referee as R
from conftest import GOLDEN_DIR

pytestmark = [pytest.mark.both_suites, pytest.mark.usefixtures("suite")]

GOLD = np.load(os.path.join(GOLDEN_DIR, "refpy_gc_importance_wide.npz"))
CELLS = [str(c) for c in GOLD["cells"]]
BLOCK_SIZES = [None if b < 0 else int(b) for b in GOLD["tensor_block_sizes"]]
N = torch.distributions.Normal
KEYS = ("q_loc", "q_scale", "p_loc", "p_scale")


def _coder(omega, bits, **kw):
    import irec
    return irec.GaussianCoder(kl_per_partition=omega, sampler=irec.ImportanceSampler(coding_bits=bits), **kw)


def _dists(g, lead=True):
    a = [torch.from_numpy(np.asarray(g[k])[None] if lead else np.asarray(g[k])) for k in KEYS]
    return N(a[0], a[1], validate_args=False), N(a[2], a[3], validate_args=False)


class _Cached:
    """The oracle with its normal stream memoised (every block of a call reads the same draws)."""

    def __init__(self, oracle):
        self._o, self.tf_random_normal = oracle, functools.lru_cache(maxsize=4)(oracle.tf_random_normal)

    def __getattr__(self, name):
        return getattr(self._o, name)


def _tensor_want(bs):
    tag = f"tensor_bs{bs}"
    return [GOLD[f"{tag}_indices"][r, :k].tolist() for r, k in enumerate(GOLD[f"{tag}_K"])], GOLD[f"{tag}_sample"], GOLD[f"{tag}_decoded"]


def test_the_golden_file_holds_every_cell():
    names = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "block_*.npz"))
                   if np.load(p)["q_loc"].size > 1024)
    assert names == ["block_D1500_large_b10", "block_D2100_large_b32", "block_D2500_large", "block_D3200_large_b30"]
    assert CELLS == [f"{n}__{m}" for n in names for m in ("omega", "bits8")]
    assert [len(GOLD[f"{c}_indices"]) for c in CELLS] == [12, 12, 17, 17, 19, 19, 25, 25]
    assert BLOCK_SIZES == [None, 3000, 1500]
    assert [GOLD[f"tensor_bs{b}_K"].tolist() for b in BLOCK_SIZES] == [[62], [24, 22, 16], [12, 12, 11, 11, 11, 6]]


@pytest.mark.parametrize("cell", CELLS)
def test_referee_is_the_reference(oracle, cell):
    g = np.load(os.path.join(GOLDEN_DIR, cell.split("__")[0] + ".npz"))
    ref_idx = GOLD[f"{cell}_indices"].tolist()
    S = oracle.importance_n_samples(float(GOLD[f"{cell}_bits"]))
    K = oracle.num_aux(oracle.block_kl(*(g[k] for k in KEYS)), float(g["kl_per_partition"]))
    assert max(K, 1) == len(ref_idx)          # the canonical K (irec_block_kl) is the reference's
    idx, z = R.encode_block(*(g[k] for k in KEYS), int(g["seed"]), S, K, oracle.tf_random_normal)
    assert idx == ref_idx
    assert np.array_equal(z, GOLD[f"{cell}_sample"])
    dec = R.decode_block(g["p_loc"], g["p_scale"], idx, int(g["seed"]), S, oracle.tf_random_normal)
    assert np.array_equal(dec, GOLD[f"{cell}_decoded"]) and np.array_equal(dec, z)


@pytest.mark.parametrize("cell", CELLS)
def test_host_path_is_the_reference(cell):
    g = np.load(os.path.join(GOLDEN_DIR, cell.split("__")[0] + ".npz"))
    coder = _coder(float(g["kl_per_partition"]), float(GOLD[f"{cell}_bits"]))
    q, p = _dists(g)
    idx, z = coder.encode_block(q, p, int(g["seed"]))
    assert coder.last_path == "host"
    assert [int(i) for i in idx] == GOLD[f"{cell}_indices"].tolist()
    assert z.shape == q.loc.shape and np.array_equal(z.numpy().reshape(-1), GOLD[f"{cell}_sample"])
    keep = list(idx)
    dec = coder.decode_block(p, idx, int(g["seed"]))
    assert coder.last_path == "host" and idx == keep
    assert torch.equal(dec, z) and np.array_equal(dec.numpy().reshape(-1), GOLD[f"{cell}_decoded"])


@pytest.mark.parametrize("bs", BLOCK_SIZES)
def test_tensor_referee_is_the_reference(oracle, bs):
    g = np.load(os.path.join(GOLDEN_DIR, "tensor_rvae_cfg2.npz"))
    omega, seed = float(g["kl_per_partition"]), int(g["seed"])
    want, sample, decoded = _tensor_want(bs)
    S = oracle.importance_n_samples(omega / np.log(2))
    assert S == 21
    ridx, rz = R.encode_tensor(*(g[k] for k in KEYS), seed, S, omega, bs, _Cached(oracle))
    assert ridx == want and np.array_equal(rz, sample) and np.array_equal(sample, decoded)


@pytest.mark.parametrize("bs", BLOCK_SIZES)
def test_tensor_host_path_is_the_reference(bs):
    g = np.load(os.path.join(GOLDEN_DIR, "tensor_rvae_cfg2.npz"))
    omega, seed = float(g["kl_per_partition"]), int(g["seed"])
    want, sample, decoded = _tensor_want(bs)
    coder = _coder(omega, omega / np.log(2), block_size=bs)
    q, p = _dists(g, lead=False)
    idx, z = coder.encode(q, p, seed)
    assert coder.last_path == "host"
    assert [[int(v) for v in ix] for ix in ([idx] if bs is None else idx)] == want
    assert np.array_equal(z.numpy(), sample)
    dec = coder.decode(p, idx, seed)
    assert coder.last_path == "host" and torch.equal(dec, z) and np.array_equal(dec.numpy(), decoded)
