"""The sequential importance coder at FINITE alpha (the Gumbel-max branch, importance_sampling.py:67-72) without a GPU:

  * irec_gumbel_table_build -- the perturbations the kernels read -- is irec.coding.utils.stateless_gumbel_sample row by row, bit for
    bit where finite, NaN where it is NaN, zero in the padding;
  * the numpy referee with alpha (tests/gc_referee_alpha.py) returns the REFERENCE'S OWN outputs
    (tests/golden/refpy_gc_importance_alpha.npz: its unmodified GaussianCoder run over oracle/tfshim) on every cell;
  * irec.GaussianCoder's host loop returns the same outputs (the yardstick of scripts/bench_gc_importance.py --alpha);
  * the perturbation decides: cells differ from their alpha = inf twins;
  * alpha < 1 and NaN raise the reference's text.
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import gc_referee_alpha as RA
from conftest import GOLDEN_DIR
from gc_alpha_cases import CELLS, GOLD, KEYS, N, WIDE_CELLS, cell_inputs, coder_of, same


def cached_normal(oracle):
    @functools.lru_cache(maxsize=32)
    def normal(seed, count):
        return oracle.tf_random_normal(seed, count)
    return normal


@pytest.mark.parametrize("S", [1, 21, 256, 1177])
def test_gumbel_table_is_stateless_gumbel_sample_row_by_row(S):
    from irec import _lib
    from irec.coding.utils import stateless_gumbel_sample
    from irec.engine import build_gumbel_table
    seed, steps = 42, 3
    s_pad = -(-S // _lib.IREC_NORMAL_TABLE_PAD) * _lib.IREC_NORMAL_TABLE_PAD
    assert _lib.load().irec_gumbel_table_floats(S, steps) == steps * s_pad
    tab = build_gumbel_table(seed, S, steps)
    assert tab.shape == (steps, s_pad) and tab.dtype == np.float32
    n_nan = 0
    for j in range(steps):
        want = stateless_gumbel_sample((S,), seed + j + 1)
        got = tab[j, :S]
        assert np.array_equal(np.isnan(got), np.isnan(want)), j
        fin = ~np.isnan(want)
        assert np.array_equal(got[fin].view(np.uint32), want[fin].view(np.uint32)), j
        assert np.array_equal(tab[j, S:].view(np.uint32), np.zeros(s_pad - S, np.uint32)), j
        n_nan += int(np.isnan(got).sum())
    if S >= 256:
        assert 0.5 < n_nan / (steps * S) < 0.8        # the normal draw inside the double log: NaN for about two samples in three
    one = build_gumbel_table(seed, S, steps, n_threads=1)
    assert np.array_equal(one.view(np.uint32), tab.view(np.uint32))


def test_gumbel_table_refuses_bad_sizes():
    from irec import _lib
    lib = _lib.load()
    out = np.zeros(64, np.float32)
    for S, steps in ((0, 1), (-3, 1), (21, 0), (21, _lib.IREC_TABLE_STEPS_MAX + 1)):
        assert lib.irec_gumbel_table_floats(S, steps) == 0 and b"irec_gumbel_table_floats" in lib.irec_last_error()
        assert lib.irec_gumbel_table_build(1, S, steps, out.ctypes.data_as(ctypes.c_void_p), 1) == -1
    assert lib.irec_gumbel_table_floats(1 << 20, 4096) == 0 and b"IREC_TABLE_BYTES_HARD" in lib.irec_last_error()
    assert lib.irec_gumbel_table_build(1, 21, 2, None, 1) == -1 and b"null output" in lib.irec_last_error()
    assert not out.any()


def test_the_golden_file_holds_every_cell():
    import glob
    names = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "block_*.npz"))
                   if np.load(p)["q_loc"].size <= 1024)
    assert CELLS == [f"{n}__a{a}__{m}" for n in names for a in (1.0, 2.5) for m in ("omega", "bits8")]
    assert WIDE_CELLS == ["wide_D1500_S21", "wide_D1100_S1177"] and float(GOLD["tensor_alpha"]) == 1.0


def test_the_perturbation_decides():
    """Cells whose indices are not their alpha = inf twin's: a coder that ignored g would return the twin's."""
    differ = [c for c in CELLS + WIDE_CELLS if GOLD[f"{c}_indices"].tolist() != GOLD[f"{c}_indices_inf"].tolist()]
    assert len(differ) >= 1 and all(c in differ for c in WIDE_CELLS)
    assert GOLD["block_D192_cfg0__a1.0__bits8_indices"].tolist() == [50, 166]
    assert GOLD["block_D192_cfg0__a2.5__bits8_indices"].tolist() == [250, 101]
    assert GOLD["block_D192_cfg0__a1.0__bits8_indices_inf"].tolist() == [67, 101]
    assert np.array_equal(GOLD["tensor_K"], GOLD["tensor_inf_K"]) and not np.array_equal(GOLD["tensor_indices"], GOLD["tensor_inf_indices"])


@pytest.mark.parametrize("cell", CELLS + WIDE_CELLS)
def test_referee_is_the_reference(oracle, cell):
    stats, omega, seed = cell_inputs(cell)
    ref_idx = GOLD[f"{cell}_indices"].tolist()
    S = oracle.importance_n_samples(float(GOLD[f"{cell}_bits"]))
    K = oracle.num_aux(oracle.block_kl(*stats), omega)
    assert max(K, 1) == len(ref_idx)
    idx, z = RA.encode_block(*stats, seed, S, K, cached_normal(oracle), float(GOLD[f"{cell}_alpha"]))
    assert idx == ref_idx
    assert same(z, GOLD[f"{cell}_sample"])


@pytest.mark.parametrize("cell", CELLS + WIDE_CELLS)
def test_host_loop_is_the_reference(cell):
    stats, omega, seed = cell_inputs(cell)
    coder = coder_of(omega, float(GOLD[f"{cell}_bits"]), float(GOLD[f"{cell}_alpha"]))
    q, p = N(*(torch.from_numpy(s[None]) for s in stats[:2]), validate_args=False), \
        N(*(torch.from_numpy(s[None]) for s in stats[2:]), validate_args=False)
    idx, z = coder.encode_block(q, p, seed)
    assert coder.last_path == "host"
    assert [int(i) for i in idx] == GOLD[f"{cell}_indices"].tolist()
    assert same(z.numpy(), GOLD[f"{cell}_sample"])
    dec = coder.decode_block(p, idx, seed)
    assert same(dec.numpy(), GOLD[f"{cell}_decoded"]) and same(dec.numpy(), z.numpy())
    # the decoder never looks at alpha (importance_sampling.py:82-103)
    other = coder_of(omega, float(GOLD[f"{cell}_bits"]), np.inf)
    assert same(other.decode_block(p, idx, seed).numpy(), z.numpy())


def test_tensor_through_split_and_merge(oracle):
    g = np.load(os.path.join(GOLDEN_DIR, "tensor_rvae_cfg2.npz"))
    omega, seed, bs = float(g["kl_per_partition"]), int(g["seed"]), int(g["block_size"])
    want = [GOLD["tensor_indices"][r, :k].tolist() for r, k in enumerate(GOLD["tensor_K"])]
    S = oracle.importance_n_samples(omega / np.log(2))

    class Cached:
        tf_random_normal = staticmethod(cached_normal(oracle))

        def __getattr__(self, name):
            return getattr(oracle, name)

    ridx, rz = RA.encode_tensor(*(g[k] for k in KEYS), seed, S, omega, bs, Cached(), 1.0)
    assert ridx == want and same(rz, GOLD["tensor_sample"])
    coder = coder_of(omega, omega / np.log(2), 1.0, block_size=bs)
    q, p = N(torch.from_numpy(g["q_loc"]), torch.from_numpy(g["q_scale"]), validate_args=False), \
        N(torch.from_numpy(g["p_loc"]), torch.from_numpy(g["p_scale"]), validate_args=False)
    idx, z = coder.encode(q, p, seed)
    assert [[int(v) for v in ix] for ix in idx] == want and same(z.numpy(), GOLD["tensor_sample"])
    dec = coder.decode(p, idx, seed)
    assert same(dec.numpy(), GOLD["tensor_decoded"]) and same(dec.numpy(), z.numpy())


@pytest.mark.parametrize("alpha", [0.5, float("nan")])
def test_alpha_below_one_raises_the_references_text(alpha):
    from irec.coding.utils import CodingError
    stats, omega, seed = cell_inputs(CELLS[0])
    coder = coder_of(omega, 8.0, alpha)
    q, p = N(*(torch.from_numpy(s[None]) for s in stats[:2]), validate_args=False), \
        N(*(torch.from_numpy(s[None]) for s in stats[2:]), validate_args=False)
    with pytest.raises(CodingError, match=r"Alpha must be in the range \[1, inf\), but (0\.5|nan) was given!"):
        coder.encode_block(q, p, seed)
    with pytest.raises(CodingError, match=r"Alpha must be in the range \[1, inf\)"):
        coder.encode(q, p, seed)
