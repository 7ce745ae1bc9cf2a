"""The cells of tests/golden/refpy_gc_importance_alpha.npz (the reference's GaussianCoder at finite alpha) and what the tests of the
finite-alpha coder share: their inputs, the coder under test, the bit-for-bit comparison.  Test infrastructure: shared by
tests/test_gc_importance_alpha_host.py and tests/test_gc_importance_alpha_gpu.py."""
import os

import numpy as np
import torch

from conftest import GOLDEN_DIR

GOLD = np.load(os.path.join(GOLDEN_DIR, "refpy_gc_importance_alpha.npz"))
CELLS = [str(c) for c in GOLD["cells"]]
WIDE_CELLS = [str(c) for c in GOLD["wide_cells"]]
N = torch.distributions.Normal
KEYS = ("q_loc", "q_scale", "p_loc", "p_scale")


def cell_inputs(cell):
    """-> ([q_loc, q_scale, p_loc, p_scale] flat float32, Omega, seed) of a block cell or a wide cell of the golden file."""
    if cell in WIDE_CELLS:
        g = np.load(os.path.join(GOLDEN_DIR, "tensor_rvae_cfg2.npz"))
        return [g[k].reshape(-1)[:int(GOLD[f"{cell}_dims"])] for k in KEYS], float(g["kl_per_partition"]), int(g["seed"])
    g = np.load(os.path.join(GOLDEN_DIR, cell.split("__")[0] + ".npz"))
    return [g[k] for k in KEYS], float(g["kl_per_partition"]), int(g["seed"])


def coder_of(omega, bits, alpha, **kw):
    import irec
    return irec.GaussianCoder(kl_per_partition=omega, sampler=irec.ImportanceSampler(coding_bits=bits, alpha=alpha), **kw)


def same(a, b):
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and \
        np.array_equal(a[~np.isnan(a)].view(np.uint32), b[~np.isnan(b)].view(np.uint32))
