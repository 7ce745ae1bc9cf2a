"""Runs the REFERENCE'S OWN GaussianCoder(sampler=ImportanceSampler(coding_bits, alpha)) at FINITE alpha -- the Gumbel-max branch of
encode_gaussian_importance_sample (rec/coding/importance_sampling.py:67-72 over rec/coding/utils.py:9-12) -- on the committed
fixtures, with the TensorFlow / TFP calls it makes served by the numpy stubs of oracle/tfshim, and writes what it returns as
tests/golden/refpy_gc_importance_alpha.npz (numbers and names only).  The sibling of make_golden_gc_importance.py (alpha = inf).

Cells: every block_*.npz fixture of at most 1024 dims at alpha 1.0 and 2.5, at coding_bits = Omega / ln 2 and at coding_bits = 8
-- encode_block and decode_block --; tensor_rvae_cfg2 through encode / decode with its block_size at alpha 1.0; and two blocks of
more than 1024 dims cut from the front of tensor_rvae_cfg2 (flattened): 1500 dims at Omega / ln 2 (S = 21) and 1100 dims at
coding_bits = 10.2 (S = 1177), both at alpha 1.0.  Next to every cell lie the indices of its alpha = inf twin (same call, the
reference's default alpha): where they differ, the perturbation decided.

Build container only (the vectors travel, the reference does not).
Run:  python tests/golden/make_golden_gc_importance_alpha.py <path of the reference checkout>
"""
import contextlib
import glob
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFERENCE = os.path.abspath(sys.argv[1])
sys.path[:0] = [os.path.join(ROOT, "oracle", "tfshim"), ROOT, REFERENCE]

import tensorflow as tf                                  # noqa: E402  (the stub)
import tensorflow_probability as tfp                     # noqa: E402  (the stub)
from rec.coding.coder import GaussianCoder               # noqa: E402  (the REAL reference classes)
from rec.coding.samplers import ImportanceSampler        # noqa: E402

tfd = tfp.distributions
assert sys.modules[GaussianCoder.__module__].__file__.startswith(REFERENCE)
MAX_DIM = 1024
ALPHAS = (1.0, 2.5)
WIDE = (("wide_D1500_S21", 1500, None), ("wide_D1100_S1177", 1100, 10.2))   # (cell, dims, coding_bits or Omega / ln 2)


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):      # the reference prints the KL of every block
        return fn(*a, **k)


def code_block(out, cell, stats, omega, bits, seed, alpha):
    """encode_block / decode_block of one [1, D] block at `alpha`, and the indices of the same call at alpha = inf."""
    q = tfd.Normal(loc=tf.constant(stats[0][None]), scale=tf.constant(stats[1][None]))
    p = tfd.Normal(loc=tf.constant(stats[2][None]), scale=tf.constant(stats[3][None]))
    coder = GaussianCoder(kl_per_partition=omega, sampler=ImportanceSampler(coding_bits=bits, alpha=alpha))
    indices, sample = quiet(coder.encode_block, q, p, seed)
    indices = [int(i) for i in indices]
    decoded = quiet(coder.decode_block, p, list(indices), seed)
    twin = GaussianCoder(kl_per_partition=omega, sampler=ImportanceSampler(coding_bits=bits))
    inf_indices = [int(i) for i in quiet(twin.encode_block, q, p, seed)[0]]
    out[f"{cell}_bits"], out[f"{cell}_alpha"] = np.float64(bits), np.float64(alpha)
    out[f"{cell}_indices"] = np.array(indices, np.int32)
    out[f"{cell}_indices_inf"] = np.array(inf_indices, np.int32)
    out[f"{cell}_sample"] = sample.numpy().reshape(-1).astype(np.float32)
    out[f"{cell}_decoded"] = decoded.numpy().reshape(-1).astype(np.float32)
    print(f"{cell}: K = {len(indices)}  differs from alpha = inf: {indices != inf_indices}  decode == encode: "
          f"{np.array_equal(out[f'{cell}_sample'], out[f'{cell}_decoded'], equal_nan=True)}", flush=True)


def main():
    out = {"kind": "refpy_gc_importance_alpha",
           "note": "outputs of the reference's GaussianCoder(sampler=ImportanceSampler(alpha < inf)) run with oracle/tfshim; "
                   "see tests/golden/make_golden_gc_importance_alpha.py"}
    cells = []
    for path in sorted(glob.glob(os.path.join(HERE, "block_*.npz"))):
        g = np.load(path)
        if g["q_loc"].size > MAX_DIM:
            continue
        name = os.path.basename(path)[:-4]
        omega, seed = float(g["kl_per_partition"]), int(g["seed"])
        for alpha in ALPHAS:
            for mode, bits in (("omega", omega / np.log(2)), ("bits8", 8.0)):
                cell = f"{name}__a{alpha}__{mode}"
                code_block(out, cell, [g[k] for k in ("q_loc", "q_scale", "p_loc", "p_scale")], omega, bits, seed, alpha)
                cells.append(cell)
    out["cells"] = np.array(cells)

    g = np.load(os.path.join(HERE, "tensor_rvae_cfg2.npz"))
    omega, seed = float(g["kl_per_partition"]), int(g["seed"])
    q = tfd.Normal(loc=tf.constant(g["q_loc"]), scale=tf.constant(g["q_scale"]))
    p = tfd.Normal(loc=tf.constant(g["p_loc"]), scale=tf.constant(g["p_scale"]))
    for tag, alpha in (("tensor", 1.0), ("tensor_inf", np.inf)):
        coder = GaussianCoder(kl_per_partition=omega, sampler=ImportanceSampler(coding_bits=omega / np.log(2), alpha=alpha),
                              block_size=int(g["block_size"]))
        indices, sample = quiet(coder.encode, q, p, seed=seed)
        indices = [[int(v) for v in ix] for ix in indices]
        K = np.array([len(ix) for ix in indices], np.int32)
        flat = np.full((len(indices), K.max()), -1, np.int32)
        for r, ix in enumerate(indices):
            flat[r, :len(ix)] = ix
        out[f"{tag}_K"], out[f"{tag}_indices"] = K, flat
        if alpha == 1.0:
            decoded = quiet(coder.decode, p, [list(ix) for ix in indices], seed=seed)
            out["tensor_alpha"] = np.float64(alpha)
            out["tensor_sample"] = sample.numpy().astype(np.float32)
            out["tensor_decoded"] = decoded.numpy().astype(np.float32)
        print(f"tensor_rvae_cfg2 at alpha {alpha}: K per block", K.tolist(), flush=True)

    wide = []
    stats = [g[k].reshape(-1) for k in ("q_loc", "q_scale", "p_loc", "p_scale")]
    for cell, dims, bits in WIDE:
        out[f"{cell}_dims"] = np.int32(dims)
        code_block(out, cell, [s[:dims] for s in stats], omega, omega / np.log(2) if bits is None else bits, seed, 1.0)
        wide.append(cell)
    out["wide_cells"] = np.array(wide)
    np.savez_compressed(os.path.join(HERE, "refpy_gc_importance_alpha.npz"), **out)
    print("wrote refpy_gc_importance_alpha.npz")


if __name__ == "__main__":
    main()
