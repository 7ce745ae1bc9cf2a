"""Runs the REFERENCE'S OWN GaussianCoder(sampler=ImportanceSampler(..)) (rec.coding, imported unmodified from a checkout of
gergely-flamich/relative-entropy-coding) on the committed fixtures, with the TensorFlow / TFP calls it makes served by the numpy
stubs of oracle/tfshim, and writes what it returns as tests/golden/refpy_gc_importance.npz (numbers and names only).

Cells: every block_*.npz fixture of at most 1024 dims at coding_bits = Omega / ln 2 (what the reference's drivers use) and at
coding_bits = 8 -- encode_block and decode_block --, tensor_rvae_cfg2 through encode / decode with its block_size, and one
zero-KL block (q == p).

Build container only (the vectors travel, the reference does not).
Run:  python tests/golden/make_golden_gc_importance.py <path of the reference checkout>
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


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):      # the reference prints the KL of every block
        return fn(*a, **k)


def main():
    out = {"kind": "refpy_gc_importance",
           "note": "outputs of the reference's GaussianCoder(sampler=ImportanceSampler) run with oracle/tfshim; "
                   "see tests/golden/make_golden_gc_importance.py"}
    cells = []
    for path in sorted(glob.glob(os.path.join(HERE, "block_*.npz"))):
        g = np.load(path)
        if g["q_loc"].size > MAX_DIM:
            continue
        name = os.path.basename(path)[:-4]
        omega, seed = float(g["kl_per_partition"]), int(g["seed"])
        for mode, bits in (("omega", omega / np.log(2)), ("bits8", 8.0)):
            coder = GaussianCoder(kl_per_partition=omega, sampler=ImportanceSampler(coding_bits=bits))
            q = tfd.Normal(loc=tf.constant(g["q_loc"][None]), scale=tf.constant(g["q_scale"][None]))
            p = tfd.Normal(loc=tf.constant(g["p_loc"][None]), scale=tf.constant(g["p_scale"][None]))
            indices, sample = quiet(coder.encode_block, q, p, seed)
            indices = [int(i) for i in indices]
            decoded = quiet(coder.decode_block, p, list(indices), seed)
            cell = f"{name}__{mode}"
            out[f"{cell}_bits"] = np.float64(bits)
            out[f"{cell}_indices"] = np.array(indices, np.int32)
            out[f"{cell}_sample"] = sample.numpy().reshape(-1).astype(np.float32)
            out[f"{cell}_decoded"] = decoded.numpy().reshape(-1).astype(np.float32)
            out[f"{cell}_codelength"] = np.float64(coder.get_codelength(indices))
            cells.append(cell)
            print(f"{cell}: K = {len(indices)}  decode == encode: {np.array_equal(out[f'{cell}_sample'], out[f'{cell}_decoded'])}", flush=True)
    out["cells"] = np.array(cells)

    g = np.load(os.path.join(HERE, "tensor_rvae_cfg2.npz"))
    omega, seed = float(g["kl_per_partition"]), int(g["seed"])
    coder = GaussianCoder(kl_per_partition=omega, sampler=ImportanceSampler(coding_bits=omega / np.log(2)), block_size=int(g["block_size"]))
    q = tfd.Normal(loc=tf.constant(g["q_loc"]), scale=tf.constant(g["q_scale"]))
    p = tfd.Normal(loc=tf.constant(g["p_loc"]), scale=tf.constant(g["p_scale"]))
    indices, sample = quiet(coder.encode, q, p, seed=seed)
    decoded = quiet(coder.decode, p, [[int(v) for v in ix] for ix in indices], seed=seed)
    K = np.array([len(ix) for ix in indices], np.int32)
    flat = np.full((len(indices), K.max()), -1, np.int32)
    for r, ix in enumerate(indices):
        flat[r, :len(ix)] = [int(v) for v in ix]
    out["tensor_K"], out["tensor_indices"] = K, flat
    out["tensor_sample"] = sample.numpy().astype(np.float32)
    out["tensor_decoded"] = decoded.numpy().astype(np.float32)
    out["tensor_codelength"] = np.float64(sum(coder.get_codelength(ix) for ix in indices))
    print("tensor_rvae_cfg2: K per block", K.tolist(), " code length", float(out["tensor_codelength"]))

    g = np.load(os.path.join(HERE, "block_D192_cfg0.npz"))    # zero KL: q == p, K = 0, one index
    p = tfd.Normal(loc=tf.constant(g["p_loc"][None]), scale=tf.constant(g["p_scale"][None]))
    coder = GaussianCoder(kl_per_partition=3., sampler=ImportanceSampler(coding_bits=3. / np.log(2)))
    indices, sample = quiet(coder.encode_block, p, p, 42)
    out["zero_kl_indices"] = np.array([int(i) for i in indices], np.int32)
    out["zero_kl_sample"] = sample.numpy().reshape(-1).astype(np.float32)
    print("zero KL block: indices", out["zero_kl_indices"].tolist())
    np.savez_compressed(os.path.join(HERE, "refpy_gc_importance.npz"), **out)
    print("wrote refpy_gc_importance.npz")


if __name__ == "__main__":
    main()
