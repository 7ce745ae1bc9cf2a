"""Runs the REFERENCE'S OWN GaussianCoder(sampler=ImportanceSampler(..)) (rec.coding, imported unmodified from a checkout of
gergely-flamich/relative-entropy-coding) on the committed fixtures of MORE than 1024 dims, with the TensorFlow / TFP calls it
makes served by the numpy stubs of oracle/tfshim, and writes what it returns as tests/golden/refpy_gc_importance_wide.npz
(numbers and names only).  The sibling of make_golden_gc_importance.py, which stops at 1024 dims.

Cells: every block_*.npz fixture of more than 1024 dims at coding_bits = Omega / ln 2 (what the reference's drivers use) and at
coding_bits = 8 -- encode_block and decode_block --, and tensor_rvae_cfg2 through encode / decode at block_size None (one block
of 8192 dims), 3000 and 1500 (five wide blocks and one of 692 dims).

Build container only (the vectors travel, the reference does not).
Run:  python tests/golden/make_golden_gc_importance_wide.py <path of the reference checkout>
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
MAX_NARROW_DIM = 1024
TENSOR_BLOCK_SIZES = (None, 3000, 1500)


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):      # the reference prints the KL of every block
        return fn(*a, **k)


def main():
    out = {"kind": "refpy_gc_importance_wide",
           "note": "outputs of the reference's GaussianCoder(sampler=ImportanceSampler) on blocks of more than 1024 dims, run with "
                   "oracle/tfshim; see tests/golden/make_golden_gc_importance_wide.py"}
    cells = []
    for path in sorted(glob.glob(os.path.join(HERE, "block_*.npz"))):
        g = np.load(path)
        if g["q_loc"].size <= MAX_NARROW_DIM:
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
            cells.append(cell)
            print(f"{cell}: D = {g['q_loc'].size}  K = {len(indices)}  decode == encode: "
                  f"{np.array_equal(out[f'{cell}_sample'], out[f'{cell}_decoded'])}", flush=True)
    out["cells"] = np.array(cells)

    g = np.load(os.path.join(HERE, "tensor_rvae_cfg2.npz"))
    omega, seed = float(g["kl_per_partition"]), int(g["seed"])
    q = tfd.Normal(loc=tf.constant(g["q_loc"]), scale=tf.constant(g["q_scale"]))
    p = tfd.Normal(loc=tf.constant(g["p_loc"]), scale=tf.constant(g["p_scale"]))
    for bs in TENSOR_BLOCK_SIZES:
        coder = GaussianCoder(kl_per_partition=omega, sampler=ImportanceSampler(coding_bits=omega / np.log(2)), block_size=bs)
        indices, sample = quiet(coder.encode, q, p, seed=seed)
        if bs is None:                                   # encode returns encode_block's flat list
            indices = [int(v) for v in indices]
            decoded = quiet(coder.decode, p, list(indices), seed=seed)
            indices = [indices]
        else:
            indices = [[int(v) for v in ix] for ix in indices]
            decoded = quiet(coder.decode, p, [list(ix) for ix in indices], seed=seed)
        K = np.array([len(ix) for ix in indices], np.int32)
        flat = np.full((len(indices), K.max()), -1, np.int32)
        for r, ix in enumerate(indices):
            flat[r, :len(ix)] = ix
        tag = f"tensor_bs{bs}"
        out[f"{tag}_K"], out[f"{tag}_indices"] = K, flat
        out[f"{tag}_sample"] = sample.numpy().astype(np.float32)
        out[f"{tag}_decoded"] = decoded.numpy().astype(np.float32)
        print(f"tensor_rvae_cfg2, block_size {bs}: K per block", K.tolist(), flush=True)
    out["tensor_block_sizes"] = np.array([-1 if bs is None else bs for bs in TENSOR_BLOCK_SIZES], np.int32)
    np.savez_compressed(os.path.join(HERE, "refpy_gc_importance_wide.npz"), **out)
    print("wrote refpy_gc_importance_wide.npz")


if __name__ == "__main__":
    main()
