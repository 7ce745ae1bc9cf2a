"""Four corners of the seed domain through the REFERENCE'S OWN PYTHON (see make_golden_refpy.py for how it runs: the reference's
rec.coding imported unmodified, its TensorFlow / TFP calls served by the numpy stubs of oracle/tfshim): what
rec.coding.BeamSearchCoder.encode_block / decode_block returned for the 64-dim block of tests/seed_cases.py at the seeds M - 3, 2^31,
-1 and 2^40 + 5 (M = 2^31 - 1) -> tests/golden/refpy_seed_corners.npz.  Data only: inputs, seeds, indices, samples.

This pins the reference's Python seed arithmetic -- `seed + iteration` on a Python int of any size, handed to tf.random.set_seed and
to the op seed -- not the Philox primitives or TensorFlow's own truncation of the seed pair, which the stubs restate from the oracle.

Where a checkout of the reference is at hand.  Run:  python tests/golden/make_golden_refpy_seeds.py REFERENCE_DIR"""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
M = 2 ** 31 - 1
SEEDS = (M - 3, 2 ** 31, -1, 2 ** 40 + 5)
OMEGA, EXTRA_SAMPLES, BEAMS = 1.0, 3.0, 10           # S = int(exp(3)) = 20


def main(reference_dir):
    sys.path[:0] = [os.path.join(ROOT, "oracle", "tfshim"), ROOT, os.path.join(ROOT, "tests"), reference_dir]
    import tensorflow as tf                      # (the stub)
    import tensorflow_probability as tfp         # (the stub)
    from rec.coding import BeamSearchCoder       # (the REAL reference class)
    import seed_cases as SC
    from oracle import oracle as O
    assert os.path.abspath(reference_dir) in os.path.abspath(sys.modules[BeamSearchCoder.__module__].__file__)
    assert set(SEEDS) <= set(SC.SEEDS)
    mq, sq, mp, sp = (a[0] for a in SC.inputs(64, 1))
    out = {"kind": "refpy_seed_corners", "seeds": np.array(SEEDS, np.int64), "inputs": np.stack([mq, sq, mp, sp]),
           "settings": np.array([OMEGA, EXTRA_SAMPLES, BEAMS], np.float64)}
    agree = 0
    for k, seed in enumerate(SEEDS):
        coder = BeamSearchCoder(kl_per_partition=OMEGA, n_beams=BEAMS, extra_samples=EXTRA_SAMPLES)
        q = tfp.distributions.Normal(tf.constant(mq[None]), tf.constant(sq[None]))
        p = tfp.distributions.Normal(tf.constant(mp[None]), tf.constant(sp[None]))
        with contextlib.redirect_stdout(io.StringIO()):
            indices, sample = coder.encode_block(q, p, seed=seed)
            indices = [int(i) for i in indices]
            decoded = coder.decode_block(p, list(indices), seed=seed)
        oidx, _ = O.encode_block(mq, sq, mp, sp, seed, OMEGA, coder.n_samples, BEAMS, mode=O.CANONICAL)
        agree += int(oidx == indices)
        out["n_samples"] = np.int64(coder.n_samples)
        out[f"s{k}_indices"] = np.array(indices, np.int32)
        out[f"s{k}_sample"] = sample.numpy().reshape(-1).astype(np.float32)
        out[f"s{k}_decoded"] = decoded.numpy().reshape(-1).astype(np.float32)
        print(f"seed {seed}: S={coder.n_samples} K={len(indices)} indices {indices[:6]}... oracle==reference: {oidx == indices}", flush=True)
    np.savez_compressed(os.path.join(HERE, "refpy_seed_corners.npz"), **out)
    print(f"wrote refpy_seed_corners.npz; oracle (canonical) == reference python on {agree} / {len(SEEDS)}")


if __name__ == "__main__":
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "rec", "coding")):
        sys.exit("usage: make_golden_refpy_seeds.py REFERENCE_DIR  (the directory that holds rec/coding)")
    main(sys.argv[1])
