"""The one seeded TensorFlow output the reference itself holds: notebooks/Discrete REC.ipynb, cell 2 --
tf.random.set_seed(42); Bernoulli(probs=0.7).sample(100) -- parsed from the notebook's stored output into
ref_notebook_bernoulli42.npz (the 100 int32 bits, the global seed, probs and a note).  No cell source is stored.

Run (build container only):  python tests/golden/make_golden_notebook.py [path to the reference checkout]
"""
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CELL = 2


def main(ref_root):
    nb = json.load(open(os.path.join(ref_root, "notebooks", "Discrete REC.ipynb")))
    cell = nb["cells"][CELL]
    text = "".join(o["data"]["text/plain"] if isinstance(o["data"]["text/plain"], str) else "".join(o["data"]["text/plain"])
                   for o in cell["outputs"] if o.get("output_type") == "execute_result")
    assert "shape=(100,)" in text and "dtype=int32" in text, text[:200]
    body = text[text.index("array(") + len("array("):text.index("], dtype=int32") + 1]
    bits = np.array([int(v) for v in re.findall(r"-?\d+", body)], dtype=np.int32)
    assert bits.shape == (100,) and set(bits.tolist()) <= {0, 1}, bits
    np.savez(os.path.join(HERE, "ref_notebook_bernoulli42.npz"), bits=bits, global_seed=np.int64(42), probs=np.float32(0.7),
             note=np.array(f"notebooks/Discrete REC.ipynb, cell index {CELL}: stored output of Bernoulli(probs=0.7).sample(100) "
                           f"after tf.random.set_seed(42)"))
    print("wrote ref_notebook_bernoulli42.npz:", int(bits.sum()), "ones of 100")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "/root/reference")
