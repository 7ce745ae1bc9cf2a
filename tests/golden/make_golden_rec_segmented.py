"""Writes tests/golden/rec_segmented_files.npz: segmented .rec files (NAME.recs) as the Python restatement of
tests/rec_segmented_cases.py makes them (one arithmetic-coder call per stream, the fields packed with `struct`), with the rows that
went in.  Structures (1, 4) and (3, 1, 5), segment_blocks = 2, three images each.  Only inputs and expected outputs are stored.

Run from the repository root:  python tests/golden/make_golden_rec_segmented.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "relative-entropy-coding_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import rec_segmented_cases as C  # noqa: E402


def main():
    rng = np.random.default_rng(2027)
    out = {"names": np.array(["1_4", "3_1_5"]), "kind": np.array("rec_segmented")}
    for name, bpr, mk, S in (("1_4", (1, 4), 7, 36), ("3_1_5", (3, 1, 5), 12, 20)):
        K, idx = C.rows_of(rng, bpr, mk, 3, S, 2)
        files = [C.file_of(K[i], idx[i], bpr, 2, S) for i in range(3)]
        out.update({f"{name}_bpr": np.array(bpr, np.int32), f"{name}_g": np.array(2, np.int32),
                    f"{name}_meta": np.array([C.SEED, C.BLOCK_SIZE, S, *C.SHAPE], np.int64), f"{name}_K": K, f"{name}_idx": idx,
                    f"{name}_bytes": np.frombuffer(b"".join(files), dtype=np.uint8),
                    f"{name}_offsets": np.concatenate([[0], np.cumsum([len(f) for f in files])]).astype(np.int64)})
    np.savez_compressed(os.path.join(HERE, "rec_segmented_files.npz"), **out)


if __name__ == "__main__":
    main()
