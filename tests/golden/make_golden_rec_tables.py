"""Golden vectors of the `.rec` wire format under empirical count tables, produced with the REAL reference code (its rec/io/utils.py on
its own Cython coder, which oracle/ref_io.py compiles into a temporary directory outside the tree and removes when this script ends),
as tests/golden/make_golden_rec.py does for the default models.  Only inputs and expected outputs are stored.

  ref_index_bytes   one file WRITTEN by the reference's write_compressed_code(..., index_counts_file=...): the index streams under an
                    index table, the counts under the default model.
  ours_both_bytes   one file written by irec.io.encode_files_ragged under an index table and count tables, which the reference's
                    read_compressed_code(..., num_aux_var_counts_file=, index_counts_file=) READ back to the lists it was made from
                    (asserted here, before anything is stored).
No reference-written file with count tables exists: with num_aux_var_counts_file its writer packs -1 for the largest partition counts
into an unsigned 'I' field, which struct refuses, so that branch of the reference cannot write at all (the `note` entry says so).

Run (build container only):  python tests/golden/make_golden_rec_tables.py
"""
import contextlib
import io
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "relative-entropy-coding_amd"), os.path.join(ROOT, "tests")]
from oracle import ref_io  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
NOTE = ("ref_index_bytes: written by the reference's write_compressed_code with index_counts_file.  ours_both_bytes: written by "
        "irec.io.encode_files_ragged with both kinds of table and read back by the reference's read_compressed_code to the same lists.  The "
        "reference cannot write a file with num_aux_var_counts_file: it packs -1 into an unsigned 'I' header field (struct.error).")


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        return fn(*a, **k)


def main():
    import rec_tables_cases as C
    from irec.io import SymbolTables, encode_files_ragged
    U = quiet(ref_io.load)
    rng = np.random.default_rng(2026)
    bpr = (4, 1, 7)
    tables = SymbolTables(C.index_tables()["geo20"], C.count_tables(len(bpr)))
    K, idx = C.make_rows(rng, 1, bpr, tables.index_counts, True)
    K = np.maximum(K, 1)                                          # (the reference's writer fails on a block without indices: its
                                                                  #  np.concatenate of an empty list turns the message into floats)
    lists = C.lists_of(K, idx, bpr)[0]
    with tempfile.TemporaryDirectory() as d:
        fi, fc, path = os.path.join(d, "i.npy"), os.path.join(d, "c.npy"), os.path.join(d, "x.rec")
        tables.save(fi, fc)
        quiet(U.write_compressed_code, path, C.SEED, C.SHAPE, C.BLOCK_SIZE, lists, 20, index_counts_file=fi)
        ref_bytes = open(path, "rb").read()
        back = quiet(U.read_compressed_code, path, index_counts_file=fi)
        assert [[list(map(int, b)) for b in blk] for blk in back[3]] == lists
        try:
            quiet(U.write_compressed_code, path, C.SEED, C.SHAPE, C.BLOCK_SIZE, lists, 20, num_aux_var_counts_file=fc, index_counts_file=fi)
            raise SystemExit("the reference wrote a file with count tables: store it, and rewrite the note")
        except Exception as e:                                    # struct.error: argument out of range
            print("reference writer with num_aux_var_counts_file:", type(e).__name__, e)
        blob, off = encode_files_ragged(C.SEED, C.SHAPE, C.BLOCK_SIZE, K, idx, 20, bpr, tables=tables)
        with open(path, "wb") as fh:
            fh.write(blob.tobytes())
        back = quiet(U.read_compressed_code, path, num_aux_var_counts_file=fc, index_counts_file=fi)
        assert (back[0], tuple(back[1]), back[2]) == (C.SEED, C.SHAPE, C.BLOCK_SIZE)
        assert [[list(map(int, b)) for b in blk] for blk in back[3]] == lists
    np.savez_compressed(os.path.join(HERE, "rec_tables_files.npz"), kind="rec_tables", note=NOTE, K=K, idx=idx, bpr=np.array(bpr),
                        max_index=20, meta=np.array([C.SEED, C.BLOCK_SIZE, *C.SHAPE], dtype=np.int64), index_counts=tables.index_counts,
                        count_counts=np.concatenate(tables.num_aux_var_counts), count_lengths=np.array([c.size for c in tables.num_aux_var_counts]),
                        ref_index_bytes=np.frombuffer(ref_bytes, dtype=np.uint8), ours_both_bytes=np.array(blob))
    print("reference-written file (index table):", len(ref_bytes), "bytes; ours under both tables, read by the reference:", blob.size, "bytes")


if __name__ == "__main__":
    main()
