"""CPU tests of the .rec coder under empirical symbol tables: the host-thread entry points (irec_rec_encode_files_tables /
irec_rec_decode_files_tables) and the core's host hooks (the lane functions of csrc/irec_rec.hip's kernels over host memory in a
plain loop) against the reference-shaped Python writer and reader (_write_compressed_code_py / _read_compressed_code_py: one
ArithmeticCoder call per stream, which tests/golden/rec_ac_vectors.npz pins to the compiled reference on non-uniform tables), the
table builder, hostile tables, damaged flagged files, the histograms and the fitter.  Every comparison is byte or integer equality."""
import math
import os

import numpy as np
import pytest

import rec_tables_cases as C

pytestmark = [pytest.mark.both_suites, pytest.mark.usefixtures("suite")]

CASES = range(len(C.case_names()))


def _encode(c, tables="own", **kw):
    from irec.io import utils as U
    return U.encode_files_ragged(C.SEED, C.SHAPE, C.BLOCK_SIZE, c["K"], c["idx"], c["max_index"], c["bpr"],
                                 tables=c["tables"] if tables == "own" else tables, **kw)


def test_the_staging_cut_is_the_headers():
    from irec import _lib
    text = open(os.path.join(os.path.dirname(__file__), "..", "include", "irec.h")).read()
    assert f"#define IREC_REC_TABLE_LDS_SYMBOLS {C.LDS_SYMBOLS}\n" in text and _lib.REC_TABLE_LDS_SYMBOLS == C.LDS_SYMBOLS
    assert "#define IREC_REC_RAGGED_MAX_RES 64\n" in text and len(C.LAYOUTS["2x64ones"][1]) == 64
    assert _lib.IREC_REC_E_TABLE == 19 and "IREC_REC_E_TABLE = 19" in text


@pytest.mark.parametrize("which", CASES, ids=C.case_names())
def test_host_files_and_core_files_equal_the_python_writer(which):
    c = C.cases()[which]
    total = int(c["offsets"][-1])
    for threads in (1, 16):
        blob, off = _encode(c, n_threads=threads)
        assert np.array_equal(off, c["offsets"])
        for i, raw in enumerate(c["files"]):
            assert blob[off[i]:off[i + 1]].tobytes() == raw, f"image {i}"
    for strided in (False, True):
        out, off, status = C.core_encode(c["K"], c["idx"], c["max_index"], c["bpr"], C.raw_tables(c["tables"]), total, strided)
        assert (status == 0).all() and np.array_equal(off, c["offsets"])
        assert np.array_equal(out[:total], c["blob"]) and (out[total:] == 0xAB).all()      # the writer's bytes, and not one byte more
    out, off, status = C.core_encode(c["K"], c["idx"], c["max_index"], c["bpr"], C.raw_tables(c["tables"]), total - 1)
    assert off[-1] == total and (status == 0).all() and (out == 0xAB).all()              # one byte short: the size, and nothing written
    t = c["tables"]
    flags = np.frombuffer(c["blob"][22:26].tobytes(), dtype="<u2")
    assert flags.tolist() == [int(t.count_cum is not None), int(t.index_cum is not None)]
    if t.count_cum is not None:
        R = len(c["bpr"])
        assert (np.frombuffer(c["blob"][28 + 12 * R:28 + 16 * R].tobytes(), dtype="<u4") == 0xFFFFFFFF).all()


@pytest.mark.parametrize("which", CASES, ids=C.case_names())
def test_host_reader_and_core_reader_equal_the_python_reader(which, tmp_path):
    from irec.io import utils as U
    c = C.cases()[which]
    t = c["tables"]
    h, w, ch = C.SHAPE
    want_hdr = np.array([C.SEED, C.BLOCK_SIZE, c["max_index"], h, w, ch, t.count_cum is not None, t.index_cum is not None, len(c["bpr"])], dtype=np.uint32)
    hdr, K, idx = U.decode_files_ragged(c["blob"], c["offsets"], c["bpr"], C.MAX_K, tables=t)
    assert np.array_equal(K, c["K"]) and np.array_equal(idx, c["idx_zeroed"]) and (hdr == want_hdr).all()
    hdr2, K2, idx2, status = C.core_decode(c["blob"], c["offsets"], c["bpr"], C.MAX_K, C.raw_tables(t))
    assert (status == 0).all() and np.array_equal(K2, K) and np.array_equal(idx2, idx) and np.array_equal(hdr2, hdr)
    fi = str(tmp_path / "i.npy") if t.index_counts is not None else None
    fc = str(tmp_path / "c.npy") if t.num_aux_var_counts is not None else None
    t.save(fi, fc)
    want = C.lists_of(c["K"], c["idx"], c["bpr"])
    for i, raw in enumerate(c["files"][:4]):
        path = tmp_path / "one.rec"
        path.write_bytes(raw)
        seed, shape, bs, blocks = U._read_compressed_code_py(str(path), 28, fc, fi)
        assert (seed, tuple(shape), bs) == (C.SEED, C.SHAPE, C.BLOCK_SIZE) and blocks == want[i] == C.lists_of(K[i:i + 1], idx[i:i + 1], c["bpr"])[0]
    assert U.rec_files_max_K(c["blob"], c["offsets"], t) == max(1, t.max_K or 1, int(c["K"].max()) if t.count_cum is None else 0)


def test_symbol_tables_save_and_load_the_references_npy_forms(tmp_path):
    from irec.io import SymbolTables
    t = C.cases()[C.case_names().index("5x4_1_7-both")]["tables"]
    fi, fc = str(tmp_path / "i.npy"), str(tmp_path / "c.npy")
    t.save(fi, fc)
    a, b = np.load(fi), np.load(fc, allow_pickle=True)                    # what the reference's two np.load calls read
    assert a.ndim == 1 and a.dtype.kind == "i" and b.dtype == object and [len(x) for x in b] == [11, 3, 16]
    u = SymbolTables.load(fi, fc)
    assert np.array_equal(u.index_cum, t.index_cum) and np.array_equal(u.count_cum, t.count_cum) and np.array_equal(u.count_first, t.count_first)
    assert u.max_K == 14 and u.n_res_blocks == 3 and u.n_index_symbols == 21
    assert np.array_equal(t.index_cum, np.concatenate([[0], np.cumsum(t.index_counts)]).astype(np.uint32))
    with pytest.raises(ValueError, match="count tables for 3 residual blocks"):
        _encode(C.cases()[C.case_names().index("3x3_3-index")], tables=t)


def test_one_call_reads_flagged_and_unflagged_files_and_no_tables_is_status_5():
    from irec.io import utils as U
    c = C.cases()[C.case_names().index("5x4_1_7-both")]
    plain, off_p = U.encode_files_ragged(C.SEED, C.SHAPE, C.BLOCK_SIZE, c["K"], c["idx"], c["max_index"], c["bpr"])
    from irec.io import SymbolTables
    same, off_s = _encode(c, tables=SymbolTables())                       # the new entry points without tables: the old entry points' bytes
    assert np.array_equal(same, plain) and np.array_equal(off_s, off_p)
    index_only = C.cases()[C.case_names().index("5x4_1_7-index")]
    mixed = np.concatenate([c["blob"], plain, _encode(c, tables=SymbolTables(c["tables"].index_counts, None))[0]])
    sizes = np.concatenate([np.diff(c["offsets"]), np.diff(off_p), np.diff(_encode(c, tables=SymbolTables(c["tables"].index_counts, None))[1])])
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    hdr, K, idx = U.decode_files_ragged(mixed, off, c["bpr"], C.MAX_K, tables=c["tables"])
    assert np.array_equal(K, np.concatenate([c["K"]] * 3)) and np.array_equal(idx, np.concatenate([c["idx_zeroed"]] * 3))
    assert hdr[:, 6].tolist() == [1] * 5 + [0] * 10 and hdr[:, 7].tolist() == [1] * 5 + [0] * 5 + [1] * 5
    assert index_only["tables"].index_cum is not None
    # a flagged file and no table for that kind: status 5, through every reader
    with pytest.raises(ValueError, match=r"empirical count tables.*\(image 0\)"):
        U.decode_files_ragged(c["blob"], c["offsets"], c["bpr"], C.MAX_K)
    with pytest.raises(ValueError, match=r"empirical count tables.*\(image 0\)"):
        U.decode_files_ragged(c["blob"], c["offsets"], c["bpr"], C.MAX_K, tables=SymbolTables(c["tables"].index_counts, None))
    _, K5, idx5, status = C.core_decode(mixed, off, c["bpr"], C.MAX_K, (None, 0, None, None, 0))
    assert status.tolist() == [5] * 5 + [0] * 5 + [5] * 5 and not K5[status == 5].any() and not idx5[status == 5].any()
    assert np.array_equal(K5[5:10], c["K"])


def test_a_value_outside_its_table_names_the_image_and_leaves_no_bytes():
    from irec.io import utils as U
    c = C.cases()[C.case_names().index("5x4_1_7-both")]
    total = int(c["offsets"][-1])
    idx = c["idx"].copy()
    idx[3, 0, 0] = 20                                                    # 20 values: 0 .. 19
    K = c["K"].copy()
    K[3, 0] = max(K[3, 0], 1)
    with pytest.raises(ValueError, match=r"index does not fit.*\(image 3\)"):
        U.encode_files_ragged(C.SEED, C.SHAPE, C.BLOCK_SIZE, K, idx, c["max_index"], c["bpr"], tables=c["tables"])
    out, off, status = C.core_encode(K, idx, c["max_index"], c["bpr"], C.raw_tables(c["tables"]), 2 * total)
    assert status.tolist() == [0, 0, 0, 2, 0] and off[4] == off[3]
    K = c["K"].copy()
    K[1, 4] = 2                                                          # residual block 1 has a 3-symbol table: K <= 1
    with pytest.raises(ValueError, match=r"K out of range \(image 1\)"):
        U.encode_files_ragged(C.SEED, C.SHAPE, C.BLOCK_SIZE, K, c["idx"], c["max_index"], c["bpr"], tables=c["tables"])
    out, off, status = C.core_encode(K, c["idx"], c["max_index"], c["bpr"], C.raw_tables(c["tables"]), 2 * total)
    assert status.tolist() == [0, 1, 0, 0, 0] and off[2] == off[1]
    assert out[off[2]:off[3]].tobytes() == c["files"][2]                 # the other images are what they would be without it


def test_tables_build_refuses_what_the_coder_cannot_code_under():
    from irec import _lib
    from irec.io import SymbolTables
    lib = _lib.load()
    for counts, why in (([3, 0, 2], "at least 1"), ([1, 1 << 30], "2\\^30"), ([5], "n_symbols >= 2"), ([2, -1], "at least 1")):
        cum = np.full(len(counts) + 1, 0xAAAAAAAA, dtype=np.uint32)
        a = np.array(counts, dtype=np.int64)
        assert lib.irec_rec_tables_build(a.ctypes.data, a.size, cum.ctypes.data) == _lib.IREC_E_INVALID
        assert (cum == 0xAAAAAAAA).all()
        with pytest.raises(ValueError, match=why):
            SymbolTables(counts)
    assert SymbolTables([1, (1 << 30) - 1]).index_cum.tolist() == [0, 1, 1 << 30]          # a total of exactly 2^30 is a table


HOSTILE = {"cum0_not_0": [1, 5, 9, 12], "repeated": [0, 5, 5, 12], "descending": [0, 9, 5, 12], "total_over_2p30": [0, 5, 9, (1 << 30) + 1],
           "all_zero": [0, 0, 0, 0], "descending_end": [0, 5, 9, 3]}


@pytest.mark.parametrize("name", HOSTILE)
def test_hostile_tables_give_status_19_and_return(name):
    """cum arrays that irec_rec_tables_build would never make, handed straight to the host core: IREC_REC_E_TABLE for every image whose
    streams meet the bad entry, no bytes for it, and the call returns."""
    from irec import _lib
    lib = _lib.load()
    c = C.cases()[C.case_names().index("3x3_3-both")]
    cum = np.array(HOSTILE[name], dtype=np.uint32)                       # 3 symbols: values 0 and 1
    K = np.minimum(c["K"], 1).astype(np.int32)
    K[:, [0, 1, 3]], K[:, [2, 4]] = 1, 0                                 # every count stream codes the values 0 and 1,
    idx = (c["idx"] % 2).astype(np.int32)
    idx[:, 0, 0], idx[:, 1, 0] = 1, 0                                    # every image's first index stream too
    good = C.raw_tables(c["tables"])
    first2 = np.array([0, 4, 8], dtype=np.int32)
    for raw in ((cum, 3, None, None, 0), (None, 0, np.concatenate([cum, cum]), first2, 8), (good[0], good[1], np.concatenate([cum, cum]), first2, 8)):
        out, off, status = C.core_encode(K, idx, 2, c["bpr"], raw, 4096)
        assert (status == _lib.IREC_REC_E_TABLE).all() and (off == 0).all() and (out == 0xAB).all()
        blob = np.full(4096, 0xAB, dtype=np.uint8)
        offsets, st = np.zeros(4, dtype=np.int64), np.full(3, -1, dtype=np.int32)
        bpr = np.array(c["bpr"], dtype=np.int32)
        total = lib.irec_rec_encode_files_tables(C.SEED, C.BLOCK_SIZE, 2, *C.SHAPE, 3, 2, bpr.ctypes.data, C.MAX_K, K.ctypes.data, idx.ctypes.data,
                                                 C._ptr(raw[0]), raw[1], C._ptr(raw[2]), C._ptr(raw[3]), raw[4], blob.ctypes.data, blob.size,
                                                 offsets.ctypes.data, st.ctypes.data, 1)
        assert total == 0 and (st == _lib.IREC_REC_E_TABLE).all() and (blob == 0xAB).all()
    # the reader: files written under a good table of the same size, read under the hostile one
    from irec.io import SymbolTables
    t = SymbolTables([4, 5, 3], [[4, 5, 3]] * 2)
    files, off_f = _encode(dict(c, K=K, idx=idx, max_index=2), tables=t)
    for raw in ((cum, 3, t.count_cum, t.count_first, t.count_cum.size), (t.index_cum, 3, np.concatenate([cum, cum]), first2, 8)):
        hdr, K2, idx2, status = C.core_decode(files, off_f, c["bpr"], C.MAX_K, raw)
        if name not in ("repeated", "descending"):                       # (those two: the search never lands on the empty interval, the
            assert (status == _lib.IREC_REC_E_TABLE).all()               #  stream just decodes to other values or fails as a corrupt one)
        assert ((status >= 0) & (status <= 19)).all()
        assert not hdr[status != 0].any() and not K2[status != 0].any() and not idx2[status != 0].any()
    # a count_first that leaves count_cum, or describes a table of no symbol
    for bad_first in ([0, 4, 9], [0, 0, 4], [-1, 4, 8], [4, 0, 8]):
        raw = (None, 0, t.count_cum, np.array(bad_first, dtype=np.int32), 8)
        _, _, status = C.core_encode(K, idx, 2, c["bpr"], raw, 4096)
        assert (status == _lib.IREC_REC_E_TABLE).all()
        _, _, _, status = C.core_decode(files, off_f, c["bpr"], C.MAX_K, (t.index_cum, 3) + raw[2:])
        assert (status == _lib.IREC_REC_E_TABLE).all()


def test_damaged_flagged_files_core_reader_equals_the_python_reader():
    d = C.damaged_set()
    hdr, K, idx, status = C.core_decode(d["blob"], d["offsets"], C.DAMAGED_BPR, C.DAMAGED_MK, C.raw_tables(d["tables"]))
    assert np.array_equal(status == 0, d["ok"])
    assert int(d["ok"].sum()) >= 200 and int((~d["ok"]).sum()) >= d["n_prefix"] + 500
    assert np.array_equal(hdr, d["hdr"]) and np.array_equal(K, d["K"]) and np.array_equal(idx, d["idx"])      # (a refused image: all zero)
    assert (status[:d["n_prefix"]] != 0).all()


def _bincount_restatement(K, idx, bpr, niv, ncv):
    T, first = sum(bpr), np.concatenate([[0], np.cumsum(bpr)])
    good = (K >= 0) & (K <= idx.shape[2]) & (K < ncv)
    live = (np.arange(idx.shape[2])[None, None, :] < K[..., None]) & good[..., None]
    vals = idx[live]
    inr = (vals >= 0) & (vals < niv)
    index = np.bincount(vals[inr], minlength=niv).astype(np.uint64)
    counts = np.stack([np.bincount(K[:, first[r]:first[r + 1]][good[:, first[r]:first[r + 1]]], minlength=ncv) for r in range(len(bpr))]).astype(np.uint64)
    streams = np.array([K.shape[0] * len(bpr)] + [K.shape[0]] * len(bpr), dtype=np.uint64)
    return index, counts, streams, np.uint64((~good).sum() + (~inr).sum())


def test_histograms_equal_bincount_and_accumulate():
    from irec.io import hist_rows
    rng = np.random.default_rng(5)
    bpr = (4, 1, 7)
    K = rng.integers(-1, 12, (40, 12)).astype(np.int32)                  # -1, and 10 and 11 above max_K = 9
    idx = rng.integers(-2, 25, (40, 12, 9)).astype(np.int32)             # below 0, and 20 .. 24 outside 20 values
    h = hist_rows(K, idx, bpr, 20, 8)                                    # K = 8, 9 outside 8 count values
    want = _bincount_restatement(K, idx, bpr, 20, 8)
    assert np.array_equal(h.index, want[0]) and np.array_equal(h.counts, want[1]) and np.array_equal(h.streams, want[2]) and h.rejected[0] == want[3]
    assert want[3] > 50 and h.index.dtype == np.uint64
    K2, idx2 = np.roll(K, 3, axis=0)[:7], np.roll(idx, 5, axis=0)[:7]
    h2 = hist_rows(K2, idx2, bpr, 20, 8, into=h)
    more = _bincount_restatement(K2, idx2, bpr, 20, 8)
    assert h2 is h and all(np.array_equal(a, b + c) for a, b, c in zip((h.index, h.counts, h.streams), want, more)) and h.rejected[0] == want[3] + more[3]
    with pytest.raises(ValueError, match="other sizes"):
        hist_rows(K, idx, bpr, 21, 8, into=h)


def test_tables_from_histograms_is_integer_and_fits_the_coder():
    from irec.io import RowHistograms, tables_from_histograms
    hist = np.array([5, 0, 3, 1 << 40, 7, (1 << 40) + 9, 0], dtype=np.uint64)
    h = RowHistograms(hist, np.stack([hist[:4], hist[3:]]), np.array([11, 0, 1 << 41], dtype=np.uint64), np.zeros(1, np.uint64))
    t = tables_from_histograms(h)
    small = tables_from_histograms(RowHistograms(hist[:3], hist[None, :3], np.array([11, 4], dtype=np.uint64), np.zeros(1, np.uint64)))
    assert small.index_counts.tolist() == [11, 6, 1, 4] and small.num_aux_var_counts[0].tolist() == [4, 6, 1, 4]      # c[0] = streams, c[m] = 1 + hist
    for c, raw, streams in ((t.index_counts, hist, 11), (t.num_aux_var_counts[0], hist[:4], 1), (t.num_aux_var_counts[1], hist[3:], 1 << 41)):
        full = np.array([max(1, streams)] + [1 + int(v) for v in raw], dtype=object)
        assert c.min() >= 1 and int(c.sum()) <= 1 << 30
        order = np.argsort(full, kind="stable")
        assert (np.diff(c[order]) >= 0).all()                                              # the shift keeps the order of the counts
        shift = next(s for s in range(64) if sum(max(1, int(v) >> s) for v in full) <= 1 << 30)
        assert c.tolist() == [max(1, int(v) >> shift) for v in full]
    assert tables_from_histograms(h, counts=False).num_aux_var_counts is None and tables_from_histograms(h, index=False).index_counts is None


def test_fitted_tables_make_every_file_strictly_smaller_where_they_must():
    """K = 8 in every block, layout (8, (8,)): a count costs log2(1011 / 101) = 3.3 bits under the default model (9 values of weight 101 and
    the terminator) and, under the table fitted to these rows -- c = [8, 1 x 8, 65, 1] of total 82 --, log2(82 / 65) = 0.34 bits."""
    from irec.io import hist_rows, tables_from_histograms, utils as U
    rng = np.random.default_rng(3)
    K = np.full((8, 8), 8, dtype=np.int32)
    idx = rng.integers(0, 20, (8, 8, C.MAX_K)).astype(np.int32)
    t = tables_from_histograms(hist_rows(K, idx, (8,), 20, C.MAX_K + 1), index=False)
    assert t.num_aux_var_counts[0].tolist() == [8] + [1] * 8 + [65] + [1]
    assert math.log2(1011 / 101) > 3.3 and math.log2(81 + 1) - math.log2(65) < 1
    plain, off_p = U.encode_files_ragged(C.SEED, C.SHAPE, C.BLOCK_SIZE, K, idx, 20, (8,))
    fitted, off_f = U.encode_files_ragged(C.SEED, C.SHAPE, C.BLOCK_SIZE, K, idx, 20, (8,), tables=t)
    print("bytes per file, default model:", np.diff(off_p).tolist(), "fitted count table:", np.diff(off_f).tolist())
    assert (np.diff(off_f) < np.diff(off_p)).all()
    _, K2, idx2 = U.decode_files_ragged(fitted, off_f, (8,), C.MAX_K, tables=t)
    assert np.array_equal(K2, K) and np.array_equal(idx2[..., :8], idx[..., :8])


def test_golden_files_of_the_real_reference():
    """tests/golden/rec_tables_files.npz (make_golden_rec_tables.py): the file the reference's writer made with index_counts_file is,
    byte for byte, what the batched writer and the core make of the same rows and table; the file of ours under both kinds of table, which
    the reference's reader read back to these rows when the fixture was made, is still what the writer gives.  (The reference cannot
    write a file with count tables at all: the fixture's note.)"""
    from conftest import GOLDEN_DIR
    from irec.io import SymbolTables, utils as U
    g = np.load(os.path.join(GOLDEN_DIR, "rec_tables_files.npz"))
    K, idx, bpr, S = g["K"], g["idx"], tuple(int(b) for b in g["bpr"]), int(g["max_index"])
    seed, bs, *shape = (int(v) for v in g["meta"])
    cuts = np.concatenate([[0], np.cumsum(g["count_lengths"])])
    both = SymbolTables(g["index_counts"], [g["count_counts"][cuts[r]:cuts[r + 1]] for r in range(len(bpr))])
    index_only = SymbolTables(g["index_counts"], None)
    assert "cannot write" in str(g["note"]) and K.min() >= 1
    for tables, want in ((index_only, g["ref_index_bytes"]), (both, g["ours_both_bytes"])):
        blob, off = U.encode_files_ragged(seed, tuple(shape), bs, K, idx, S, bpr, tables=tables)
        assert blob.tobytes() == want.tobytes()
        out, _, status = C.core_encode(K, idx, S, bpr, C.raw_tables(tables), want.size)
        assert status[0] == 0 and out[:want.size].tobytes() == want.tobytes()
        hdr, K2, idx2 = U.decode_files_ragged(want, np.array([0, want.size]), bpr, C.MAX_K, tables=tables)
        assert np.array_equal(K2, K) and np.array_equal(idx2, np.where(np.arange(C.MAX_K)[None, None, :] < K[..., None], idx, 0))
