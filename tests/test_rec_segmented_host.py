"""CPU tests of the segmented .rec container (NAME.recs): the host-thread entry points (irec_rec_encode_files_segmented /
irec_rec_decode_files_segmented) and the core's host hooks (irec_rec_test_core_*_segmented: the lane functions of csrc/irec_rec_seg.hip's
kernels over host memory in a plain loop) against the Python restatement of tests/rec_segmented_cases.py, which builds every stream with
one call of an arithmetic coder -- irec_ac_encode, and in the CPU suite the compiled reference's own ArithmeticCoder.  Every comparison
is byte or integer equality."""
import contextlib
import io
import os

import numpy as np
import pytest

import rec_ragged_cases as RC
import rec_segmented_cases as C

from conftest import GOLDEN_DIR

both_suites = [pytest.mark.both_suites, pytest.mark.usefixtures("suite")]

CASES = range(len(C.case_names()))


def _plain_streams(raw, R):
    """(count streams, index streams) of a plain .rec file's bytes."""
    dyn = np.frombuffer(raw[28:28 + 16 * R], dtype="<u4").reshape(4, R)
    cuts = np.concatenate([[28 + 16 * R], 28 + 16 * R + np.cumsum(np.concatenate([dyn[1], dyn[2]]))])
    streams = [raw[int(cuts[k]):int(cuts[k + 1])] for k in range(2 * R)]
    assert int(cuts[-1]) == len(raw)
    return streams[:R], streams[R:]


def _segment_streams(raw, R, n_seg):
    """[(max_part, count stream, index stream)] of a segmented file's bytes, by its directory."""
    d0 = 40 + 4 * R
    entries = np.frombuffer(raw[d0:d0 + 12 * n_seg], dtype="<u4").reshape(n_seg, 3)
    at, out = d0 + 12 * n_seg, []
    for mp, cb, xb in entries.tolist():
        out.append((mp, raw[at:at + cb], raw[at + cb:at + cb + xb]))
        at += cb + xb
    assert at == len(raw)
    return out


@pytest.mark.both_suites
@pytest.mark.usefixtures("suite")
@pytest.mark.parametrize("which", CASES, ids=C.case_names())
def test_files_equal_the_restatement_and_decode_to_the_rows(which):
    from irec.io import segmented as SG
    from irec.io import utils as U
    h, w, ch = C.SHAPE
    for g in C.SEGMENT_BLOCKS:
        c = C.case(which, g)
        K, idx, bpr, S, mk = c["K"], c["idx"], c["bpr"], c["max_index"], c["idx"].shape[2]
        n, total = K.shape[0], int(c["offsets"][-1])
        for threads in (1, 16):
            blob, off = SG.encode_files_segmented(C.SEED, C.SHAPE, C.BLOCK_SIZE, K, idx, S, bpr, g, n_threads=threads)
            assert np.array_equal(off, c["offsets"]) and np.array_equal(blob, c["blob"]), (g, threads)
        for strided in (False, True):
            out, off, status = C.core_encode(K, idx, S, bpr, g, strided=strided)
            assert (status == 0).all() and np.array_equal(off, c["offsets"]), (g, strided)
            assert np.array_equal(out[:total], c["blob"]) and (out[total:] == 0xAB).all()   # the expected bytes, and not one byte more
        out, off, status = C.core_encode(K, idx, S, bpr, g, cap=total)                     # exact capacity
        assert np.array_equal(out[:total], c["blob"]) and (out[total:] == 0xAB).all()
        if n:
            out, off, status = C.core_encode(K, idx, S, bpr, g, cap=total - 1)             # one byte short: the sizes, and nothing written
            assert (out == 0xAB).all() and np.array_equal(off, c["offsets"]) and (status == 0).all()
        else:                                                                              # no images: no bytes, offsets [0]; slots without rows are refused
            assert total == 0 and off.tolist() == [0] and blob.size == 0
            with pytest.raises(ValueError, match="irec_rec_encode_files_segmented: bad arguments"):
                SG.encode_files_segmented(C.SEED, C.SHAPE, C.BLOCK_SIZE, K, np.zeros((0, K.shape[1], 3), np.int32), S, bpr, g)
        want_hdr = np.array([C.SEED, C.BLOCK_SIZE, S, h, w, ch, 0, 0, len(bpr)], dtype=np.uint32)
        hdr, K2, idx2 = SG.decode_files_segmented(c["blob"], c["offsets"], bpr, mk, g)
        assert np.array_equal(K2, K) and np.array_equal(idx2, c["idx_zeroed"]) and (hdr == want_hdr).all()
        hdr, K2, idx2 = SG.decode_files_segmented(c["blob"], c["offsets"], bpr, mk + 3)    # g from the header; a wider max_K adds zero columns
        assert np.array_equal(K2, K) and np.array_equal(idx2[..., :mk], c["idx_zeroed"]) and not idx2[..., mk:].any()
        hdr, K3, idx3, status = C.core_decode(c["blob"], c["offsets"], bpr, g, mk)
        assert (status == 0).all() and np.array_equal(K3, K) and np.array_equal(idx3, c["idx_zeroed"]) and (hdr == want_hdr).all()
        assert all(SG.segment_blocks_of(f[:40]) == g and SG.is_segmented(f) for f in c["files"][:1])
        assert SG.segmented_files_max_K(c["blob"], c["offsets"]) == max([1] + K.reshape(-1).tolist())
        # the plain .rec of the same rows: the same rows come back, and with one segment per residual block the streams are its streams
        plain, poff = U.encode_files_ragged(C.SEED, C.SHAPE, C.BLOCK_SIZE, K, idx, S, bpr)
        _, Kp, idxp = U.decode_files_ragged(plain, poff, bpr, mk)
        assert np.array_equal(Kp, K2[:, :]) and np.array_equal(idxp, c["idx_zeroed"])
        assert not SG.is_segmented(plain[:4])
        if g == 512:
            for i in range(n):
                counts, indices = _plain_streams(plain[poff[i]:poff[i + 1]].tobytes(), len(bpr))
                segs = _segment_streams(c["files"][i], len(bpr), len(bpr))
                assert [s[1] for s in segs] == counts and [s[2] for s in segs] == indices
                first = np.concatenate([[0], np.cumsum(bpr)])
                assert [s[0] for s in segs] == [int(K[i, first[r]:first[r + 1]].max()) for r in range(len(bpr))]


def test_the_cases_hold_what_they_are_to_hold():
    """K = 0 blocks, a segment of only K = 0 blocks (its index stream the terminator alone), K = max_K, a partial last segment."""
    seen = set()
    for which in CASES:
        for g in C.SEGMENT_BLOCKS:
            c = C.case(which, g)
            K, mk = c["K"], c["idx"].shape[2]
            segs = C.segments_of(c["bpr"], g)
            assert (K == mk).any() or K.shape[0] == 0
            seen |= {"zero"} if (K == 0).any() else set()
            seen |= {"partial"} if any(nb < g for r, _, nb in segs if c["bpr"][r] > g) else set()
            for i in range(K.shape[0]):
                for (_r, row, nb), (mp, _cs, xs) in zip(segs, _segment_streams(c["files"][i], len(c["bpr"]), len(segs))):
                    if not K[i, row:row + nb].any():
                        seen.add("zero_segment")
                        assert mp == 0 and xs == C.stream_of([], c["max_index"], 1000)
    assert seen == {"zero", "partial", "zero_segment"}


def test_the_reference_coder_writes_the_same_streams():
    """The restatement once more with the compiled reference's ArithmeticCoder for every stream: the same files.  (Where the reference's
    sources are: the build container.)"""
    from oracle import ref_io
    if not ref_io.available():
        pytest.skip("no reference sources here (GPU box)")
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        ref = ref_io.load()

    def coder(model, message):
        return "".join(ref.ArithmeticCoder(np.asarray(model, dtype=np.int32), precision=32).encode(np.asarray(message, dtype=np.int64)))
    names = C.case_names()
    for name, g in (("1-N1-S20", 1), ("1_4-N3-S36", 2), ("3_1_5-N3-S20", 2), ("3_1_5-N1-S1", 4), ("2_2_2-N3-S36", 1), ("13_302-N1-S36", 16),
                    ("13_302-N1-S20", 512)):
        c = C.case(names.index(name), g)
        for i, raw in enumerate(c["files"]):
            assert C.file_of(c["K"][i], c["idx"][i], c["bpr"], g, c["max_index"], coder=coder) == raw, (name, g, i)


@pytest.mark.both_suites
@pytest.mark.usefixtures("suite")
def test_the_golden_files():
    """tests/golden/rec_segmented_files.npz (tests/golden/make_golden_rec_segmented.py: the restatement's files with the rows that went in)."""
    from irec.io import segmented as SG
    gold = np.load(os.path.join(GOLDEN_DIR, "rec_segmented_files.npz"))
    assert [str(n) for n in gold["names"]] == ["1_4", "3_1_5"]
    for name in gold["names"]:
        bpr, g = tuple(int(b) for b in gold[f"{name}_bpr"]), int(gold[f"{name}_g"])
        seed, block_size, S, h, w, ch = (int(v) for v in gold[f"{name}_meta"])
        K, idx, want, woff = gold[f"{name}_K"], gold[f"{name}_idx"], gold[f"{name}_bytes"], gold[f"{name}_offsets"]
        assert g == 2 and K.shape[0] == 3
        blob, off = SG.encode_files_segmented(seed, (h, w, ch), block_size, K, idx, S, bpr, g)
        assert np.array_equal(off, woff) and np.array_equal(blob, want)
        out, off, status = C.core_encode(K, idx, S, bpr, g, seed=seed, shape=(h, w, ch), block_size=block_size)
        assert (status == 0).all() and np.array_equal(out[:off[-1]], want)
        for i in range(3):
            assert C.file_of(K[i], idx[i], bpr, g, S, seed=seed, shape=(h, w, ch), block_size=block_size) == want[woff[i]:woff[i + 1]].tobytes()
        hdr, K2, idx2 = SG.decode_files_segmented(want, woff, bpr, idx.shape[2])
        assert np.array_equal(K2, K) and np.array_equal(idx2, np.where(np.arange(idx.shape[2]) < K[..., None], idx, 0))


@pytest.mark.both_suites
@pytest.mark.usefixtures("suite")
def test_damaged_files_get_a_status_of_their_own_and_zeroed_rows():
    D = C.damaged_set()
    bpr, g, mk = C.DAMAGED_BPR, C.DAMAGED_G, C.DAMAGED_MAX_K
    names, want, n_named = D["names"], D["want"], D["n_named"]
    hdr, K, idx, st = C.core_decode(D["blob"], D["offsets"], bpr, g, mk)
    hdr_t, K_t, idx_t, st_t = C.host_decode(D["blob"], D["offsets"], bpr, g, mk, n_threads=16)
    assert np.array_equal(st, st_t) and np.array_equal(K, K_t) and np.array_equal(idx, idx_t) and np.array_equal(hdr, hdr_t)
    assert [(n, int(s)) for n, s in zip(names[:n_named], st[:n_named])] == list(zip(names[:n_named], want))
    assert {"valid"} == {n for n, s in zip(names, st) if n == "valid" and s == 0} and all(s == 0 for n, s in zip(names, st) if n == "valid")
    ok = st == 0
    valid = np.array([n == "valid" for n in names])
    assert (K[valid] == D["K0"]).all() and (idx[valid] == D["idx0"]).all()                 # every intact neighbour, whatever stands beside it
    assert not hdr[~ok].any() and not K[~ok].any() and not idx[~ok].any()                   # a refused image: zeroed rows
    assert (st[n_named:-1] != 0).sum() >= 3 * C.N_RANDOM // 4
    reached = set(st.tolist())
    print("statuses:", sorted(reached))
    assert {4, 5, 6, 7, 9, 13, 17, 18, C.E_SEG_MAGIC, C.E_SEG_DIRECTORY, C.E_SEG_BLOCKS} <= reached
    # the call's own g and max_K: another g is every file's IREC_REC_E_SEG_BLOCKS, a max_K one lower refuses the valid file
    one = np.frombuffer(D["data"], dtype=np.uint8)
    off = np.array([0, one.size])
    for other in (1, 2, 16):
        assert C.core_decode(one, off, bpr, other, mk)[3].tolist() == [C.E_SEG_BLOCKS] == C.host_decode(one, off, bpr, other, mk)[3].tolist()
    assert C.core_decode(one, off, bpr, g, mk - 1)[3].tolist() == [18] == C.host_decode(one, off, bpr, g, mk - 1)[3].tolist()
    assert C.core_decode(one, off, (3, 1, 8), g, mk)[3].tolist() == [17] and C.core_decode(one, off, (4, 9), g, mk)[3].tolist() == [17]
    from irec.io import segmented as SG
    with pytest.raises(ValueError, match=r"not the file's length \(image 0\)"):
        SG.decode_files_segmented(one[:-1], np.array([0, one.size - 1]), bpr, mk, g)
    with pytest.raises(ValueError, match=r"segment_blocks.*\(image 0\)"):
        SG.decode_files_segmented(one, off, bpr, mk, 2)


@pytest.mark.both_suites
@pytest.mark.usefixtures("suite")
def test_the_writer_refuses_one_image_alone():
    from irec.io import segmented as SG
    c = C.case(C.case_names().index("3_1_5-N3-S20"), 2)
    bpr, g, files = c["bpr"], 2, c["files"]
    K, idx, mk = np.array(c["K"]), np.array(c["idx"]), c["idx"].shape[2]
    for image in range(3):
        bad, K1 = idx.copy(), K.copy()
        K1[image, 8] = max(K1[image, 8], 1)
        bad[image, 8, 0] = 20                                  # an index equal to max_index, in the last (partial) segment
        want = [C.file_of(K1[i], idx[i], bpr, g, 20) if i != image else b"" for i in range(3)]
        out, off, status = C.core_encode(K1, bad, 20, bpr, g)
        assert status.tolist() == [2 if i == image else 0 for i in range(3)]
        assert [out[off[i]:off[i + 1]].tobytes() for i in range(3)] == want and (out[off[3]:] == 0xAB).all()
        with pytest.raises(ValueError, match=rf"max_index.*\(image {image}\)"):
            SG.encode_files_segmented(C.SEED, C.SHAPE, C.BLOCK_SIZE, K1, bad, 20, bpr, g)
        for k_bad in (mk + 1, -1):
            Kbad = K.copy()
            Kbad[image, 5] = k_bad
            out, off, status = C.core_encode(Kbad, idx, 20, bpr, g)
            assert status.tolist() == [1 if i == image else 0 for i in range(3)]
            assert [out[off[i]:off[i + 1]].tobytes() for i in range(3)] == [f if i != image else b"" for i, f in enumerate(files)]


@pytest.mark.both_suites
@pytest.mark.usefixtures("suite")
def test_the_plain_readers_refuse_a_segmented_blob(tmp_path):
    """Every reader of the plain container, given segmented files: a status or an error, never rows."""
    from irec.io import SymbolTables
    from irec.io import utils as U
    c = C.case(C.case_names().index("1_4-N3-S20"), 2)
    bpr, mk, blob, off = c["bpr"], c["idx"].shape[2], c["blob"], c["offsets"]
    assert C.SHAPE[1] < 65536 and all(raw[26:28] == b"\x00\x00" for raw in c["files"])      # what they take for R
    hdr, K, idx, st = RC.core_decode(blob, off, bpr, mk)
    assert (st != 0).all() and not K.any() and not idx.any() and not hdr.any()
    with pytest.raises(ValueError, match=r"\(image 0\)"):
        U.decode_files_ragged(blob, off, bpr, mk)
    with pytest.raises(ValueError):
        U.decode_files(blob, off, 1, 5, mk)
    tables = SymbolTables(index_counts=np.array([1] + [7] * 20), num_aux_var_counts=[np.array([1] + [3] * (mk + 1))] * len(bpr))
    hdr, K, idx, st = U._decode_files_tables_status(blob, off, bpr, mk, tables)
    assert (st != 0).all() and not K.any() and not idx.any() and not hdr.any()
    path = tmp_path / "one.recs"
    path.write_bytes(c["files"][0])
    with pytest.raises(ValueError):
        U.read_compressed_code(str(path))
    with pytest.raises(ValueError):
        U._native_decode(c["files"][0])
    words = U.rec_header_words(c["files"][0])
    assert words is None or words["R"] == 0
    # and the segmented reader refuses a plain file
    plain, poff = U.encode_files_ragged(C.SEED, C.SHAPE, C.BLOCK_SIZE, c["K"], c["idx"], 20, bpr)
    assert (C.core_decode(plain, poff, bpr, 2, mk)[3] == C.E_SEG_MAGIC).all()


@pytest.mark.both_suites
@pytest.mark.usefixtures("suite")
def test_argument_errors():
    from irec import _lib
    from irec.io import segmented as SG
    lib = _lib.load()
    K, idx = np.ones((2, 5), dtype=np.int32), np.zeros((2, 5, 1), dtype=np.int32)
    for g in (0, -3):
        out, off, status = C.core_encode(K, idx, 36, (4, 1), g, expect=_lib.IREC_E_INVALID)
        assert b"segment_blocks" in lib.irec_last_error()
        assert (out == 0xAB).all() and (off == -1).all() and (status == -1).all()           # outputs untouched
        hdr, K2, idx2, st = C.core_decode(np.zeros(64, np.uint8), np.array([0, 32, 64]), (4, 1), g, 1, expect=_lib.IREC_E_INVALID)
        assert (st == -1).all() and (K2 == -1).all()
        with pytest.raises(ValueError, match="segment_blocks"):
            SG.encode_files_segmented(C.SEED, C.SHAPE, C.BLOCK_SIZE, K, idx, 36, (4, 1), g)
        assert lib.irec_rec_seg_workspace_bytes(2, 2, np.array([4, 1], np.int32).ctypes.data, g) == 0
    C.core_encode(K, idx, 36, (4, 0, 1), 2, expect=_lib.IREC_E_INVALID)
    assert b"below 1" in lib.irec_last_error()
    C.core_encode(np.ones((1, 65), np.int32), np.zeros((1, 65, 1), np.int32), 36, (1,) * 65, 2, expect=_lib.IREC_E_INVALID)
    assert b"IREC_REC_RAGGED_MAX_RES" in lib.irec_last_error()
    big = np.array([2 ** 30], dtype=np.int32)                                               # 2^30 segments of one block: refused before a row is read
    o, s = np.full(2, -1, np.int64), np.full(1, -1, np.int32)
    assert lib.irec_rec_test_core_encode_files_segmented(1, 10, 36, 8, 8, 3, 1, 1, big.ctypes.data, 1, 1, K.ctypes.data, 1, idx.ctypes.data, 1, None, 0,
                                                         o.ctypes.data, s.ctypes.data) == _lib.IREC_E_INVALID
    assert b"2^22" in lib.irec_last_error() and (o == -1).all()
    assert lib.irec_rec_seg_workspace_bytes(1, 1, big.ctypes.data, 1) == 0 and lib.irec_rec_seg_workspace_bytes(1, 1, big.ctypes.data, 512) > 0
    with pytest.raises(ValueError, match=r"not \[N, 5\]"):
        SG.encode_files_segmented(C.SEED, C.SHAPE, C.BLOCK_SIZE, K[:, :4], idx[:, :4], 36, (4, 1), 2)
    assert SG.segment_blocks_of(b"IRSG") is None and SG.segment_blocks_of(b"\x2a" + bytes(60)) is None
    st = _lib.load()
    assert (_lib.IREC_REC_E_SEG_MAGIC, _lib.IREC_REC_E_SEG_DIRECTORY, _lib.IREC_REC_E_SEG_BLOCKS) == (C.E_SEG_MAGIC, C.E_SEG_DIRECTORY, C.E_SEG_BLOCKS)
    text = open(os.path.join(os.path.dirname(__file__), "..", "include", "irec.h")).read()
    assert all(f"IREC_REC_E_SEG_{n} = {v}" in text for n, v in (("MAGIC", 20), ("DIRECTORY", 21), ("BLOCKS", 22))) and "IREC_REC_E_TABLE = 19" in text
