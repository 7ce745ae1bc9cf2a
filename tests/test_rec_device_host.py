"""CPU tests of the device .rec coder's core (csrc/irec_rec_core.h through the host hooks irec_rec_test_core_encode_files /
irec_rec_test_core_decode_files, which run the lane functions of the kernels over host memory in a plain loop).  The referee is
irec_io.cpp -- irec_rec_encode_files / irec_rec_decode_files, byte-identical to the compiled reference (tests/test_rec_io.py) -- and the
golden .rec files, never the code under test.  Every comparison is byte or integer equality."""
import numpy as np
import pytest

import rec_device_cases as C


@pytest.mark.parametrize("which", range(len(C.case_names())), ids=C.case_names())
def test_core_files_equal_the_host_coder(which):
    c = C.cases()[which]
    K, idx = c["K"], c["idx"]
    n, R, bpt = K.shape
    mk = idx.shape[3]
    total = int(c["offsets"][-1])
    args = (c["seed"], c["shape"], c["block_size"], K, idx, c["max_index"])
    out, off, status = C.core_encode(*args)
    assert (status == 0).all()
    assert np.array_equal(off, c["offsets"])
    assert np.array_equal(out[:total], c["blob"]) and (out[total:] == 0xAB).all()      # the host's bytes, and not one byte more
    if c["golden"]:
        for i, want in enumerate(c["golden"]):
            assert out[off[i]:off[i + 1]].tobytes() == want
    # the strided form (one joined [rows][1 + width] tensor) gives the same bytes
    out_s, off_s, status_s = C.core_encode(*args, strided=True)
    assert (status_s == 0).all() and np.array_equal(off_s, off) and np.array_equal(out_s[:total], c["blob"])
    # one byte short: nothing is written, offsets[N] holds the true size
    out_c, off_c, status_c = C.core_encode(*args, cap=total - 1)
    assert (out_c == 0xAB).all() and int(off_c[-1]) == total and np.array_equal(off_c, off) and (status_c == 0).all()
    # exactly enough
    out_e, off_e, _ = C.core_encode(*args, cap=total)
    assert np.array_equal(out_e[:total], c["blob"]) and (out_e[total:] == 0xAB).all()
    # and back
    hdr, K2, idx2, st = C.core_decode(c["blob"], c["offsets"], R, bpt, mk)
    assert (st == 0).all()
    assert np.array_equal(K2, K) and np.array_equal(idx2, c["idx_zeroed"])
    h, w, ch = c["shape"]
    assert (hdr == np.array([c["seed"], c["block_size"], c["max_index"], h, w, ch, 0, 0, R], dtype=np.uint32)).all()


def test_core_errors_name_the_image():
    from irec.io import utils as U
    K = np.ones((3, 2, 2), dtype=np.int32)
    idx = np.zeros((3, 2, 2, 2), dtype=np.int32)
    bad = idx.copy()
    bad[1, 0, 0, 0] = 36                                      # an index equal to max_index
    out, off, status = C.core_encode(1, (8, 8, 3), 10, K, bad, 36)
    assert status.tolist() == [0, 2, 0] and off[2] == off[1]  # (a file with an error has no bytes)
    with pytest.raises(ValueError, match=r"max_index.*\(image 1\)"):
        U._raise_first_status(status)
    with pytest.raises(ValueError, match=r"\(image 1\)"):      # the host's own words for it
        U.encode_files(1, (8, 8, 3), 10, K, bad, 36)
    Kbad = K.copy()
    Kbad[2, 1, 1] = 3                                         # a K above max_K
    out, off, status = C.core_encode(1, (8, 8, 3), 10, Kbad, idx, 36)
    assert status.tolist() == [0, 0, 1]
    with pytest.raises(ValueError, match=r"K out of range \(image 2\)"):
        U._raise_first_status(status)
    try:
        U.encode_files(1, (8, 8, 3), 10, Kbad, idx, 36)
        raise AssertionError("the host coder accepted K > max_K")
    except ValueError as e:                                   # the same text as the host's
        assert str(e) == "irec_rec_encode_files: K out of range (image 2)"
    # a file of another structure
    blob, off = U.encode_files(1, (8, 8, 3), 10, K, idx, 36)
    hdr, K2, idx2, st = C.core_decode(blob, off, 2, 3, 2)
    assert (st == C.IREC_REC_E_STRUCTURE).all()
    assert not hdr.any() and not K2.any() and not idx2.any()   # zeroed outputs
    with pytest.raises(ValueError, match=r"structure.*\(image 0\)"):
        U._raise_first_status(st)
    # host-checkable argument errors are IREC_E_INVALID
    from irec import _lib
    lib = _lib.load()
    o, s = np.zeros(4, np.int64), np.zeros(3, np.int32)
    assert lib.irec_rec_test_core_encode_files(1, 10, 36, 70000, 8, 3, 3, 2, 2, 2, K.ctypes.data, 1, idx.ctypes.data, 2, None, 0,
                                               o.ctypes.data, s.ctypes.data) == _lib.IREC_E_INVALID


def test_core_reader_agrees_with_the_host_reader_on_damaged_files():
    """Every prefix of a container, 800 copies with one to three bytes replaced, 200 copies with a byte of the seed / block-size / height /
    width / channel fields replaced -- as one blob of 1746 files: the core's status is nonzero exactly when the host reader fails, and
    where both accept, K, idx and the header are equal.  (The host reader here rejects 793 of the 800, accepts all 200 and rejects all
    746 prefixes: both branches are alive.)"""
    D = C.damaged_set()
    R, bpt, mk = C.DAMAGED_SHAPE
    n_prefix = D["n_prefix"]
    ok = D["ok"]
    # what the inputs must be, asserted of the host reader alone
    assert n_prefix == 746 and ok.size == 1746
    assert not ok[:n_prefix].any()
    assert (~ok[n_prefix:n_prefix + 800]).sum() >= 700
    assert ok[n_prefix + 800:].all()
    assert (D["K"][n_prefix + 800:] == D["K0"]).all() and (D["idx"][n_prefix + 800:] == D["idx0"]).all()
    hdr, K, idx, st = C.core_decode(D["blob"], D["offsets"], R, bpt, mk)
    print("host reader rejects", int((~ok[n_prefix:n_prefix + 800]).sum()), "of 800; core", int((st[n_prefix:n_prefix + 800] != 0).sum()))
    assert np.array_equal(st == 0, ok), np.flatnonzero((st == 0) != ok)
    assert np.array_equal(hdr[ok], D["hdr"][ok]) and np.array_equal(K[ok], D["K"][ok]) and np.array_equal(idx[ok], D["idx"][ok])
    assert not hdr[~ok].any() and not K[~ok].any() and not idx[~ok].any()
