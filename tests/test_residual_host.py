"""The .res container through its host entry points (irec_res_encode_files / irec_res_decode_files: csrc/irec_res_core.h in plain
loops) against the restatement of tests/residual_cases.py: the integer counts, the files' bytes, the round trip, a bound on the
files' size, and what every kind of damage is answered with."""
import struct

import numpy as np
import pytest

import residual_cases as RC

CASES = RC.make_cases()
SCALES = [1e-4, 2.0 ** -8, 0.05, 1.0, 100.0]
M_GRID = sorted(set(range(-2048, 2048, 61)) | {-2048, -1, 0, 1, 2047})


@pytest.fixture(scope="module")
def res():
    from irec.io import residual
    return residual


@pytest.fixture(scope="module")
def host_files(res):
    """Every case's files from the host twin, made once."""
    return {name: res.encode_residuals(p, l, s, stream_len=L) for name, (p, l, s, L) in CASES.items()}


@pytest.mark.parametrize("scale", SCALES)
def test_counts_equal_the_referee(res, scale):
    for m in M_GRID:
        C, want = res.model_counts(m, scale).astype(np.int64), RC.ref_counts(m, scale)
        assert np.array_equal(C, want), (m, scale, np.flatnonzero(C != want)[:5])
        assert C[0] == 0 and C[256] == 65536 and (np.diff(C) >= 1).all(), (m, scale)


def test_exp_restatement_is_an_exp():
    x = np.linspace(-700, 700, 28001)
    assert np.allclose(RC.ref_exp(x), np.exp(x), rtol=1e-14, atol=0)


@pytest.mark.parametrize("name", list(CASES))
def test_bytes_equal_the_referee_and_decode(res, host_files, name):
    pixels, loc, scale, L = CASES[name]
    blob, off = host_files[name]
    want_blob, want_off = RC.ref_files(pixels, loc, scale, L)
    assert np.array_equal(off, want_off)
    assert np.array_equal(blob, want_blob)
    assert np.array_equal(res.decode_residuals(blob, off, loc, scale), pixels)               # stream_len from the header
    for threads in (1, 3):
        b2, o2 = res.encode_residuals(pixels, loc, scale, stream_len=L, n_threads=threads)
        assert np.array_equal(b2, blob) and np.array_equal(o2, off)
        assert np.array_equal(res.decode_residuals(blob, off, loc, scale, stream_len=L, n_threads=threads), pixels)


def test_tiny_scale_case_is_what_it_says(res):
    pixels, loc, scale, _ = CASES["tiny_scale_far"]
    bits = res.residual_model_bits(pixels, loc, scale)
    assert bits[0] >= 15.5 * pixels[0].size            # nearly every symbol has a count of 1 or 2: about 16 bits each
    assert np.allclose(bits, RC.ref_model_bits(pixels, loc, scale), rtol=1e-12)


@pytest.mark.parametrize("name", list(CASES))
def test_size_bound(res, host_files, name):
    """file bits <= residual_model_bits + allowance, the allowance from the format alone:
      header                28 bytes;
      per stream            16 bits of length word, 2 bits that end the code, at most 7 bits of padding to a byte;
      per symbol            log2(1 / (1 - 2^-14)) bits.  The coder narrows width to floor(width D / 2^16) - floor(width C / 2^16)
                            >= width n / 2^16 - 1 for a symbol of count n = D - C >= 1; width >= 2^30 on entry, so width n / 2^16 >= 2^14
                            and the new width is at least (width n / 2^16)(1 - 2^-14).  Every bit but the last two of a stream is one
                            doubling of width, width ends at most 2^32 where it began, so the doublings number at most
                            sum_k [-log2(n_k / 2^16) - log2(1 - 2^-14)]."""
    pixels, loc, scale, L = CASES[name]
    blob, off = host_files[name]
    ideal = res.residual_model_bits(pixels, loc, scale)
    _, c, h, w = pixels.shape
    bits = np.diff(off) * 8
    assert (bits <= ideal + RC.size_allowance_bits(c, h, w, L)).all(), (bits, ideal)
    assert (bits >= ideal).all()


def test_encode_statuses(res):
    pixels, loc, _, L = CASES["ragged_2x2_L5"]
    for scale in (0.0, -1.0, float("nan"), float("inf"), 2.0 ** -25, 2.0 ** 25):
        with pytest.raises(ValueError, match=r"likelihood scale.*\(image 0\)"):
            res.encode_residuals(pixels, loc, scale, stream_len=L)
    bad = loc.copy()
    bad[1, 2, 1, 1] = np.nan
    with pytest.raises(ValueError, match=r"not finite \(image 1\)"):
        res.encode_residuals(pixels, bad, 0.05, stream_len=L)
    with pytest.raises(ValueError, match="stream_len"):
        res.encode_residuals(pixels, loc, 0.05, stream_len=4097)


# ---- damage ---------------------------------------------------------------------------------------------------------------------------
def _status(res, blob, off, loc, scale, L):
    return res.decode_residuals(blob, off, loc, scale, stream_len=L, strict=False)


HEADER_FIELDS = [("magic", 0, "<I", RC.E_MAGIC), ("version", 4, "<H", RC.E_MAGIC), ("channels", 6, "<H", RC.E_SHAPE),
                 ("stream_len", 8, "<I", RC.E_SHAPE), ("height", 12, "<I", RC.E_SHAPE), ("width", 16, "<I", RC.E_SHAPE),
                 ("scale", 20, "<I", RC.E_SCALE_WORD), ("checksum", 24, "<I", RC.E_CHECKSUM), ("length", 28, "<H", RC.E_TRUNCATED_STREAMS)]


def damaged_header(blob, off, image, field):
    """The blob with one header field of one image changed (the length word: made longer than the file)."""
    _, at, fmt, _ = next(f for f in HEADER_FIELDS if f[0] == field)
    out = blob.copy()
    at += int(off[image])
    old = struct.unpack_from(fmt, out, at)[0]
    new = 0xFFFF if field == "length" else old + 1
    out[at:at + struct.calcsize(fmt)] = np.frombuffer(struct.pack(fmt, new), dtype=np.uint8)
    return out


@pytest.mark.parametrize("field", [f[0] for f in HEADER_FIELDS])
def test_every_header_field_has_its_status(res, host_files, field):
    pixels, loc, scale, L = CASES["near_uniform"]
    blob, off = host_files["near_uniform"]
    want = next(f for f in HEADER_FIELDS if f[0] == field)[3]
    out, status = _status(res, damaged_header(blob, off, 1, field), off, loc, scale, L)
    assert status.tolist() == [0, want]
    assert np.array_equal(out[0], pixels[0]) and not out[1].any()
    with pytest.raises(ValueError, match=r"\(image 1\)"):
        res.decode_residuals(damaged_header(blob, off, 1, field), off, loc, scale, stream_len=L)


def test_every_truncation_is_refused_without_a_read_past_the_cut(res, host_files):
    """The file's own bytes stay in place behind every cut: a reader that went past the range it was given would find the stream whole
    and answer 0."""
    pixels, loc, scale, L = CASES["ragged_2x2_L5"]
    blob, off = host_files["ragged_2x2_L5"]
    one, n_streams = blob[:off[1]], 3
    for cut in range(len(one)):
        out, status = _status(res, one, np.array([0, cut]), loc[:1], scale, L)
        want = RC.E_TRUNCATED_HEADER if cut < RC.HEADER + 2 * n_streams else RC.E_TRUNCATED_STREAMS
        assert status.tolist() == [want], cut
        assert not out.any()
    # and from the other side: the file in the middle of a buffer of other bytes
    buf = np.concatenate([np.full(64, 0xA5, np.uint8), one, np.full(64, 0xA5, np.uint8)])
    assert np.array_equal(res.decode_residuals(buf, np.array([64, 64 + len(one)]), loc[:1], scale, stream_len=L), pixels[:1])


# (byte, image and pixel below were run through the host twin: each of them gives the nonzero status the test names)
FLIP_CASE, FLIP_IMAGE, FLIP_FROM_END = "near_uniform", 1, 9
MOVE_CASE, MOVE_IMAGE, MOVE_PIXEL = "ragged_2x2_L5", 0, (1, 0, 1)


def flipped_stream_byte(blob, off):
    out = blob.copy()
    out[int(off[FLIP_IMAGE + 1]) - FLIP_FROM_END] ^= 0x10
    return out


def moved_loc(loc):
    out = loc.copy()
    out[(MOVE_IMAGE,) + MOVE_PIXEL] -= np.float32(1.0 / 256.0)
    return out


def test_flipped_stream_byte(res, host_files):
    pixels, loc, scale, L = CASES[FLIP_CASE]
    blob, off = host_files[FLIP_CASE]
    out, status = _status(res, flipped_stream_byte(blob, off), off, loc, scale, L)
    assert status[0] == 0 and status[1] in (RC.E_CORRUPT, RC.E_CHECKSUM)
    assert np.array_equal(out[0], pixels[0]) and not out[1].any()


def test_moved_loc_is_a_status_for_that_image_only(res, host_files):
    pixels, loc, scale, L = CASES[MOVE_CASE]
    blob, off = host_files[MOVE_CASE]
    out, status = _status(res, blob, off, moved_loc(loc), scale, L)
    assert status[MOVE_IMAGE] in (RC.E_CORRUPT, RC.E_CHECKSUM) and status[1 - MOVE_IMAGE] == 0
    assert np.array_equal(out[1 - MOVE_IMAGE], pixels[1 - MOVE_IMAGE]) and not out[MOVE_IMAGE].any()
