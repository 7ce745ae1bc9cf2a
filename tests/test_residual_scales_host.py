"""One likelihood scale per channel, on the host: the version-2 .res container through irec_res_encode_files_scales /
irec_res_decode_files_scales against the restatement of tests/residual_scales_cases.py, every status of the new entry points, the cost
table, scale_bits against irec_res_symbol_counts and against the float64 model bits, and fit_scales on the host twin."""
import struct

import numpy as np
import pytest

import residual_cases as RC
import residual_scales_cases as SC

CASES = SC.make_cases()


@pytest.fixture(scope="module")
def res():
    from irec.io import residual
    return residual


@pytest.fixture(scope="module")
def host_files(res):
    """Every case's version-2 files from the host twin, made once."""
    return {name: res.encode_residuals(p, l, s, stream_len=L) for name, (p, l, s, L) in CASES.items()}


# ---- the version-2 container ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_bytes_equal_the_restatement_and_decode(res, host_files, name):
    pixels, loc, scales, L = CASES[name]
    blob, off = host_files[name]
    want_blob, want_off = SC.ref_files_v2(pixels, loc, scales, L)
    assert np.array_equal(off, want_off)
    assert np.array_equal(blob, want_blob)
    assert res.version_of(blob) == 2
    assert np.array_equal(res.decode_residuals(blob, off, loc, scales), pixels)               # stream_len from the header
    for threads in (1, 3):
        b2, o2 = res.encode_residuals(pixels, loc, list(scales), stream_len=L, n_threads=threads)
        assert np.array_equal(b2, blob) and np.array_equal(o2, off)
        assert np.array_equal(res.decode_residuals(blob, off, loc, scales, stream_len=L, n_threads=threads), pixels)


@pytest.mark.parametrize("name", list(CASES))
def test_equal_scales_give_version_1_stream_bytes(res, name):
    pixels, loc, _, L = CASES[name]
    c = pixels.shape[1]
    v1 = SC.split(*res.encode_residuals(pixels, loc, 0.05, stream_len=L))
    v2 = SC.split(*res.encode_residuals(pixels, loc, [0.05] * c, stream_len=L))
    for a, b in zip(v1, v2):
        assert b[28 + 4 * (c - 1):] == a[28:]                        # stream length words and streams
        assert b[:4] == a[:4] and b[6:20] == a[6:20] and b[20 + 4 * c:24 + 4 * c] == a[24:28]   # magic, shape, checksum
        assert struct.unpack_from("<H", b, 4) == (2,) and struct.unpack_from("<H", a, 4) == (1,)
        assert b[20:20 + 4 * c] == a[20:24] * c


def test_a_scalar_scale_still_writes_version_1(res):
    pixels, loc, _, L = CASES["cross_3x5x7_L16"]
    blob, off = res.encode_residuals(pixels, loc, 0.05, stream_len=L)
    want_blob, want_off = RC.ref_files(pixels, loc, 0.05, L)
    assert np.array_equal(blob, want_blob) and np.array_equal(off, want_off)
    assert np.array_equal(res.decode_residuals(blob, off, loc, np.float32(0.05)), pixels)


@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan"), float("inf"), 2.0 ** -25, 2.0 ** 25])
def test_a_bad_scale_in_one_channel_is_the_scale_status(res, bad):
    pixels, loc, scales, L = CASES["cross_3x5x7_L16"]
    scales = scales.copy()
    scales[2] = bad
    with pytest.raises(ValueError, match=r"likelihood scale.*\(image 0\)"):
        res.encode_residuals(pixels, loc, scales, stream_len=L)
    # the reader: the words can never agree with a scale that the coder refuses
    blob, off = res.encode_residuals(pixels, loc, CASES["cross_3x5x7_L16"][2], stream_len=L)
    got, status = res.decode_residuals(blob, off, loc, scales, stream_len=L, strict=False)
    assert status.tolist() == [RC.E_SCALE_WORD] * 3 and not got.any()


def test_scale_range_ends_are_coded(res):
    pixels, loc, _, L = CASES["cross_3x5x7_L16"]
    scales = np.array([2.0 ** -24, 1.0, 2.0 ** 24], dtype=np.float32)
    blob, off = res.encode_residuals(pixels, loc, scales, stream_len=L)
    assert np.array_equal(res.decode_residuals(blob, off, loc, scales), pixels)


@pytest.mark.parametrize("name", list(CASES))
def test_damage_is_a_status_per_image(res, host_files, name):
    """Header-level damage of image 1 of N: the reader's status is the restatement's, the image is zero, its neighbours are intact."""
    pixels, loc, scales, L = CASES[name]
    files = SC.split(*host_files[name])
    v1 = SC.split(*res.encode_residuals(pixels, loc, float(scales[0]), stream_len=L))
    seen = set()
    for label, damaged, want in SC.damaged_sets(files, v1, pixels.shape[1:], L, scales):
        blob, off = SC.join(damaged)
        got, status = res.decode_residuals(blob, off, loc, scales, stream_len=L, strict=False)
        assert want != RC.OK, label
        assert status.tolist() == [want if i == 1 else 0 for i in range(len(files))], (label, status)
        assert all(np.array_equal(got[i], pixels[i]) for i in range(len(files)) if i != 1) and not got[1].any(), label
        seen.add(want)
    assert {RC.E_TRUNCATED_HEADER, RC.E_MAGIC, RC.E_SHAPE, RC.E_SCALE_WORD, RC.E_TRUNCATED_STREAMS} <= seen


def test_versions_do_not_read_each_other(res, host_files):
    pixels, loc, scales, L = CASES["cross_3x5x7_L16"]
    files = SC.split(*host_files["cross_3x5x7_L16"])
    v1 = SC.split(*res.encode_residuals(pixels, loc, float(scales[0]), stream_len=L))
    # a version-2 file among version-1 files, read by the version-1 reader
    blob, off = SC.join([v1[0], files[1], v1[2]])
    got, status = res.decode_residuals(blob, off, loc, float(scales[0]), stream_len=L, strict=False)
    assert status.tolist() == [0, RC.E_MAGIC, 0] and np.array_equal(got[0], pixels[0]) and np.array_equal(got[2], pixels[2]) and not got[1].any()
    # a version-1 file among version-2 files, read by the version-2 reader -- also when it is shorter than a version-2 header
    for short in (v1[1], v1[1][:30]):
        blob, off = SC.join([files[0], short, files[2]])
        got, status = res.decode_residuals(blob, off, loc, scales, stream_len=L, strict=False)
        assert status.tolist() == [0, RC.E_MAGIC, 0] and np.array_equal(got[0], pixels[0]) and not got[1].any()


@pytest.mark.parametrize("name", ["cross_3x5x7_L16", "wide_3x80x81_L64"])
def test_another_loc_is_the_checksum_status(res, host_files, name):
    pixels, loc, scales, L = CASES[name]
    blob, off = host_files[name]
    moved = SC.another_loc(loc)
    got, status = res.decode_residuals(blob, off, moved, scales, stream_len=L, strict=False)
    assert status.tolist() == [0, RC.E_CHECKSUM] + [0] * (len(status) - 2), status
    assert np.array_equal(got[0], pixels[0]) and not got[1].any()


def test_wrong_number_of_scales_is_refused(res):
    pixels, loc, scales, L = CASES["cross_3x5x7_L16"]
    with pytest.raises(ValueError, match="3 channels"):
        res.encode_residuals(pixels, loc, scales[:2], stream_len=L)


# ---- the cost table and scale_bits ----------------------------------------------------------------------------------------------------
def test_cost_table(res):
    cost = res.cost_table().astype(np.int64)
    assert cost.shape == (65537,) and cost[0] == 0 and cost[1] == 2 ** 20 and cost[65536] == 0
    for e in range(17):
        assert cost[1 << e] == (16 - e) << 16
    assert (np.diff(cost[1:]) <= 0).all()
    assert np.array_equal(cost, SC.ref_cost_table())


@pytest.fixture(scope="module")
def bits_case():
    pixels, loc, _ = SC.make(SC.BITS_SHAPE[0], SC.BITS_SHAPE[1:], 77)
    return pixels, loc


@pytest.mark.parametrize("n_cand", [1, 2, 64])
def test_scale_bits_equal_the_counts_under_the_table(res, bits_case, n_cand):
    pixels, loc = bits_case
    assert pixels.shape[2] * pixels.shape[3] > SC.TILE and (pixels.shape[2] * pixels.shape[3]) % SC.TILE
    if n_cand == 64:
        pixels, loc = pixels[:1], loc[:1]                            # (the plain loop is 64 x the work)
    scales = SC.candidates(3, n_cand)
    bits, skipped = res.scale_bits(pixels, loc, scales)
    assert skipped == 0 and bits.dtype == np.int64 and bits.shape == (pixels.shape[0], 3, n_cand)
    assert np.array_equal(bits, SC.plain_scale_bits(res, pixels, loc, scales))
    for threads in (1, 5):
        assert np.array_equal(res.scale_bits(pixels, loc, scales, n_threads=threads)[0], bits)


@pytest.mark.parametrize("name", list(CASES))
def test_scale_bits_on_the_container_shapes(res, name):
    pixels, loc, scales, _ = CASES[name]
    cand = np.stack([scales, scales[::-1]], axis=1)
    bits, skipped = res.scale_bits(pixels, loc, cand)
    assert skipped == 0 and np.array_equal(bits, SC.plain_scale_bits(res, pixels, loc, cand))


def test_scale_bits_are_the_model_bits_to_half_a_unit_per_pixel(res, bits_case):
    """cost[n] is (16 - log2 n) 2^16 rounded to an integer: each pixel's share is within 2^-17 bit of the float64 figure."""
    pixels, loc = bits_case
    scales = np.array([0.02, 0.05, 0.11], dtype=np.float32)
    bits, _ = res.scale_bits(pixels, loc, scales.reshape(3, 1))
    ideal = res.residual_model_bits(pixels, loc, scales)
    assert (np.abs(bits.sum(axis=(1, 2)) / 65536.0 - ideal) <= pixels[0].size * 2.0 ** -17).all()
    one = res.scale_bits(pixels, loc, np.float32([0.05]))[0]                                   # [n_cand]: every channel's row
    assert (np.abs(one.sum(axis=(1, 2)) / 65536.0 - res.residual_model_bits(pixels, loc, 0.05)) <= pixels[0].size * 2.0 ** -17).all()


def test_a_loc_that_is_not_finite_is_counted_and_left_out(res, bits_case):
    pixels, loc = bits_case
    scales = SC.candidates(3, 2)
    whole, _ = res.scale_bits(pixels, loc, scales)
    holes = loc.copy()
    at = [(0, 0, 0, 0), (0, 2, 66, 70), (1, 1, 60, 3), (1, 1, 60, 4)]                          # (image 1, channel 1: in the second tile)
    for i, v in zip(at, (np.nan, np.inf, -np.inf, np.nan)):
        holes[i] = v
    bits, skipped = res.scale_bits(pixels, holes, scales)
    assert skipped == 4
    want = whole.copy()
    for i in at:
        px, lc = pixels[i].reshape(1, 1, 1, 1), loc[i].reshape(1, 1, 1, 1)
        want[i[0], i[1]] -= res.scale_bits(px, lc, scales[i[1]].reshape(1, -1))[0][0, 0]
    assert np.array_equal(bits, want)


def test_a_candidate_outside_the_range_is_int64_max(res, bits_case):
    pixels, loc = bits_case
    scales = SC.candidates(3, 4)
    good, _ = res.scale_bits(pixels, loc, scales)
    for bad in (0.0, -0.05, np.nan, np.inf, 2.0 ** -25, 2.0 ** 25):
        s = scales.copy()
        s[1, 2] = bad
        bits, skipped = res.scale_bits(pixels, loc, s)
        want = good.copy()
        want[:, 1, 2] = SC.INT64_MAX
        assert skipped == 0 and np.array_equal(bits, want), bad


def test_rows_do_not_depend_on_the_batch(res, bits_case):
    pixels, loc = bits_case
    scales = SC.candidates(3, 3)
    both, _ = res.scale_bits(pixels, loc, scales)
    for i in range(pixels.shape[0]):
        assert np.array_equal(res.scale_bits(pixels[i:i + 1], loc[i:i + 1], scales)[0][0], both[i])
    swapped, _ = res.scale_bits(pixels[::-1], loc[::-1], scales)
    assert np.array_equal(swapped[::-1], both)


def test_no_images_and_bad_candidate_counts(res):
    bits, skipped = res.scale_bits(np.zeros((0, 3, 4, 4), np.uint8), np.zeros((0, 3, 4, 4), np.float32), np.float32([0.05, 0.1]))
    assert bits.shape == (0, 3, 2) and skipped == 0
    pixels, loc, _, _ = CASES["cross_3x5x7_L16"]
    for n_cand in (0, 65):
        with pytest.raises(ValueError):
            res.scale_bits(pixels, loc, np.full((3, n_cand), 0.05, np.float32))


# ---- fit_scales on the host twin ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def logistic():
    return SC.logistic_images()


@pytest.fixture(scope="module")
def fits(res, logistic):
    pixels, loc = logistic
    batches = [(pixels[:5], loc[:5]), (pixels[5:], loc[5:])]
    return {"single": res.fit_scales(batches, start=0.0), "channels": res.fit_scales(batches, per_channel=True, start=0.0)}


def _bits_at(res, logistic, log_scales):
    pixels, loc = logistic
    scales = np.array([res.scale_from_log(v) for v in np.broadcast_to(log_scales, (3,))], dtype=np.float32).reshape(3, 1)
    return res.scale_bits(pixels, loc, scales)[0].sum(axis=(0, 2))   # per channel


def test_fit_is_the_least_of_everything_evaluated(res, logistic, fits):
    log_scale, bits, ev = fits["single"]
    assert isinstance(log_scale, float) and -9.0 <= log_scale <= 1.0
    assert len(ev["single"]) >= 33 + 1 and 0.0 in dict(ev["single"])                       # `start` was among them
    assert bits == min(b for _, b in ev["single"]) and bits <= dict(ev["single"])[0.0]
    assert log_scale == min(v for v, b in ev["single"] if b == bits)                         # ties: the smaller scale
    assert bits == int(_bits_at(res, logistic, log_scale).sum())                             # and it is what scale_bits says
    log_scales, ch_bits, ev = fits["channels"]
    assert log_scales.shape == (3,) and ch_bits.shape == (3,)
    for ch in range(3):
        assert ch_bits[ch] == min(b for _, b in ev["channels"][ch])
        assert fits["single"][0] in dict(ev["channels"][ch])                                 # the single scale is every channel's candidate
    assert np.array_equal(ch_bits, _bits_at(res, logistic, log_scales))


def test_per_channel_total_is_at_most_the_single_scale_total(fits):
    assert int(fits["channels"][1].sum()) <= fits["single"][1]


def test_last_round_best_is_inside_its_span(fits):
    for name in ("single", "channels"):
        for grid, k in fits[name][2]["last_round"]:
            assert len(grid) == 33
            assert 0 < k < 32 or (k == 0 and grid[0] == -9.0) or (k == 32 and grid[32] == 1.0), (name, k, grid[[0, k, 32]])


def test_recovery_of_the_true_scales(res, logistic, fits):
    """8 images of 3 x 32 x 32 drawn from logistics of scale 0.01 / 0.03 / 0.1: every fitted log-scale within 0.1 of the truth (ten
    times the 0.004 - 0.010 of the optimum's own offset on 8192 pixels per row; sampling error there is about 0.01), and the
    per-channel bits strictly below the single scale's."""
    log_scales, ch_bits, _ = fits["channels"]
    deviation = log_scales - np.log(SC.TRUE_SCALES)
    print("fitted log-scales", log_scales, "deviation from log(true)", deviation, "single", fits["single"][0])
    assert (np.abs(deviation) < 0.1).all(), deviation
    assert int(ch_bits.sum()) < fits["single"][1]
    pixels, loc = logistic
    per_channel = res.residual_model_bits(pixels, loc, [res.scale_from_log(v) for v in log_scales]).sum()
    single = res.residual_model_bits(pixels, loc, res.scale_from_log(fits["single"][0])).sum()
    print("model bits per pixel: per channel", per_channel / pixels.size, "single", single / pixels.size,
          "log_scale 0", res.residual_model_bits(pixels, loc, 1.0).sum() / pixels.size)
    assert per_channel < single
