"""The .res container on the device (irec_res_encode_files_device / irec_res_decode_files_device: csrc/irec_res.hip) against its host
twin over the same core: the same bytes, offsets, pixels and statuses on every case of tests/residual_cases.py, lanes that cross
workgroups, a short and an exactly-sized output, and the damage cases of tests/test_residual_host.py."""
import numpy as np
import pytest
import torch

import residual_cases as RC
import test_residual_host as H

pytestmark = pytest.mark.gpu

CASES = RC.make_cases()


@pytest.fixture(scope="module")
def res(engine):
    from irec.io import residual
    return residual


@pytest.fixture(scope="module")
def host_files(res):
    return {name: res.encode_residuals(p, l, s, stream_len=L) for name, (p, l, s, L) in CASES.items()}


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _decode(res, blob, off, loc, scale, L):
    out, status = res.decode_residuals_device(*_dev(blob), off, *_dev(loc), scale, stream_len=L, strict=False)
    return out.cpu().numpy(), status


@pytest.mark.parametrize("name", list(CASES))
def test_device_equals_the_host_twin(res, host_files, name):
    pixels, loc, scale, L = CASES[name]
    want_blob, want_off = host_files[name]
    blob, off = res.encode_residuals_device(*_dev(pixels, loc), scale, stream_len=L)
    assert np.array_equal(off.cpu().numpy(), want_off)
    assert np.array_equal(blob.cpu().numpy(), want_blob)
    out = res.decode_residuals_device(*_dev(want_blob), want_off, *_dev(loc), scale)          # stream_len from the header
    assert out.dtype == torch.uint8 and np.array_equal(out.cpu().numpy(), pixels)


def test_lanes_cross_workgroups_and_the_last_one_is_partial(res):
    """6 images of 8 x 8 x 3 at stream_len 4: 48 streams each, 288 lanes, a workgroup of 256 and one of 32."""
    rng = np.random.default_rng(5)
    pixels, loc = RC._near(rng, (6, 3, 8, 8), 4)
    want_blob, want_off = res.encode_residuals(pixels, loc, 2.0 ** -6, stream_len=4)
    blob, off = res.encode_residuals_device(*_dev(pixels, loc), 2.0 ** -6, stream_len=4)
    assert np.array_equal(off.cpu().numpy(), want_off) and np.array_equal(blob.cpu().numpy(), want_blob)
    out, status = res.decode_residuals_device(blob, off, *_dev(loc), 2.0 ** -6, stream_len=4, strict=False)
    assert not status.any() and np.array_equal(out.cpu().numpy(), pixels)
    # offsets that stay on the device (the model path's launch form)
    out2, status2 = res._decode_residuals_device_launch(blob, off, *_dev(loc), 2.0 ** -6, 4, on_device=True)
    assert not status2.cpu().numpy().any() and torch.equal(out2, out)


def test_short_and_exact_out(res, host_files):
    pixels, loc, scale, L = CASES["near_uniform"]
    want_blob, want_off = host_files["near_uniform"]
    total = int(want_off[-1])
    dp, dl = _dev(pixels, loc)
    short = torch.full((total - 1,), 0xAB, dtype=torch.uint8, device="cuda")
    offsets, status, _ = res._encode_residuals_device_launch(dp, dl, scale, L, short)
    assert np.array_equal(offsets.cpu().numpy(), want_off) and not status.cpu().numpy().any()      # the true size is reported
    assert (short == 0xAB).all()                                                                   # and nothing was written
    blob, off = res.encode_residuals_device(dp, dl, scale, stream_len=L, out=short)                # the public call runs again
    assert np.array_equal(blob.cpu().numpy(), want_blob) and np.array_equal(off.cpu().numpy(), want_off)
    guarded = torch.full((total + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    offsets, status, _ = res._encode_residuals_device_launch(dp, dl, scale, L, guarded[:total])
    assert np.array_equal(guarded[:total].cpu().numpy(), want_blob) and (guarded[total:] == 0xAB).all()


def test_encode_statuses(res):
    pixels, loc, _, L = CASES["ragged_2x2_L5"]
    with pytest.raises(ValueError, match=r"likelihood scale.*\(image 0\)"):
        res.encode_residuals_device(*_dev(pixels, loc), 0.0, stream_len=L)
    bad = loc.copy()
    bad[1, 2, 1, 1] = np.inf
    with pytest.raises(ValueError, match=r"not finite \(image 1\)"):
        res.encode_residuals_device(*_dev(pixels, bad), 0.05, stream_len=L)


def test_damaged_headers(res, host_files):
    pixels, loc, scale, L = CASES["near_uniform"]
    blob, off = host_files["near_uniform"]
    for field, _, _, want in H.HEADER_FIELDS:
        bad = H.damaged_header(blob, off, 1, field)
        out, status = _decode(res, bad, off, loc, scale, L)
        assert status.tolist() == [0, want] == res.decode_residuals(bad, off, loc, scale, stream_len=L, strict=False)[1].tolist(), field
        assert np.array_equal(out[0], pixels[0]) and not out[1].any()
    with pytest.raises(ValueError, match=r"\(image 1\)"):
        res.decode_residuals_device(*_dev(H.damaged_header(blob, off, 1, "magic")), off, *_dev(loc), scale, stream_len=L)


def test_every_truncation_in_one_call(res, host_files):
    """Image k of the call is the first k bytes of the file, the files' own bytes following each cut in the blob."""
    pixels, loc, scale, L = CASES["ragged_2x2_L5"]
    blob, off = host_files["ragged_2x2_L5"]
    one = blob[:off[1]]
    n = len(one)
    cuts = np.concatenate([one[:k] for k in range(n)] + [one])
    offs = np.concatenate([[0], np.cumsum(np.arange(n))]).astype(np.int64)
    locs = np.repeat(loc[:1], n, axis=0)
    out, status = _decode(res, cuts, offs, locs, scale, L)
    want = res.decode_residuals(cuts, offs, locs, scale, stream_len=L, strict=False)[1]
    assert np.array_equal(status, want)
    assert set(status[:RC.HEADER + 6].tolist()) == {RC.E_TRUNCATED_HEADER} and set(status[RC.HEADER + 6:].tolist()) == {RC.E_TRUNCATED_STREAMS}
    assert not out.any()


def test_flipped_byte_and_moved_loc(res, host_files):
    pixels, loc, scale, L = CASES[H.FLIP_CASE]
    blob, off = host_files[H.FLIP_CASE]
    bad = H.flipped_stream_byte(blob, off)
    out, status = _decode(res, bad, off, loc, scale, L)
    assert np.array_equal(status, res.decode_residuals(bad, off, loc, scale, stream_len=L, strict=False)[1]) and status[0] == 0 and status[1] != 0
    assert np.array_equal(out[0], pixels[0]) and not out[1].any()
    pixels, loc, scale, L = CASES[H.MOVE_CASE]
    blob, off = host_files[H.MOVE_CASE]
    out, status = _decode(res, blob, off, H.moved_loc(loc), scale, L)
    assert np.array_equal(status, res.decode_residuals(blob, off, H.moved_loc(loc), scale, stream_len=L, strict=False)[1])
    assert status[H.MOVE_IMAGE] in (RC.E_CORRUPT, RC.E_CHECKSUM) and status[1 - H.MOVE_IMAGE] == 0
    assert np.array_equal(out[1 - H.MOVE_IMAGE], pixels[1 - H.MOVE_IMAGE]) and not out[H.MOVE_IMAGE].any()
