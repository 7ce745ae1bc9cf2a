"""CPU tests of the resize: the host twin irec_resize_bilinear_host (through irec.image on CPU tensors) against the numpy.float32
restatement of tests/resize_cases.py bit for bit, against its float64 referee and against torch's interpolate within the bound
derived there, and the entry's refusals."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resize_cases as R


def _twin(x, out_h, out_w, layout, n_threads=0):
    from irec import image
    return image.resize_bilinear(torch.from_numpy(np.array(x)), (out_h, out_w), layout, n_threads=n_threads).numpy()


def _magnitude(x):
    return float(np.abs(R.as_float(x)).max())


@pytest.mark.parametrize("shape_name,n,layout,family", R.CASES)
def test_host_twin_is_the_restatement_bit_for_bit(shape_name, n, layout, family):
    x = R.fixture(shape_name, n, layout, family)
    _, _, out_h, out_w = R.SIZES[shape_name]
    got = _twin(x, out_h, out_w, layout)
    want = R.resize(x, out_h, out_w, layout)
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("shape_name,n,layout,family", R.CASES)
def test_host_twin_against_float64_referee(shape_name, n, layout, family):
    x = R.fixture(shape_name, n, layout, family)
    _, _, out_h, out_w = R.SIZES[shape_name]
    err = np.abs(_twin(x, out_h, out_w, layout).astype(np.float64) - R.resize(x, out_h, out_w, layout, np.float64)).max()
    assert err <= R.bound(_magnitude(x)), (err, R.bound(_magnitude(x)))


@pytest.mark.parametrize("shape_name,n,layout,family", R.CASES)
def test_host_twin_against_torch_interpolate(shape_name, n, layout, family):
    x = R.fixture(shape_name, n, layout, family)
    _, _, out_h, out_w = R.SIZES[shape_name]
    v = torch.from_numpy(np.array(R.as_float(x)))
    v = v if layout == "nchw" else v.permute(0, 3, 1, 2).contiguous()
    want = F.interpolate(v, size=(out_h, out_w), mode="bilinear", align_corners=False, antialias=False)
    want = (want if layout == "nchw" else want.permute(0, 2, 3, 1)).numpy()
    err = np.abs(_twin(x, out_h, out_w, layout).astype(np.float64) - want.astype(np.float64)).max()
    assert err <= R.bound(_magnitude(x)), (err, R.bound(_magnitude(x)))


@pytest.mark.parametrize("layout", R.LAYOUTS)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_identity_sizes_are_a_copy(layout, family):
    x = R.fixture("identity", 3, layout, family)
    assert np.array_equal(_twin(x, 64, 64, layout), R.as_float(x))


def test_identity_keeps_negative_zero_and_non_finite_bits():
    x = np.array(R.fixture("identity", 1, "nchw", "centred"))
    x[0, 0, 0, :3] = [-0.0, np.inf, np.nan]
    assert np.array_equal(_twin(x, 64, 64, "nchw").view(np.uint32), x.view(np.uint32))


def test_result_does_not_depend_on_threads():
    x = R.fixture("ragged_tiles", 3, "nhwc", "unit")
    assert np.array_equal(_twin(x, 128, 192, "nhwc", n_threads=1), _twin(x, 128, 192, "nhwc", n_threads=7))


def test_non_finite_values_reach_their_taps_only():
    x = R.non_finite_fixture()
    _, _, out_h, out_w = R.SIZES["both_axes"]
    got = _twin(x, out_h, out_w, "nchw")
    clean = np.where(np.isfinite(x), x, np.float32(0.25))
    want = R.resize(clean, out_h, out_w, "nchw")
    for ch in range(R.C):
        hit = R.taps_mask(~np.isfinite(x[0, ch]), out_h, out_w)
        assert hit.sum() == 0 if ch == 2 else 1 <= hit.sum() <= 9          # (a shrink by less than 2: at most 3 outputs per axis)
        assert not np.isfinite(got[0, ch][hit]).any()
        assert np.array_equal(got[0, ch][~hit], want[0, ch][~hit])
    assert np.array_equal(got.view(np.uint32), R.resize(x, out_h, out_w, "nchw").view(np.uint32))


# ---- refusals: status, message, output untouched ------------------------------------------------------------------------------------
def _call(src, dtype, n, c, in_h, in_w, out_h, out_w, layout, dst):
    from irec import _lib
    lib = _lib.load()
    st = lib.irec_resize_bilinear_host(src, dtype, n, c, in_h, in_w, out_h, out_w, layout, dst, 1)
    return st, lib.irec_last_error().decode()


REFUSALS = [
    ("n", dict(n=0), "positive"), ("c", dict(c=0), "positive"), ("in_h", dict(in_h=0), "positive"), ("in_w", dict(in_w=-1), "positive"),
    ("out_h", dict(out_h=0), "positive"), ("out_w", dict(out_w=0), "positive"),
    ("grow_h", dict(out_h=9), "only shrinks"), ("grow_w", dict(out_w=9), "only shrinks"),
    ("layout", dict(layout=2), "layout"), ("dtype", dict(dtype=2), "src_dtype"), ("side", dict(in_h=65537), "65536"),
    ("null_src", dict(src=None), "null pointer"), ("null_dst", dict(dst=None), "null pointer"),
]


@pytest.mark.parametrize("name,change,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(name, change, text):
    from irec import _lib
    src = np.zeros((1, 3, 8, 8), dtype=np.float32)
    dst = np.full((1, 3, 8, 8), 7.0, dtype=np.float32)
    args = dict(src=src.ctypes.data, dtype=0, n=1, c=3, in_h=8, in_w=8, out_h=8, out_w=8, layout=0, dst=dst.ctypes.data)
    args.update(change)
    st, message = _call(**args)
    assert st == _lib.IREC_E_INVALID
    assert message.startswith("irec_resize_bilinear_host") and text in message, message
    assert (dst == 7.0).all()


def test_python_entry_refuses_before_the_library():
    from irec import image
    x = torch.zeros(1, 3, 8, 8)
    for bad in (lambda: image.resize_bilinear(x, (9, 8)), lambda: image.resize_bilinear(x, (8, 8), layout="chw"),
                lambda: image.resize_bilinear(x.double(), (8, 8)), lambda: image.resize_bilinear(x[0], (8, 8)),
                lambda: image.resize_bilinear(x, (0, 8))):
        with pytest.raises(ValueError):
            bad()


def test_driver_size():
    from irec import image
    assert image.driver_size(375, 500) == (320, 448)
    assert image.driver_size(512, 768) == (512, 768)
    assert image.driver_size(64, 127) == (64, 64)
    for h, w in ((63, 500), (500, 63), (0, 0)):
        with pytest.raises(ValueError):
            image.driver_size(h, w)
