"""GPU tests of the resize: irec_resize_bilinear_device (through irec.image on CUDA tensors) against the host twin bit for bit on every
case of tests/resize_cases.py, batch independence as bytes, and one run inside the canary arena of tests/guarded.py."""
import numpy as np
import pytest
import torch

import guarded
import resize_cases as R

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("shape_name,n,layout,family", R.CASES)
def test_device_is_the_host_twin_bit_for_bit(shape_name, n, layout, family):
    from irec import image
    x = torch.from_numpy(np.array(R.fixture(shape_name, n, layout, family)))
    size = R.SIZES[shape_name][2:]
    got = image.resize_bilinear(x.cuda(), size, layout)
    want = image.resize_bilinear(x, size, layout)
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == want.shape
    assert np.array_equal(_bits(got), _bits(want))


def test_non_finite_values_on_the_device():
    from irec import image
    x = torch.from_numpy(R.non_finite_fixture())
    size = R.SIZES["both_axes"][2:]
    assert np.array_equal(_bits(image.resize_bilinear(x.cuda(), size)), _bits(image.resize_bilinear(x, size)))


@pytest.mark.parametrize("layout", R.LAYOUTS)
@pytest.mark.parametrize("family", ("centred", "uint8"))
@pytest.mark.parametrize("shape_name", ("ragged_tiles", "identity"))
def test_an_image_of_a_batch_is_that_image_alone(shape_name, layout, family):
    from irec import image
    x = torch.from_numpy(np.array(R.fixture(shape_name, 3, layout, family))).cuda()
    size = R.SIZES[shape_name][2:]
    batch = image.resize_bilinear(x, size, layout)
    for i in range(3):
        alone = image.resize_bilinear(x[i:i + 1], size, layout)
        assert np.array_equal(_bits(batch[i:i + 1]), _bits(alone))


@pytest.mark.parametrize("layout", R.LAYOUTS)
@pytest.mark.parametrize("family", ("unit", "uint8"))
def test_inside_the_canary_arena(layout, family):
    """Outputs pre-filled, inputs compared as bytes afterwards, nothing written outside dst (arrays 4 bytes past a 256-byte boundary)."""
    from irec import _lib, image
    lib = _lib.load()
    x = R.fixture("ragged_tiles", 3, layout, family)
    in_h, in_w, out_h, out_w = R.SIZES["ragged_tiles"]
    out_shape = (3, R.C, out_h, out_w) if layout == "nchw" else (3, out_h, out_w, R.C)
    arena = guarded.Arena(x.nbytes + 4 * int(np.prod(out_shape)) + guarded.slack(2), device="cuda")
    src = arena.put(x, "in", name="src")
    dst = arena.region(torch.float32, out_shape, "out", name="dst")
    arena.arm()
    st = lib.irec_resize_bilinear_device(src.data_ptr(), 1 if family == "uint8" else 0, 3, R.C, in_h, in_w, out_h, out_w, image.LAYOUTS[layout],
                                         dst.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert st == 0, lib.irec_last_error()
    torch.cuda.synchronize()
    arena.check()
    want = image.resize_bilinear(torch.from_numpy(np.array(x)), (out_h, out_w), layout)
    assert np.array_equal(_bits(dst), _bits(want))


def test_a_refused_call_launches_nothing():
    from irec import _lib
    lib = _lib.load()
    arena = guarded.Arena(4 * 3 * 64 * 2 + guarded.slack(2), device="cuda")
    src = arena.put(np.zeros((1, 3, 8, 8), np.float32), "in", name="src")
    dst = arena.region(torch.float32, (1, 3, 8, 8), "out", name="dst")
    arena.arm()
    st = lib.irec_resize_bilinear_device(src.data_ptr(), 0, 1, 3, 8, 8, 9, 8, 0, dst.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert st == _lib.IREC_E_INVALID and b"only shrinks" in lib.irec_last_error()
    torch.cuda.synchronize()
    arena.check()
    assert (dst.view(torch.int32) == guarded._signed(guarded.PREFILL_F32_BITS, 32)).all()
