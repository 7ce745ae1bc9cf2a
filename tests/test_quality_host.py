"""CPU tests of the quality metrics: the host twin irec_quality_host and irec.metrics on CPU tensors against the float64 referee of
tests/quality_cases.py, under its tolerance rule (measured against the reference arithmetic, never against the code under test)."""
import ctypes

import numpy as np
import pytest
import torch

import quality_cases as Q


def _quality(a, b, power_factors, **kw):
    from irec import metrics
    psnr, ms, per_scale = metrics.quality(torch.from_numpy(np.array(a)), torch.from_numpy(np.array(b)), power_factors, **kw)
    assert psnr.dtype == torch.float64 and ms.dtype == torch.float64 and per_scale.dtype == torch.float32
    return psnr.numpy(), ms.numpy(), per_scale.numpy()


@pytest.mark.parametrize("shape_name,family", Q.CASES)
def test_host_twin_against_referee(shape_name, family):
    a, b = Q.fixture(shape_name, family)
    y = Q.yardstick(shape_name, family)
    psnr, ms, per_scale = _quality(a, b, y.power_factors, **Q.UNIT)
    who = f"host {shape_name}/{family}"
    y.check("per_scale", per_scale, who)
    y.check("psnr", psnr, who)
    y.check("ms_ssim", ms, who, flat=family == "flat")
    if family == "bad":
        assert (ms == 0.0).all()


def test_psnr_and_ms_ssim_are_quality_columns():
    from irec import metrics
    a, b = (torch.from_numpy(np.array(v)) for v in Q.fixture("two_scales", "noise"))
    psnr, ms, _ = metrics.quality(a, b, (0.5, 0.5), **Q.UNIT)
    assert torch.equal(metrics.psnr(a, b, mul=1.0, clip=False), psnr)
    assert torch.equal(metrics.ms_ssim(a, b, (0.5, 0.5), **Q.UNIT), ms)


@pytest.mark.parametrize("shape_name", ["last_scale_11", "odd_every_scale", "single_11"])
def test_identical_images_are_exactly_one_and_inf(shape_name):
    a, _ = Q.fixture(shape_name, "noise")
    psnr, ms, per_scale = _quality(a, a, Q.SHAPES[shape_name][1], **Q.UNIT)
    assert (ms == 1.0).all() and (per_scale == 1.0).all()
    assert np.isposinf(psnr).all()


def test_pre_transform_with_clip():
    """Images in [-0.2, 1.2] under the reference's convention (mul 255, the reconstruction clipped, the original not; here both, so
    that both branches of the clamp are live on both images): the referee on the clipped pixels."""
    from irec import metrics
    rng = np.random.default_rng(5)
    shape, pf = (2, 3, 45, 52), Q.POWER_FACTORS[:3]
    b = (Q._structured(rng, shape) / 255.0 * 1.4 - 0.2).astype(np.float32)
    a = (b + rng.normal(0, 0.03, size=shape)).astype(np.float32)
    assert a.min() < 0 and a.max() > 1 and b.min() < 0 and b.max() > 1
    for clip in ((True, False), (True, True)):
        kw = {"mul": 255.0, "add": 0.0, "clip": clip, "max_val": 255.0}
        y = Q.Yardstick(Q.transformed(a, 255.0, 0.0, clip[0]).astype(np.float32), Q.transformed(b, 255.0, 0.0, clip[1]).astype(np.float32), pf)
        psnr, ms, per_scale = _quality(a, b, pf, **kw)
        for kind, got in (("psnr", psnr), ("ms_ssim", ms), ("per_scale", per_scale)):
            y.check(kind, got, f"clip {clip}")
    # the defaults are that convention; the helper derives another range's
    assert metrics.transform_for((0., 1.)) == {"mul": 255.0, "add": 0.0, "clip": (True, False), "max_val": 255.0}
    assert metrics.transform_for((-0.5, 0.5)) == {"mul": 255.0, "add": 127.5, "clip": (True, False), "max_val": 255.0}
    got = metrics.quality(torch.from_numpy(a), torch.from_numpy(b), pf)
    want = metrics.quality(torch.from_numpy(a), torch.from_numpy(b), pf, **metrics.transform_for((0., 1.)))
    assert all(torch.equal(g, w) for g, w in zip(got, want))
    shifted = metrics.quality(torch.from_numpy(a - 0.5), torch.from_numpy(b - 0.5), pf, **metrics.transform_for((-0.5, 0.5)))
    y = Q.Yardstick(Q.transformed(a - np.float32(0.5), 255.0, 127.5, True).astype(np.float32),
                    Q.transformed(b - np.float32(0.5), 255.0, 127.5, False).astype(np.float32), pf)
    y.check("ms_ssim", shifted[1].numpy(), "image_range (-0.5, 0.5)")
    y.check("psnr", shifted[0].numpy(), "image_range (-0.5, 0.5)")


def test_thread_counts_give_the_same_bits():
    a, b = Q.fixture("last_scale_11", "noise")
    one = _quality(a, b, Q.POWER_FACTORS, n_threads=1, **Q.UNIT)
    three = _quality(a, b, Q.POWER_FACTORS, n_threads=3, **Q.UNIT)
    for u, v in zip(one, three):
        assert u.tobytes() == v.tobytes()


def test_nan_stays_in_its_image():
    rng = np.random.default_rng(9)
    b = Q._structured(rng, (3, 3, 45, 45)).astype(np.float32)
    a = (b + rng.normal(0, 4, size=b.shape)).astype(np.float32)
    clean = _quality(a, b, Q.POWER_FACTORS[:3], **Q.UNIT)
    a2 = a.copy()
    a2[1, 2, 17, 30] = np.nan
    dirty = _quality(a2, b, Q.POWER_FACTORS[:3], **Q.UNIT)
    for u, v in zip(clean, dirty):
        assert u[0].tobytes() == v[0].tobytes() and u[2].tobytes() == v[2].tobytes()
    assert not np.isfinite(dirty[0][1]) and not np.isfinite(dirty[1][1])
    # under the clamp too: a NaN is not clamped away
    clipped = _quality(a2 / 255, b / 255, Q.POWER_FACTORS[:3], clip=(True, True))
    assert not np.isfinite(clipped[0][1]) and not np.isfinite(clipped[1][1]) and np.isfinite(clipped[1][[0, 2]]).all()


def test_argument_errors():
    import irec
    from irec import metrics
    lib = irec._lib.load()
    p = irec._lib.IrecQualityParams(255.0, 0.0, 255.0, 0.0, 1, 0, 255.0, 0.01, 0.03)
    a = np.zeros((1, 1, 176, 176), np.float32)
    per_scale, sse = np.zeros((1, 1, 5, 2), np.float32), np.zeros(1, np.float32)

    def host(a_ptr=a.ctypes.data, b_ptr=a.ctypes.data, shape=(1, 1, 176, 176), n_scales=5, params=p, out=per_scale.ctypes.data, sse_ptr=sse.ctypes.data):
        return lib.irec_quality_host(a_ptr, b_ptr, *shape, n_scales, ctypes.byref(params) if params is not None else None, out, sse_ptr, 1)

    assert host() == 0
    for kw, text in (({"a_ptr": None}, b"null pointer"), ({"b_ptr": None}, b"null pointer"), ({"params": None}, b"null pointer"),
                     ({"out": None}, b"null pointer"), ({"sse_ptr": None}, b"null pointer"),
                     ({"n_scales": 0}, b"n_scales must be 1 .. 5"), ({"n_scales": 6}, b"n_scales must be 1 .. 5"),
                     ({"shape": (1, 1, 160, 176)}, b"image too small"), ({"shape": (1, 1, 176, 10), "n_scales": 1}, b"image too small"),
                     ({"params": irec._lib.IrecQualityParams(255.0, 0.0, 255.0, 0.0, 1, 0, 0.0, 0.01, 0.03)}, b"max_val must be positive"),
                     ({"params": irec._lib.IrecQualityParams(255.0, 0.0, 255.0, 0.0, 1, 0, float("nan"), 0.01, 0.03)}, b"max_val must be positive"),
                     ({"shape": (0, 1, 176, 176)}, b"shape out of range")):
        assert host(**kw) == irec._lib.IREC_E_INVALID, kw
        assert b"irec_quality_host" in lib.irec_last_error() and text in lib.irec_last_error(), (kw, lib.irec_last_error())
    # the sizing function: 0 for what the entries refuse
    assert lib.irec_quality_workspace_bytes(1, 1, 176, 176, 5) > 0
    assert lib.irec_quality_workspace_bytes(1, 1, 160, 176, 5) == 0 and lib.irec_quality_workspace_bytes(1, 1, 176, 176, 6) == 0
    # without a GPU the device entry still answers argument errors, and a short workspace, before any launch
    ws = np.zeros(16, np.float64)
    dev = lambda n_scales, ws_bytes: lib.irec_quality_device(a.ctypes.data, a.ctypes.data, 1, 1, 176, 176, n_scales, ctypes.byref(p),  # noqa: E731
                                                             per_scale.ctypes.data, sse.ctypes.data, ws.ctypes.data, ws_bytes, None)
    assert dev(6, 128) == irec._lib.IREC_E_INVALID and b"n_scales must be 1 .. 5" in lib.irec_last_error()
    assert dev(5, 128) == irec._lib.IREC_E_WORKSPACE and b"workspace too small" in lib.irec_last_error()
    # the Python surface: ValueError with the library's text; shapes that do not match
    t = torch.zeros(1, 3, 20, 20)
    with pytest.raises(ValueError, match="image too small"):
        metrics.ms_ssim(t, t, Q.POWER_FACTORS[:2])
    with pytest.raises(ValueError, match="n_scales must be 1 .. 5"):
        metrics.ms_ssim(t, t, ())
    with pytest.raises(ValueError, match="max_val must be positive"):
        metrics.psnr(t, t, max_val=-1.0)
    with pytest.raises(ValueError, match="not one"):
        metrics.psnr(t, t[:, :2])
    assert metrics.min_side(5) == 161 and metrics.min_side(1) == 11
