"""Fixtures and referees of the quality metrics (irec.metrics, include/irec.h: irec_quality_*).  A helper, no tests in it.

`reference(a, b, power_factors, dtype)` restates tf.image.psnr and tf.image.ssim_multiscale of TF 2.1 (filter_size 11, filter_sigma
1.5, k1 0.01, k2 0.03) in numpy with a direct 121-tap filter, on pixels as they are (the transform is the caller's).  In float64 it is
the referee.  In float32 it is the literal restatement of TF's own op order -- uncentred moments, the 2-D kernel from a softmax, every
intermediate in float32 -- whose distance from the referee, e_ref32, is what float32 arithmetic of that form costs on the fixture: the
yardstick of the tolerance rule below.  Nothing here shares code with the product.

The tolerance rule: a value passes if its error against the float64 referee is at most
    max(2 e_ref32, 16 ulp of float32 at max(1, |value|))
with e_ref32 the largest error of the float32 restatement over the fixture's values of the same kind (psnr, ms_ssim, per-scale).  The
factor 2 covers a summation order other than TF's; the floor is what float32 outputs and the five powers, the product and the mean can
cost alone (e_ref32 is exactly 0 on `bad`).  On the `flat` family the final MS-SSIM must also be within e_ref32 / 10: there TF's form
loses 4e-4 to cancellation in F(x^2 + y^2) - (m0^2 + m1^2) at magnitude 1.3e5, and only arithmetic centred at mid-grey gets below a
tenth of that.

Pixels are in [0, 255] units (mul 1, add 0, no clip) so that the `flat` levels are exact in float32."""
import functools

import numpy as np

POWER_FACTORS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
MAX_VAL, K1, K2 = 255.0, 0.01, 0.03
UNIT = {"mul": 1.0, "add": 0.0, "clip": False, "max_val": MAX_VAL}       # the fixtures' transform: pixels as they are

# (shape, power_factors): each the smallest shape that reaches its corner
SHAPES = {
    "last_scale_11": ((2, 3, 176, 176), POWER_FACTORS),                  # the last scale is 11 x 11: one output pixel
    "odd_every_scale": ((1, 3, 177, 191), POWER_FACTORS),                # 177 -> 89 -> 45 -> 23 -> 12: odd at scale 0 and below
    "one_channel_wide": ((1, 1, 183, 370), POWER_FACTORS),
    "straddles_tiles": ((1, 1, 75, 139), POWER_FACTORS[:3]),             # no multiple of any tile size in either direction
    "two_scales": ((2, 3, 32, 32), (0.5, 0.5)),
    "single_11": ((1, 3, 11, 11), POWER_FACTORS[:1]),                    # the smallest image a single scale allows
}
FAMILIES = ("noise", "blur", "flat", "bad")
CASES = [(shape, family) for shape in SHAPES for family in FAMILIES]


def _structured(rng, shape):
    """An image with structure at every scale: two sinusoids, a ramp, and per-pixel texture; float64 in [0, 255]."""
    n, c, h, w = shape
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    out = np.empty(shape)
    for i in range(n):
        for j in range(c):
            fy, fx, ph = rng.uniform(0.02, 0.2), rng.uniform(0.02, 0.2), rng.uniform(0, 6.28)
            out[i, j] = 127.5 + 50 * np.sin(fy * y + fx * x + ph) + 25 * np.sin(0.9 * x - 0.7 * y) + 20 * (x + y) / (h + w) + \
                rng.uniform(-25, 25, size=(h, w))
    return np.clip(out, 0, 255)


def _box_blur(x):
    p = np.pad(x, [(0, 0), (0, 0), (1, 1), (1, 1)], mode="edge")
    h, w = x.shape[2:]
    return sum(p[:, :, i:i + h, j:j + w] for i in range(3) for j in range(3)) / 9.0


@functools.lru_cache(maxsize=None)
def fixture(shape_name, family):
    """(a, b) float32 [N, C, H, W], read-only: reconstruction and original in pixel units."""
    shape, _ = SHAPES[shape_name]
    rng = np.random.default_rng(1000 * list(SHAPES).index(shape_name) + FAMILIES.index(family))
    b = _structured(rng, shape)
    if family == "noise":
        a = b + rng.normal(0.0, 6.0, size=shape)
    elif family == "blur":
        a = _box_blur(b)
    elif family == "flat":
        a = np.full(shape, 250.0)
        a[..., shape[3] // 2:] = 255.0
        a[:, :, shape[2] // 2:, :] = np.where(a[:, :, shape[2] // 2:, :] == 250.0, 255.0, 250.0)     # a 2 x 2 board of the two levels
        b = a - 3.0
    else:
        a = 255.0 - b
    a, b = a.astype(np.float32), b.astype(np.float32)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def _kernel(dtype):
    coords = np.arange(11, dtype=dtype) - dtype(5)
    g = np.square(coords) * dtype(-0.5 / 1.5 ** 2)
    g = (g[None, :] + g[:, None]).reshape(-1)
    e = np.exp(g - g.max())                                              # softmax
    return (e / e.sum(dtype=dtype)).astype(dtype).reshape(11, 11)


def _filter(x, kernel):
    """VALID filtering of [..., H, W] by the 11 x 11 kernel, 121 taps added in row-major order in x's dtype."""
    h, w = x.shape[-2] - 10, x.shape[-1] - 10
    out = np.zeros(x.shape[:-2] + (h, w), dtype=x.dtype)
    for i in range(11):
        for j in range(11):
            out += kernel[i, j] * x[..., i:i + h, j:j + w]
    return out


def _down(x):
    ph, pw = x.shape[-2] % 2, x.shape[-1] % 2
    x = np.pad(x, [(0, 0)] * (x.ndim - 2) + [(0, ph), (0, pw)], mode="symmetric")
    return ((x[..., 0::2, 0::2] + x[..., 0::2, 1::2] + x[..., 1::2, 0::2] + x[..., 1::2, 1::2]) * x.dtype.type(0.25)).astype(x.dtype)


def reference(a, b, power_factors=POWER_FACTORS, dtype=np.float64, max_val=MAX_VAL, k1=K1, k2=K2):
    """(psnr [N], ms_ssim [N], per_scale [N, C, n_scales, 2] -- mean lum cs and mean cs, not clamped) of pixels a against b, every
    operation in `dtype`."""
    t = np.dtype(dtype).type
    x, y = np.asarray(a).astype(dtype), np.asarray(b).astype(dtype)
    mse = np.mean(np.square(x - y), axis=(1, 2, 3), dtype=dtype)
    with np.errstate(divide="ignore"):
        psnr = (t(20.0) * np.log10(t(max_val)) - t(10.0) * np.log10(mse)).astype(dtype)
    kernel = _kernel(t)
    c1, c2 = t((k1 * max_val) ** 2), t((k2 * max_val) ** 2)
    per_scale = np.zeros(x.shape[:2] + (len(power_factors), 2), dtype=dtype)
    for k in range(len(power_factors)):
        if k:
            x, y = _down(x), _down(y)
        m0, m1 = _filter(x, kernel), _filter(y, kernel)
        num0 = m0 * m1 * t(2.0)
        den0 = np.square(m0) + np.square(m1)
        lum = (num0 + c1) / (den0 + c1)
        num1 = _filter(x * y, kernel) * t(2.0)
        den1 = _filter(np.square(x) + np.square(y), kernel)
        cs = (num1 - num0 + c2) / (den1 - den0 + c2)
        per_scale[:, :, k, 0] = np.mean(lum * cs, axis=(2, 3), dtype=dtype)
        per_scale[:, :, k, 1] = np.mean(cs, axis=(2, 3), dtype=dtype)
    terms = np.concatenate([per_scale[:, :, :-1, 1], per_scale[:, :, -1:, 0]], axis=2)
    terms = np.maximum(terms, t(0.0))
    ms = np.mean(np.prod(np.power(terms, np.asarray(power_factors, dtype=dtype)), axis=2, dtype=dtype), axis=1, dtype=dtype)
    return psnr, ms, per_scale


def transformed(v, mul=1.0, add=0.0, clip=False, max_val=MAX_VAL):
    """The pixel transform in float64, for referees of calls that use one."""
    p = np.asarray(v, dtype=np.float64) * mul + add
    return np.clip(p, 0.0, max_val) if clip else p


def ulp32(v):
    return float(np.spacing(np.float32(max(1.0, abs(float(v))))))


class Yardstick:
    """The referee's values of a pair of pixel arrays and the tolerance rule built on them."""

    def __init__(self, a, b, power_factors=POWER_FACTORS):
        self.power_factors = tuple(power_factors)
        self.psnr, self.ms_ssim, self.per_scale = reference(a, b, self.power_factors, np.float64)
        p32, m32, s32 = reference(a, b, self.power_factors, np.float32)
        finite = np.isfinite(self.psnr)
        self.e_ref32 = {"psnr": float(np.max(np.abs(p32[finite].astype(np.float64) - self.psnr[finite]), initial=0.0)),
                        "ms_ssim": float(np.max(np.abs(m32.astype(np.float64) - self.ms_ssim))),
                        "per_scale": float(np.max(np.abs(s32.astype(np.float64) - self.per_scale)))}

    def check(self, kind, got, who="", flat=False):
        """Asserts the rule for every value of `got` (numpy, the shape of the referee's `kind`); prints the figures first."""
        want = getattr(self, kind)
        got = np.asarray(got, dtype=np.float64)
        assert got.shape == want.shape, (kind, got.shape, want.shape)
        e = self.e_ref32[kind]
        worst = 0.0
        for g, w in zip(got.reshape(-1), want.reshape(-1)):
            if not np.isfinite(w):
                assert g == w, f"{who} {kind}: {g} where the referee has {w}"
                continue
            tol = max(2.0 * e, 16.0 * ulp32(w))
            if flat and kind == "ms_ssim":
                tol = min(tol, e / 10.0)
            worst = max(worst, abs(g - w))
            assert abs(g - w) <= tol, f"{who} {kind}: {g!r} against the referee's {w!r}: error {abs(g - w):.3e} > {tol:.3e} (e_ref32 {e:.3e})"
        print(f"{who} {kind}: worst error {worst:.3e}, e_ref32 {e:.3e}")
        return worst


@functools.lru_cache(maxsize=None)
def yardstick(shape_name, family):
    a, b = fixture(shape_name, family)
    y = Yardstick(a, b, SHAPES[shape_name][1])
    if family == "bad":
        assert (y.ms_ssim == 0.0).all(), "the `bad` family is exactly 0 through the clamp"
    return y
