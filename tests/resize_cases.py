"""Shared cases of the resize tests (tests/test_resize_host.py, tests/test_resize_gpu.py): the shapes, the seeded inputs, a restatement
of the definition in numpy.float32 (every operation an IEEE float32 operation, in the order DESIGN.md §3 "resize" writes them), the
float64 referee, and the bound between the two.  A helper, no tests in it."""
import functools

import numpy as np

# (name, in_h, in_w, out_h, out_w): the smallest shapes at which the kernel can go wrong (a tile is 16 rows x 64 row elements)
SHAPES = [
    ("both_axes", 65, 67, 64, 64),
    ("one_axis_identity", 127, 64, 64, 64),
    ("identity", 64, 64, 64, 64),
    ("ragged_tiles", 130, 201, 128, 192),       # source rows span more than one tile, ragged last tile in NHWC (576 = 9 x 64) and rows
    ("shrink_by_1_5", 191, 129, 128, 128),
]
BATCHES = (1, 3)
LAYOUTS = ("nchw", "nhwc")
FAMILIES = ("centred", "unit", "uint8")          # float32 in [-0.5, 0.5], float32 in [0, 1], uint8
C = 3
CASES = [(s[0], n, layout, family) for s in SHAPES for n in BATCHES for layout in LAYOUTS for family in FAMILIES]
SIZES = {s[0]: s[1:] for s in SHAPES}

U = 2.0 ** -24                                   # the unit round-off of float32


def bound(magnitude=1.0):
    """The absolute bound between the float32 path and a referee that does the pixel arithmetic exactly (float64) under the SAME
    float32 coordinates -- lo, hi and t are float32 numbers by definition, so they are the referee's too.  For taps of magnitude at
    most M, to first order in U:
      top = tl + (tr - tl) * tx:  the difference rounds once (<= 2 M U), the product carries that and rounds once (<= 2 M U more),
                                  the sum rounds once (<= M U, the result lying between the taps)           -> 5 M U; the same for bot
      out = top + (bot - top) * ty:  carries (1 - ty) e_top + ty e_bot <= 5 M U, and its own three roundings <= 5 M U     -> 10 M U
    A referee that shares no code (torch's interpolate: the same float32 coordinates, weights w and 1 - w, a sum of four products)
    has its own roundings, one for 1 - w per axis, four products, three sums, which the same count bounds by 10 M U.  So two
    float32 evaluations differ by at most 20 M U, and one float32 evaluation from the exact value by half of that; the tests use
    20 M U = 1.2e-6 M for both.  The uint8 conversion u / 255 is one more float32 operation of the definition: the referee starts from
    the converted float32 taps."""
    return 20.0 * magnitude * U


@functools.lru_cache(maxsize=None)
def fixture(shape_name, n, layout, family):
    in_h, in_w, _, _ = SIZES[shape_name]
    rng = np.random.default_rng([SHAPES.index(next(s for s in SHAPES if s[0] == shape_name)), n, FAMILIES.index(family)])
    shape = (n, C, in_h, in_w)
    if family == "uint8":
        x = rng.integers(0, 256, size=shape, dtype=np.uint8)
    else:
        x = rng.random(size=shape, dtype=np.float32) - (np.float32(0.5) if family == "centred" else np.float32(0.0))
    x = np.ascontiguousarray(x if layout == "nchw" else x.transpose(0, 2, 3, 1))
    x.setflags(write=False)
    return x


def as_float(x):
    """The taps as the definition sees them: float32, a uint8 source as float32(u) / float32(255)."""
    return x.astype(np.float32) / np.float32(255.0) if x.dtype == np.uint8 else x


def axis(n_in, n_out):
    """(lo, hi, t) of every output position of an axis, in float32 operations; an axis of equal sizes is not interpolated (t None)."""
    o = np.arange(n_out)
    if n_in == n_out:
        return o, o, None
    scale = np.float32(n_in) / np.float32(n_out)
    s = (o.astype(np.float32) + np.float32(0.5)) * scale - np.float32(0.5)
    assert s.dtype == np.float32
    fl = np.floor(s)
    lo = np.minimum(np.maximum(fl.astype(np.int64), 0), n_in - 1)
    hi = np.minimum(np.ceil(s).astype(np.int64), n_in - 1)
    return lo, hi, s - fl


def _lerp(a, b, t):
    return a if t is None else a + (b - a) * t


def resize(x, out_h, out_w, layout, dtype=np.float32):
    """The definition over x [N, C, H, W] / [N, H, W, C]: dtype float32 is the restatement (the twin's bits), float64 the referee (the
    float32 coordinates, the pixel arithmetic exact to double rounding)."""
    v = as_float(x)
    v = (v if layout == "nchw" else v.transpose(0, 3, 1, 2)).astype(dtype)
    ylo, yhi, ty = axis(v.shape[2], out_h)
    xlo, xhi, tx = axis(v.shape[3], out_w)
    tx = None if tx is None else tx.astype(dtype)[None, None, None, :]
    ty = None if ty is None else ty.astype(dtype)[None, None, :, None]
    with np.errstate(invalid="ignore"):
        top = _lerp(v[:, :, ylo][:, :, :, xlo], v[:, :, ylo][:, :, :, xhi], tx)
        bot = _lerp(v[:, :, yhi][:, :, :, xlo], v[:, :, yhi][:, :, :, xhi], tx)
        out = _lerp(top, bot, ty)
    assert out.dtype == dtype
    return np.ascontiguousarray(out if layout == "nchw" else out.transpose(0, 2, 3, 1))


def taps_mask(bad, out_h, out_w):
    """For bad [H, W] bool (where a plane holds a non-finite value): [out_h, out_w] bool, the outputs that have one among their taps
    (an axis that is not interpolated has one tap)."""
    ylo, yhi, _ = axis(bad.shape[0], out_h)
    xlo, xhi, _ = axis(bad.shape[1], out_w)
    return bad[ylo][:, xlo] | bad[ylo][:, xhi] | bad[yhi][:, xlo] | bad[yhi][:, xhi]


def non_finite_fixture(shape_name="both_axes"):
    """One [1, 3, H, W] float32 image holding a NaN and an infinity, away from each other and from the borders."""
    in_h, in_w, _, _ = SIZES[shape_name]
    x = np.array(fixture(shape_name, 1, "nchw", "unit"))
    x[0, 0, 20, 30] = np.nan
    x[0, 1, 40, 11] = np.inf
    return x
