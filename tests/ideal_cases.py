"""The ideal half of a results row (include/irec.h: irec_posterior_draw_*, irec_loglik_*): the shapes, the inputs, a Python
restatement of the noise and of every per-element term, the two referees, and the raw calls of the host twins that
tests/test_ideal_host.py and tests/test_ideal_gpu.py run.  A helper, no tests in it.

Shapes: `dims` per image at the scalar tail (1, 3, 4, 5), one wave (255, 256, 257), one pass of a workgroup (1023, 1025) and a tile
edge below, at and above, for two tiles and three (4095, 4096, 4097, 8193); one image and three.

The restatement follows csrc/irec_ideal_core.h line by line: Philox4x32-10 in numpy integers, ndtri64 in numpy float64 (IEEE + - * /
sqrt, nothing fused) over the oracle's det_log, det_exp from irec.coding.coder's mirror of the device function.

Referee 1 (the rule of every kl / ll check): the per-element terms by the header's operation sequence, added with math.fsum; a
float64 sum of n terms in ANY order is within n 2^-53 sum |term| of it, and nothing else is allowed.
Referee 2: the same formulas over numpy's own exp / log.  Its distance from the library is a measurement (`python
tests/ideal_cases.py --write` records the largest relative distance over the cases in profiles/ideal/referee.json); the test asserts
four times the recorded value, the margin being for other libm builds."""
import ctypes
import functools
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFEREE_JSON = os.path.join(ROOT, "profiles", "ideal", "referee.json")

TILE = 4096
DIMS = (1, 3, 4, 5, 255, 256, 257, 1023, 1025, 4095, 4096, 4097, 8193)
N_IMAGES = (1, 3)
CASES = [(d, n) for d in DIMS for n in N_IMAGES]
LOGLIK_CASES = [(1, d, n, 1) for d, n in CASES] + [(3, 35, 2, 3), (3, 1366, 1, 3), (3, 2731, 3, 3), (3, 1024, 2, 1)]   # (c, plane, n, n_scales)
SEED, TAG, BASE = 20211021, 7, 5
BINSIZE = 1.0 / 256.0


def case_id(case):
    return "x".join(str(v) for v in case)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def stats(dims, n):
    """(mq, sq, mp, sp), float32 [n, dims], read-only: posteriors that sit a fraction of a prior's width away, scales over a decade."""
    rng = np.random.default_rng([dims, n, 11])
    mp = rng.normal(0.0, 1.0, (n, dims)).astype(np.float32)
    sp = np.exp(rng.normal(0.0, 0.5, (n, dims))).astype(np.float32)
    mq = (mp + sp * rng.normal(0.0, 0.7, (n, dims))).astype(np.float32)
    sq = (sp * np.exp(rng.normal(-0.5, 0.5, (n, dims)))).astype(np.float32)
    return _frozen(mq, sq, mp, sp)


@functools.lru_cache(maxsize=None)
def images(c, plane, n, n_scales):
    """(x, loc, log_scales): x on the 1/256 grid of [-0.5, 0.5) with some values off it, loc within the reference's clip, read-only."""
    rng = np.random.default_rng([c, plane, n, n_scales, 13])
    x = (rng.integers(0, 256, (n, c, plane)) / 256.0 - 0.5 + (rng.random((n, c, plane)) < 0.1) * rng.random((n, c, plane)) / 300.0).astype(np.float32)
    loc = np.clip(x + rng.normal(0.0, 0.03, x.shape), -0.5 + 1.0 / 512.0, 0.5 - 1.0 / 512.0).astype(np.float32)
    log_scales = (-4.0 + rng.random(n_scales)).astype(np.float32)
    return _frozen(x, loc, log_scales)


# ---- the restatement --------------------------------------------------------------------------------------------------------------
def philox_blocks(seed, tag, image, blocks):
    """uint32 [len(blocks), 4]: Philox4x32-10 under the key (seed lo32, seed hi32), counter (block lo32, block hi32, image, tag)."""
    blocks = np.asarray(blocks, dtype=np.uint64)
    s = int(seed) & (2 ** 64 - 1)
    mask = np.uint64(0xFFFFFFFF)
    c0, c1 = blocks & mask, blocks >> np.uint64(32)
    c2, c3 = np.full_like(blocks, int(image)), np.full_like(blocks, int(tag))
    k0, k1 = s & 0xFFFFFFFF, s >> 32
    for _ in range(10):
        a, b = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        n0 = (b >> np.uint64(32)) ^ c1 ^ np.uint64(k0)
        n2 = (a >> np.uint64(32)) ^ c3 ^ np.uint64(k1)
        c1, c3, c0, c2 = b & mask, a & mask, n0, n2
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=1).astype(np.uint32)


def det_log(x):
    """The oracle's det_log over an array."""
    from oracle import oracle as O
    x = np.asarray(x, dtype=np.float64)
    return np.array([O.det_log(float(v)) for v in x.reshape(-1)], dtype=np.float64).reshape(x.shape)


def det_exp(x):
    from irec.coding.coder import _det_exp
    x = np.asarray(x, dtype=np.float64)
    return _det_exp(x).reshape(x.shape)


def _horner(v, coefficients):
    acc = np.full_like(v, coefficients[0])
    for c in coefficients[1:]:
        acc = acc * v + c
    return acc


P0 = (-5.99633501014107895267E1, 9.80010754185999661536E1, -5.66762857469070293439E1, 1.39312609387279679503E1, -1.23916583867381258016E0)
Q0 = (1.0, 1.95448858338141759834E0, 4.67627912898881538453E0, 8.63602421390890590575E1, -2.25462687854119370527E2,
      2.00260212380060660359E2, -8.20372256168333339912E1, 1.59056225126211695515E1, -1.18331621121330003142E0)
P1 = (4.05544892305962419923E0, 3.15251094599893866154E1, 5.71628192246421288162E1, 4.40805073893200834700E1, 1.46849561928858024014E1,
      2.18663306850790267539E0, -1.40256079171354495875E-1, -3.50424626827848203418E-2, -8.57456785154685413611E-4)
Q1 = (1.0, 1.57799883256466749731E1, 4.53907635128879210584E1, 4.13172038254672030440E1, 1.50425385692907503408E1,
      2.50464946208309415979E0, -1.42182922854787788574E-1, -3.80806407691578277194E-2, -9.33259480895457427372E-4)


def ndtri64(u):
    u = np.asarray(u, dtype=np.float64)
    low = u < 0.5
    p = np.where(low, u, 1.0 - u)
    x = np.empty_like(p)
    centre = p > 0.1353352832366127
    w = p[centre] - 0.5
    ww = w * w
    x[centre] = (w + (w * ww) * (_horner(ww, P0) / _horner(ww, Q0))) * 2.5066282746310002
    pt = p[~centre]
    z = np.sqrt(-2.0 * det_log(pt))
    first = z - det_log(z) / z
    rz = 1.0 / z
    x[~centre] = -(first - (_horner(rz, P1) / _horner(rz, Q1)) / z)
    return np.where(low, x, -x)


def eps_ref(seed, tag, image, dims):
    """float32 [dims]: the noise of one image."""
    words = philox_blocks(seed, tag, image, np.arange((dims + 3) // 4)).reshape(-1)[:dims]
    u = ((words >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    return ndtri64(u).astype(np.float32)


def sample_ref(mq, sq, seed, tag, base):
    out = np.empty_like(mq)
    for i in range(mq.shape[0]):
        out[i] = mq[i] + (sq[i] * eps_ref(seed, tag, base + i, mq.shape[1])).astype(np.float32)
    return out


def kl_terms(mq, sq, mp, sp):
    """float64, the shape of the inputs: kl_dim by the header's operation sequence."""
    mq, sq, mp, sp = (np.asarray(a, np.float32).astype(np.float64) for a in (mq, sq, mp, sp))
    with np.errstate(all="ignore"):
        t = sq / sp
        dm = (mq - mp) / sp
        return 0.5 * (dm * dm) + (0.5 * (t * t - 1.0) - det_log(t))


def ll_terms(x, loc, log_scales, binsize=BINSIZE, exp=None, log=None):
    """float64 [n, c, plane]: the likelihood terms by the header's operation sequence (exp / log: another pair, for referee 2)."""
    exp, log = exp or det_exp, log or det_log
    xd, ld = np.asarray(x, np.float32).astype(np.float64), np.asarray(loc, np.float32).astype(np.float64)
    scale = exp(np.asarray(log_scales, np.float32).astype(np.float64))
    scale = np.broadcast_to(scale.reshape(1, -1, 1), xd.shape) if scale.size > 1 else np.full(xd.shape, float(scale[0]))
    step = binsize / scale
    a = (np.floor(xd / binsize) * binsize - ld) / scale
    b = a + step
    v = (1.0 / (1.0 + exp(-b)) - 1.0 / (1.0 + exp(-a))) + 1e-7
    return log(v)


def referee(terms):
    """(sum float64 [n], bound [n]) of terms [n, ...]: math.fsum per image and n 2^-53 sum |term|."""
    flat = np.asarray(terms, np.float64).reshape(terms.shape[0], -1)
    sums = np.array([math.fsum(row.tolist()) for row in flat])
    bounds = np.array([row.size * 2.0 ** -53 * math.fsum(np.abs(row).tolist()) for row in flat])
    return sums, bounds


def kl_libm(mq, sq, mp, sp):
    mq, sq, mp, sp = (np.asarray(a, np.float32).astype(np.float64) for a in (mq, sq, mp, sp))
    t = sq / sp
    dm = (mq - mp) / sp
    terms = 0.5 * (dm * dm) + (0.5 * (t * t - 1.0) - np.log(t))
    return referee(terms)[0]


def ll_libm(x, loc, log_scales, binsize=BINSIZE):
    return referee(ll_terms(x, loc, log_scales, binsize, exp=np.exp, log=np.log))[0]


# ---- the host twins, called raw -----------------------------------------------------------------------------------------------------
def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def placed(array, shift):
    """A contiguous copy of the float32 array whose first byte lies `shift` (0 .. 15) floats past a 64-byte boundary."""
    a = np.ascontiguousarray(array, dtype=np.float32)
    room = np.empty(a.size + 32, dtype=np.float32)
    start = (-(room.ctypes.data // 4)) % 16 + shift
    out = room[start:start + a.size].reshape(a.shape)
    out[...] = a
    assert out.ctypes.data % 64 == shift * 4
    return out


def host_draw(mq, sq, mp, sp, seed=SEED, tag=TAG, base=BASE, n_threads=0, shift=0):
    """(sample float32 [n, dims], kl float64 [n]) of irec_posterior_draw_host; shift: every float32 array that many floats past a
    64-byte boundary (1: no 8- or 16-byte access is aligned)."""
    from irec import _lib
    lib = _lib.load()
    n, dims = mq.shape
    arrays = [placed(a, shift) for a in (mq, sq, mp, sp)]
    sample = placed(np.full((n, dims), np.float32(-7.0)), shift)
    kl = np.full(n, -7.0, dtype=np.float64)
    st = lib.irec_posterior_draw_host(*(_ptr(a) for a in arrays), n, dims, seed, tag, base, _ptr(sample), _ptr(kl), n_threads)
    assert st == 0, lib.irec_last_error()
    return sample.copy(), kl


def host_loglik(x, loc, log_scales, binsize=BINSIZE, n_threads=0, shift=0):
    """ll float64 [n] of irec_loglik_host for x, loc [n, c, plane]."""
    from irec import _lib
    lib = _lib.load()
    n, c, plane = x.shape
    xa, la, sa = placed(x, shift), placed(loc, shift), placed(log_scales, shift)
    ll = np.full(n, -7.0, dtype=np.float64)
    st = lib.irec_loglik_host(_ptr(xa), _ptr(la), _ptr(sa), log_scales.size, n, c, plane, binsize, _ptr(ll), n_threads)
    assert st == 0, lib.irec_last_error()
    return ll


@functools.lru_cache(maxsize=None)
def host_draw_of(dims, n):
    """The host twin's (sample, kl) of a case at (SEED, TAG, BASE): computed once, shared by the tests, read-only."""
    return _frozen(*host_draw(*stats(dims, n)))


@functools.lru_cache(maxsize=None)
def host_loglik_of(case):
    return _frozen(host_loglik(*images(*case)))[0]


# ---- referee 2: the measurement -----------------------------------------------------------------------------------------------------
def measure_libm_distance():
    """The largest relative distance |library - libm referee| / |libm referee| over the cases: {"kl": .., "ll": ..}."""
    worst = {"kl": 0.0, "ll": 0.0}
    for d, n in CASES:
        want = kl_libm(*stats(d, n))
        worst["kl"] = max(worst["kl"], float(np.max(np.abs(host_draw_of(d, n)[1] - want) / np.abs(want))))
    for case in LOGLIK_CASES:
        want = ll_libm(*images(*case))
        worst["ll"] = max(worst["ll"], float(np.max(np.abs(host_loglik_of(case) - want) / np.abs(want))))
    return worst


if __name__ == "__main__":
    for p in (ROOT, os.path.join(ROOT, "relative-entropy-coding_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    measured = measure_libm_distance()
    print(json.dumps(measured))
    if "--write" in sys.argv:
        os.makedirs(os.path.dirname(REFEREE_JSON), exist_ok=True)
        with open(REFEREE_JSON, "w") as fh:
            json.dump({"what": "largest relative distance of the host twins' kl / ll from the float64 referee over numpy's exp / log, over "
                               "the cases of tests/ideal_cases.py", "max_relative_distance": measured,
                       "numpy": np.__version__}, fh, indent=1)
            fh.write("\n")
