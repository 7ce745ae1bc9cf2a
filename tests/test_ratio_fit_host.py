"""The auxiliary-variance ratio fit (GaussianCoder.update_auxiliary_variance_ratios, rec/coding/coder.py:233-410) on the host:
irec_fit_aux_ratios_host -- the twin of the gfx950 kernels of csrc/irec_fit.hip, DESIGN.md §3 "ratio fit" -- against the
independent float64 referee of tests/ratio_fit_referee.py, the method's semantics, and planted mistakes.  Needs no GPU.

Measured: over every case of CASES -- and every other comparison of this file -- the fitted float32 ratios EQUAL the
referee's (largest |delta ratio| = 0): two float64 computations that differ by ~1e-15 and are rounded to float32 once.  The
partition counts, array lengths, average counts and iterations per step are equal too.  RATIO_TOL is eight times the measured
figure, i.e. equality.  The referee's stop margin exceeds 1e-9 on every step of every case (asserted), so no float64 rounding
can move a stop.  det_exp against math.exp on a 200 001-point grid over [-40, 40]: at most 1 ulp (2.3e-16 relative).
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import irec
from irec import _lib
from irec.coding.coder import _Dist, _det_exp
from irec.coding.utils import CodingError
from irec.engine import build_normal_table

import latent_families as LF
import ratio_fit_referee as R

MAX_DELTA_MEASURED = 0.0
RATIO_TOL = 8 * MAX_DELTA_MEASURED
MIN_MARGIN = 1e-9
SEED = 42


def survey_rows(n_rows, D, first=0):
    from oracle import oracle as O
    rows = [O.synthetic_latent(first + i, D) for i in range(n_rows)]
    return tuple(np.ascontiguousarray(np.stack([r[j] for r in rows])) for j in range(4))


def family_rows(family, n_rows, D, omega):
    return LF.stack([LF.block(family, D, seed, omega) for seed in range(n_rows)])


def reference_case_small():
    """rec/coding/tests/test_coder.py:27-28."""
    return (np.array([[5.], [-5.1]], np.float32), np.full((2, 1), 0.01, np.float32), np.zeros((2, 1), np.float32),
            np.ones((2, 1), np.float32))


def reference_case_1000():
    """rec/coding/tests/test_coder.py:46-53."""
    return (np.stack([np.repeat(0.1, 1000), np.repeat(-0.1, 1000)]).astype(np.float32), np.full((2, 1000), 0.9, np.float32),
            np.zeros((2, 1000), np.float32), np.ones((2, 1000), np.float32))


SIZES = ((2, 1), (6, 192), (16, 1000), (3, 1024), (2, 8192))
OMEGAS = (3., 5., 6.)
CASES = {}
# first image id of a case's rows, where the default (0) leaves a stop closer than MIN_MARGIN to the tolerance in the REFEREE
# (survey-2x8192-om3 from image 0: step 45 stops with a margin of 9.1e-10)
FIRST_IMAGE = {(2, 8192, 3.): 2}
for _n, _D in SIZES:
    for _om in OMEGAS:
        CASES[f"survey-{_n}x{_D}-om{_om:g}"] = (lambda n=_n, D=_D, f=FIRST_IMAGE.get((_n, _D, _om), 0): survey_rows(n, D, f), _om)
for _i, _fam in enumerate(f for f in LF.FAMILIES if f != "mixed"):
    _om = OMEGAS[_i % 3]
    CASES[f"{_fam}-6x192-om3"] = (lambda f=_fam: family_rows(f, 6, 192, 3.), 3.)
    CASES[f"{_fam}-16x1000-om{_om:g}"] = (lambda f=_fam, om=_om: family_rows(f, 16, 1000, om), _om)
CASES["mixed-10x192-om3"] = (lambda: LF.stack(LF.mixed(192, 0, 3.)), 3.)
CASES["mixed-10x1000-om6"] = (lambda: LF.stack(LF.mixed(1000, 1, 6.)), 6.)
CASES["reference-2x1-om6"] = (reference_case_small, 6.)
CASES["reference-2x1000-om6"] = (reference_case_1000, 6.)


def dists(stats, device="cpu"):
    mq, sq, mp, sp = (torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in stats)
    return _Dist(mq, sq), _Dist(mp, sp)


def new_coder(omega, **kw):
    return irec.GaussianCoder(kl_per_partition=omega, sampler=None, extrapolate_auxiliary_ratios=False, **kw)


def referee_fit(stats, omega, seed=SEED, ratios=(1.,), counts=(1.,), **kw):
    _, num = R.partition_counts(*stats, omega, kw.get("mistake"))
    M = int(num.max())
    table = build_normal_table(seed, stats[0].shape[0], stats[0].shape[1], M - 1) if M > 1 else None
    return R.fit(*stats, omega, table, ratios, counts, **kw)


def compare(coder, ref, what=""):
    """The comparison of the host twin (or the device path) with the referee; returns the largest |delta ratio|."""
    assert coder.aux_variable_variance_ratios.dtype == np.float32 and coder.average_counts.dtype == np.float32
    assert coder.aux_variable_variance_ratios.shape == ref["ratios"].shape, what
    assert np.array_equal(coder.average_counts, ref["counts"]), what
    assert coder.last_fit_iters == ref["iters"], (what, coder.last_fit_iters, ref["iters"])
    delta = float(np.max(np.abs(coder.aux_variable_variance_ratios.astype(np.float64) - ref["ratios"].astype(np.float64))))
    print(f"{what}: M = {ref['ratios'].size}, iters = {ref['iters']}, max |delta ratio| = {delta:.3e}, "
          f"min stop margin = {min(ref['margin_stop'] + ref['margin_prev'] + [math.inf]):.3e}")
    assert delta <= RATIO_TOL, (what, delta)
    return delta


def check_margins(ref, what=""):
    for j, (a, b) in enumerate(zip(ref["margin_stop"], ref["margin_prev"])):
        assert a > MIN_MARGIN and b > MIN_MARGIN, (what, j, a, b)


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_twin_matches_referee(name):
    make, omega = CASES[name]
    stats = make()
    ref = referee_fit(stats, omega)
    check_margins(ref, name)
    coder = new_coder(omega)
    coder.update_auxiliary_variance_ratios(*dists(stats), seed=SEED)
    assert coder.last_path == "host" and coder._initialized
    compare(coder, ref, name)
    for i in range(ref["ratios"].size):
        assert coder.get_auxiliary_ratio(i) == coder.aux_variable_variance_ratios[i]
    if name.startswith("reference"):        # test_coder.py:29-30, :54-55 call the method twice
        ref2 = referee_fit(stats, omega, ratios=ref["ratios"], counts=ref["counts"])
        check_margins(ref2, name + " (second call)")
        coder.update_auxiliary_variance_ratios(*dists(stats), seed=SEED)
        compare(coder, ref2, name + " (second call)")


def test_partition_counts_are_the_reference_s_floor_not_the_encoder_s_ceil():
    stats = survey_rows(16, 1000)
    kl, num = R.partition_counts(*stats, 3.)
    lib = _lib.load()
    out_kl, out_num = np.empty(16, np.float32), np.empty(16, np.int32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    _lib.check(lib.irec_fit_partitions_host(3., 16, 1000, *(vp(a) for a in stats), vp(out_kl), vp(out_num), 0), "partitions")
    assert np.array_equal(out_num, num)
    assert np.allclose(out_kl, kl, rtol=1e-6)
    assert np.array_equal(out_num, 1 + np.floor(out_kl / np.float32(3.)).astype(np.int32))


def test_second_call_averages_and_starts_from_the_fitted_values():
    stats, omega = survey_rows(16, 1000), 3.
    coder = new_coder(omega)
    coder.update_auxiliary_variance_ratios(*dists(stats))
    first, counts, iters = coder.aux_variable_variance_ratios.copy(), coder.average_counts.copy(), list(coder.last_fit_iters)
    coder.update_auxiliary_variance_ratios(*dists(stats))
    ref = referee_fit(stats, omega, ratios=first, counts=counts)
    check_margins(ref)
    compare(coder, ref, "second call")
    assert np.array_equal(coder.average_counts[1:], 2 * counts[1:]) and coder.average_counts[0] == 1.
    # started at the fitted values: the first branch of coder.py:324-329, so far fewer iterations than the first call took
    assert sum(coder.last_fit_iters) < sum(iters) / 4
    assert np.max(np.abs(coder.aux_variable_variance_ratios - first)) < 2e-3


def test_higher_kl_batch_grows_the_arrays():
    omega = 3.
    low, high = survey_rows(6, 192), survey_rows(4, 1000, first=20)
    coder = new_coder(omega)
    coder.update_auxiliary_variance_ratios(*dists(low))
    n_low = coder.aux_variable_variance_ratios.size
    ref1 = referee_fit(low, omega)
    compare(coder, ref1, "low")
    coder.update_auxiliary_variance_ratios(*dists(high))
    ref2 = referee_fit(high, omega, ratios=ref1["ratios"], counts=ref1["counts"])
    check_margins(ref2)
    compare(coder, ref2, "high")
    n_high = coder.aux_variable_variance_ratios.size
    assert n_high > n_low + 1
    # entries beyond the old length were zero: all but the topmost start from ratios[ratio] (the `ratio < max` branch, :326-327)
    # and have been averaged over the new rows only
    assert np.all(coder.average_counts[n_low:] <= 4) and np.all(coder.average_counts[n_low:] >= 1)
    assert np.all((coder.aux_variable_variance_ratios > 0) & (coder.aux_variable_variance_ratios <= 1))


def test_max_iters_cuts_every_step():
    stats, omega = survey_rows(16, 1000), 3.
    coder = new_coder(omega)
    coder.update_auxiliary_variance_ratios(*dists(stats), max_iters=5)
    ref = referee_fit(stats, omega, max_iters=5)
    compare(coder, ref, "max_iters=5")
    assert coder.last_fit_iters[1:] == [5] * (len(coder.last_fit_iters) - 1) and max(coder.last_fit_iters) == 5
    with pytest.raises(CodingError):
        coder.update_auxiliary_variance_ratios(*dists(stats), max_iters=0)


def test_same_seed_same_bits_other_seed_other_ratios():
    stats, omega = survey_rows(4, 1000, first=20), 3.
    a, b, c = new_coder(omega), new_coder(omega), new_coder(omega)
    a.update_auxiliary_variance_ratios(*dists(stats), seed=7)
    b.update_auxiliary_variance_ratios(*dists(stats), seed=7)
    c.update_auxiliary_variance_ratios(*dists(stats), seed=8)
    assert a.aux_variable_variance_ratios.tobytes() == b.aux_variable_variance_ratios.tobytes()
    assert a.last_fit_iters == b.last_fit_iters
    ra, rc = a.aux_variable_variance_ratios, c.aux_variable_variance_ratios
    assert ra.size == rc.size >= 3
    assert ra[-1] == rc[-1]                      # the first fitted ratio has seen no draw yet
    assert np.all(ra[1:-1] != rc[1:-1])          # every one below it has


def test_extrapolating_coder_is_still_a_noop():
    coder = irec.GaussianCoder(kl_per_partition=3., sampler=None)
    assert coder.update_auxiliary_variance_ratios(*dists(survey_rows(2, 192))) is None
    assert not hasattr(coder, "aux_variable_variance_ratios")
    assert coder.get_auxiliary_ratio(1) == np.power(2., -0.7864636765648174)


def test_zero_rows_and_infinite_kl_raise():
    coder = new_coder(3.)
    empty = tuple(np.zeros((0, 8), np.float32) for _ in range(4))
    with pytest.raises(CodingError):
        coder.update_auxiliary_variance_ratios(*dists(empty))
    blocked = new_coder(3., block_size=100)       # one block per tensor: the only block is the last one, which is left off
    with pytest.raises(CodingError):
        blocked.update_auxiliary_variance_ratios(*dists(survey_rows(2, 64)))
    mq, sq, mp, sp = survey_rows(3, 64)
    sp = sp.copy()
    sp[1, 5] = 0.
    with pytest.raises(CodingError):
        coder.update_auxiliary_variance_ratios(*dists((mq, sq, mp, sp)))
    assert not coder._initialized and coder.aux_variable_variance_ratios.tolist() == [1.]


def test_block_size_rows_are_all_blocks_but_the_last():
    omega, bs = 3., 192
    stats = survey_rows(2, 3 * 192 + 40)                   # two tensors of four blocks each: three full ones and a short one
    coder = new_coder(omega, block_size=bs)
    coder.update_auxiliary_variance_ratios(*dists(tuple(a.reshape(2, 2, -1) for a in stats)), seed=11)
    rows = [[] for _ in range(4)]
    for i in range(2):
        blocks = coder.split(*(torch.from_numpy(a[i:i + 1]) for a in stats), seed=11)
        assert len(blocks[0]) == 4
        for k in range(4):
            rows[k].extend(b.numpy() for b in blocks[k][:-1])
    rows = tuple(np.stack(r) for r in rows)
    assert rows[0].shape == (6, 192)
    ref = referee_fit(rows, omega, seed=11)
    compare(coder, ref, "block_size")
    full = new_coder(omega, block_size=bs)                  # the last block is dropped even when it is full
    full.update_auxiliary_variance_ratios(*dists(survey_rows(1, 2 * 192)), seed=11)
    assert full.average_counts[-1] == 1.


def test_set_ratios_with_counts_then_fit_continues_the_average():
    stats, omega = survey_rows(6, 192), 3.
    first = new_coder(omega)
    first.update_auxiliary_variance_ratios(*dists(stats))
    restored = new_coder(omega)
    restored.set_auxiliary_variance_ratios(first.aux_variable_variance_ratios, average_counts=first.average_counts)
    first.update_auxiliary_variance_ratios(*dists(stats))
    restored.update_auxiliary_variance_ratios(*dists(stats))
    assert restored.aux_variable_variance_ratios.tobytes() == first.aux_variable_variance_ratios.tobytes()
    assert restored.average_counts.tobytes() == first.average_counts.tobytes()
    plain = new_coder(omega)                                # average_counts=None: ones, as before this argument existed
    plain.set_auxiliary_variance_ratios([1., 0.5, 0.3])
    assert plain.average_counts.tolist() == [1., 1., 1.]
    with pytest.raises(CodingError):
        plain.set_auxiliary_variance_ratios([1., 0.5], average_counts=[1.])


def test_beam_search_coder_fits_through_the_inherited_method():
    stats, omega = survey_rows(6, 192), 3.
    beam = irec.BeamSearchCoder(kl_per_partition=omega, n_beams=10, extra_samples=1., extrapolate_auxiliary_ratios=False)
    plain = new_coder(omega)
    beam.update_auxiliary_variance_ratios(*dists(stats))
    plain.update_auxiliary_variance_ratios(*dists(stats))
    assert beam.aux_variable_variance_ratios.tobytes() == plain.aux_variable_variance_ratios.tobytes()
    assert beam._initialized and beam.get_auxiliary_ratio(1) == plain.aux_variable_variance_ratios[1]
    with pytest.raises(CodingError, match="KL divergence higher than auxiliary variables can account for"):
        beam.get_auxiliary_ratio(plain.aux_variable_variance_ratios.size)


# ---- planted mistakes: each one, applied to a copy of the referee, must fail the comparison ------------------------------------
def _two_calls(omega, **kw):
    """A fit, then a second one over other rows: the averaged ratio and the step's own then differ (coder.py:385-390)."""
    a, b = survey_rows(15, 1000), survey_rows(16, 1000, first=100)
    # one more row whose KL is 18 = 6 Omega exactly (one dim shifted by 6 sigma, q == p elsewhere): 1 + floor gives it 7
    # partitions, ceil 6 -- the only kind of row on which the two differ
    edge = [np.zeros((1, 1000), np.float32), np.ones((1, 1000), np.float32), np.zeros((1, 1000), np.float32), np.ones((1, 1000), np.float32)]
    edge[0][0, 0] = 6.
    a = tuple(np.concatenate([x, e]) for x, e in zip(a, edge))
    r1 = referee_fit(a, omega, **kw)
    return a, b, r1, referee_fit(b, omega, ratios=r1["ratios"], counts=r1["counts"], **kw)


@pytest.mark.parametrize("mistake", ["grad_sign", "stop_early", "rho_last", "ceil"])
def test_planted_mistake_fails_the_comparison(mistake):
    omega = 3.
    a, b, _, good = _two_calls(omega)
    _, _, _, bad = _two_calls(omega, mistake=mistake)
    coder = new_coder(omega)
    coder.update_auxiliary_variance_ratios(*dists(a))
    coder.update_auxiliary_variance_ratios(*dists(b))
    compare(coder, good, "sound referee")
    with pytest.raises(AssertionError):
        compare(coder, bad, mistake)


# ---- det_exp ---------------------------------------------------------------------------------------------------------------------
def test_det_exp_against_libm_and_mirror_bit_equal():
    x = np.concatenate([np.linspace(-40., 40., 200001), [0., -0., 1e-300, -708., -708.5, 709., 709.5, 700., -700., np.inf, -np.inf]])
    out = np.empty_like(x)
    _lib.check(_lib.load().irec_test_det_exp(x.ctypes.data_as(ctypes.c_void_p), x.size, out.ctypes.data_as(ctypes.c_void_p)), "det_exp")
    mirror = _det_exp(x)
    assert np.array_equal(out.view(np.uint64), mirror.view(np.uint64))
    grid = slice(0, 200001)
    want = np.array([math.exp(v) for v in x[grid]])
    ulps = np.abs(out[grid] - want) / np.spacing(want)
    print("det_exp: max error", float(ulps.max()), "ulp,", float(np.max(np.abs(out[grid] - want) / want)), "relative")
    assert ulps.max() <= 1.0
    assert out[-2] == np.inf and out[-1] == 0. and out[200001] == 1. and out[200005] == 0. and out[200007] == np.inf
    nan = np.array([np.nan])
    assert np.isnan(_det_exp(nan)[0])


# ---- models ------------------------------------------------------------------------------------------------------------------------
def test_model_update_coders_fits_every_residual_block():
    """resnet_vae.py:795-801 / :497-499 on CPU tensors: a pass over the images, then one fit per residual block from that block's
    posterior and prior (rows: every block of 1000 dims but the last of every image's 8192-dim latent)."""
    from irec.models import BidirectionalResNetVAE
    from irec.models.resnet_vae import ModelError
    torch.manual_seed(0)
    m = BidirectionalResNetVAE(num_res_blocks=2, sampler="beam_search", sampler_args={"n_beams": 20, "extra_samples": 1.2},
                               coder_args={"block_size": 1000, "extrapolate_auxiliary_ratios": False},
                               deterministic_filters=16, stochastic_filters=8, kl_per_partition=3.).eval()
    with pytest.raises(ModelError):
        m.residual_blocks[0].update_coders()
    torch.manual_seed(1)
    images = torch.rand(2, 3, 64, 64) - 0.5
    m.update_coders(images, seed=42, max_iters=50)
    for b in m.residual_blocks:
        c = b.coder
        assert c._initialized and c.last_path == "host" and c.aux_variable_variance_ratios.size >= 2
        assert c.average_counts[1] <= 16 and max(c.last_fit_iters) <= 50
        rows = [[] for _ in range(4)]
        for i in range(2):
            blocks = c.split(*(t[i:i + 1] for t in (b.posterior.loc, b.posterior.scale, b.prior.loc, b.prior.scale)), seed=42)
            for k in range(4):
                rows[k].extend(x.numpy() for x in blocks[k][:-1])
        ref = referee_fit(tuple(np.stack(r) for r in rows), 3., seed=42, max_iters=50)
        compare(c, ref, b.name)
    again = [(b.coder.aux_variable_variance_ratios.copy(), b.coder.average_counts.copy()) for b in m.residual_blocks]
    m.update_coders(images, seed=42, max_iters=50)      # the same pass (seeded posterior draws), averaged into the same table
    for b, (r, c) in zip(m.residual_blocks, again):
        assert np.array_equal(b.coder.average_counts[1:], 2 * c[1:])
        assert np.max(np.abs(b.coder.aux_variable_variance_ratios - r)) < 0.05
