"""CPU tests of the ideal half of a results row: the host twins irec_posterior_draw_host / irec_loglik_host (the core that the kernels
run, csrc/irec_ideal_core.h) against the Python restatement and the two referees of tests/ideal_cases.py, the properties
include/irec.h promises of the stream and of the sums, and the arithmetic of the harness's new columns with stub models."""
import json
import types

import numpy as np
import pytest
import torch

import ideal_cases as C
import seed_cases


# ---- the stream -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,n", C.CASES, ids=[C.case_id(c) for c in C.CASES])
def test_eps_and_sample_equal_the_restatement(dims, n):
    mq, sq, mp, sp = C.stats(dims, n)
    sample, _ = C.host_draw_of(dims, n)
    assert sample.tobytes() == C.sample_ref(mq, sq, C.SEED, C.TAG, C.BASE).tobytes()
    eps, _ = C.host_draw(np.zeros_like(mq), np.ones_like(sq), mp, sp)            # 0 + 1 * eps: the noise itself
    want = np.stack([C.eps_ref(C.SEED, C.TAG, C.BASE + i, dims) for i in range(n)])
    assert eps.tobytes() == want.tobytes() and float(np.abs(eps).max()) < 5.5


def test_misaligned_pointers_give_the_same_bits():
    """The five float32 arrays 4 bytes past a 16-byte boundary (no 16-byte access is aligned), at sizes where the aligned call takes
    its 16-byte runs: the same bits."""
    for dims, n in ((4096, 3), (8193, 1), (256, 3)):
        sample, kl = C.host_draw(*C.stats(dims, n), shift=1)
        want = C.host_draw_of(dims, n)
        assert sample.tobytes() == want[0].tobytes() and kl.tobytes() == want[1].tobytes()
    case = (3, 1024, 2, 1)
    assert C.host_loglik(*C.images(*case), shift=1).tobytes() == C.host_loglik_of(case).tobytes()


@pytest.mark.parametrize("dims", [5, 4097])
def test_batch_independence(dims):
    """Image i at base b is a one-image call at base b + i."""
    mq, sq, mp, sp = C.stats(dims, 3)
    sample, kl = C.host_draw_of(dims, 3)
    for i in range(3):
        s1, k1 = C.host_draw(mq[i:i + 1], sq[i:i + 1], mp[i:i + 1], sp[i:i + 1], base=C.BASE + i)
        assert s1.tobytes() == sample[i:i + 1].tobytes() and k1.tobytes() == kl[i:i + 1].tobytes()


def test_other_seeds_tags_and_images_give_other_streams():
    mq, sq, mp, sp = C.stats(257, 1)
    zero, one = np.zeros_like(mq), np.ones_like(sq)
    eps = lambda **kw: C.host_draw(zero, one, mp, sp, **kw)[0]  # noqa: E731
    base = eps()
    assert base.tobytes() == eps().tobytes()
    for other in (eps(seed=C.SEED + 1), eps(tag=C.TAG + 1), eps(base=C.BASE + 1), eps(seed=C.SEED + 2 ** 32)):
        assert (other != base).mean() > 0.99
    assert eps(base=2 ** 32 - 1).shape == base.shape              # the last image number


def test_seed_ladder_accepted_and_pairwise_distinct():
    mq, sq, mp, sp = C.stats(5, 1)
    streams = [C.host_draw(np.zeros_like(mq), np.ones_like(sq), mp, sp, seed=seed)[0].tobytes() for seed in seed_cases.SEEDS]
    assert len(set(streams)) == len(seed_cases.SEEDS)
    for seed in (-2 ** 63, 2 ** 63 - 1):
        C.host_draw(mq, sq, mp, sp, seed=seed)


def test_moments_of_the_noise():
    """2^20 draws of one fixed seed: five-sigma bounds on the mean and the variance of a standard normal, deterministic."""
    n = 2 ** 20
    z = np.zeros((1, n), np.float32)
    eps = C.host_draw(z, z + 1, z, z + 1, seed=1234, tag=0, base=0)[0].astype(np.float64).reshape(-1)
    mean, var = eps.mean(), eps.var()
    print("mean", mean, "var", var, "max |eps|", np.abs(eps).max())
    assert abs(mean) <= 5.0 / np.sqrt(n) and abs(var - 1.0) <= 5.0 * np.sqrt(2.0 / n)
    assert np.abs(eps).max() < 5.5


# ---- the sums ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,n", C.CASES, ids=[C.case_id(c) for c in C.CASES])
def test_kl_against_the_referee(dims, n):
    want, bound = C.referee(C.kl_terms(*C.stats(dims, n)))
    got = C.host_draw_of(dims, n)[1]
    print("kl", got, "referee", want, "bound", bound)
    assert (np.abs(got - want) <= bound).all()


@pytest.mark.parametrize("case", C.LOGLIK_CASES, ids=C.case_id)
def test_ll_against_the_referee(case):
    want, bound = C.referee(C.ll_terms(*C.images(*case)))
    got = C.host_loglik_of(case)
    print("ll", got, "referee", want, "bound", bound)
    assert (np.abs(got - want) <= bound).all()


def test_libm_referee_within_four_times_the_recorded_distance():
    with open(C.REFEREE_JSON) as fh:
        recorded = json.load(fh)["max_relative_distance"]
    measured = C.measure_libm_distance()
    print("measured", measured, "recorded", recorded)
    for kind in ("kl", "ll"):
        assert recorded[kind] > 0.0 and measured[kind] <= 4.0 * recorded[kind]


def test_same_bits_for_any_thread_count():
    mq, sq, mp, sp = C.stats(8193, 3)
    case = (3, 2731, 3, 3)
    want_draw, want_ll = C.host_draw_of(8193, 3), C.host_loglik_of(case)
    for n_threads in (1, 3, 16):
        sample, kl = C.host_draw(mq, sq, mp, sp, n_threads=n_threads)
        assert sample.tobytes() == want_draw[0].tobytes() and kl.tobytes() == want_draw[1].tobytes()
        assert C.host_loglik(*C.images(*case), n_threads=n_threads).tobytes() == want_ll.tobytes()


def test_nan_stays_in_its_image():
    mq, sq, mp, sp = (a.copy() for a in C.stats(4097, 3))
    mp[1, 4096] = np.nan
    sample, kl = C.host_draw(mq, sq, mp, sp)
    want = C.host_draw_of(4097, 3)
    assert np.isnan(kl[1]) and kl[[0, 2]].tobytes() == want[1][[0, 2]].tobytes() and sample.tobytes() == want[0].tobytes()
    x, loc, ls = (a.copy() for a in C.images(3, 2731, 3, 3))
    loc[1, 2, 5] = np.nan
    ll = C.host_loglik(x, loc, ls)
    assert np.isnan(ll[1]) and ll[[0, 2]].tobytes() == C.host_loglik_of((3, 2731, 3, 3))[[0, 2]].tobytes()


def test_argument_errors():
    from irec import _lib
    lib = _lib.load()
    mq, sq, mp, sp = C.stats(5, 1)
    out, kl = np.zeros_like(mq), np.zeros(1)
    p = lambda a: a.ctypes.data  # noqa: E731
    call = lambda *a: lib.irec_posterior_draw_host(*a)  # noqa: E731
    assert call(p(mq), p(sq), p(mp), p(sp), 1, 5, 1, 0, 0, p(out), p(kl), 0) == 0
    for bad in ((None, p(sq), p(mp), p(sp), 1, 5, 1, 0, 0, p(out), p(kl), 0), (p(mq) + 2, p(sq), p(mp), p(sp), 1, 5, 1, 0, 0, p(out), p(kl), 0),
                (p(mq), p(sq), p(mp), p(sp), 0, 5, 1, 0, 0, p(out), p(kl), 0), (p(mq), p(sq), p(mp), p(sp), 1, 0, 1, 0, 0, p(out), p(kl), 0),
                (p(mq), p(sq), p(mp), p(sp), 1, 5, 1, 0, -1, p(out), p(kl), 0), (p(mq), p(sq), p(mp), p(sp), 1, 5, 1, 0, 2 ** 32, p(out), p(kl), 0)):
        assert call(*bad) == _lib.IREC_E_INVALID
    assert lib.irec_ideal_workspace_bytes(3, 8193) == 3 * 3 * 8 and lib.irec_ideal_workspace_bytes(0, 5) == 0
    x, loc, ls = C.images(3, 35, 2, 3)
    ll = np.zeros(2)
    assert lib.irec_loglik_host(p(x), p(loc), p(ls), 3, 2, 3, 35, C.BINSIZE, p(ll), 0) == 0
    assert lib.irec_loglik_host(p(x), p(loc), p(ls), 2, 2, 3, 35, C.BINSIZE, p(ll), 0) == _lib.IREC_E_INVALID
    assert lib.irec_loglik_host(p(x), p(loc), p(ls), 3, 2, 3, 35, 0.0, p(ll), 0) == _lib.IREC_E_INVALID


# ---- the Python layer on CPU tensors ------------------------------------------------------------------------------------------------------
def test_python_layer_takes_the_host_twins():
    from irec import ideal
    mq, sq, mp, sp = (torch.from_numpy(np.array(a)).reshape(3, 17, 241) for a in C.stats(4097, 3))
    N = types.SimpleNamespace
    sample, kl = ideal.posterior_draw(N(loc=mq, scale=sq), N(loc=mp, scale=sp), C.SEED, C.TAG, C.BASE)
    want = C.host_draw_of(4097, 3)
    assert sample.shape == mq.shape and sample.numpy().tobytes() == want[0].tobytes() and kl.numpy().tobytes() == want[1].tobytes()
    x, loc, ls = C.images(3, 2731, 3, 3)
    ll = ideal.log_likelihood(torch.from_numpy(np.array(x)).reshape(3, 3, 2731, 1), torch.from_numpy(np.array(loc)).reshape(3, 3, 2731, 1),
                              torch.from_numpy(np.array(ls)))
    assert ll.dtype == torch.float64 and ll.numpy().tobytes() == C.host_loglik_of((3, 2731, 3, 3)).tobytes()
    one = ideal.log_likelihood(torch.from_numpy(np.array(x)).reshape(3, 3, 2731, 1), torch.from_numpy(np.array(loc)).reshape(3, 3, 2731, 1), -3.5)
    assert one.numpy().tobytes() == C.host_loglik(x, loc, np.array([-3.5], np.float32)).tobytes()
    with pytest.raises(ValueError):
        ideal.posterior_draw(N(loc=mq, scale=sq), N(loc=mp, scale=sp[:2]), 1, 0)
    with pytest.raises(ValueError):
        ideal.log_likelihood(torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 4), torch.zeros(2))


def test_models_refuse_what_is_not_built():
    from irec.models import BidirectionalResNetVAE, Large2LevelVAE
    from irec.models.resnet_vae import ModelError
    with pytest.raises(NotImplementedError):
        Large2LevelVAE(level_1_filters=4, level_2_filters=2).forward(torch.zeros(1, 3, 64, 64))
    for family in ("gaussian", "laplace", "ms-ssim"):
        model = BidirectionalResNetVAE(num_res_blocks=1, sampler="beam_search", sampler_args={"n_beams": 2, "extra_samples": 1.},
                                       likelihood_function=family, deterministic_filters=4, stochastic_filters=2, kl_per_partition=3.)
        with pytest.raises(ModelError, match=family):
            model.forward(torch.zeros(1, 3, 8, 8), seed=1)


# ---- the harness's columns, with stub models ------------------------------------------------------------------------------------------------
import test_harness_drivers_host as D  # noqa: E402  (the stub models and their canned rows; no test of it is collected from here)

RESIDUAL = np.array([1000.5, 2000.25, 3000.125, 4000.0625, 5000.0])
KL = np.array([300.0, 310.5, 320.25, 330.125, 340.0625])
COMP_KL = np.array([305.0, 315.0, 325.0, 335.0, 345.0])


class IdealRVAE(D.StubRVAE):
    """StubRVAE with the ideal surface: canned residual / kl / comp_kl per image tag; it records (tags, seed, image_base) per pass."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.passes = []

    def coded_kl(self):
        return torch.from_numpy(COMP_KL[self.last])

    def compress_packed(self, image, seed, update_sampler=False):
        self.last = D.tags(image)
        return super().compress_packed(image, seed, update_sampler)

    def compress(self, image, seed, update_sampler=False):
        self.last = D.tags(image)
        return super().compress(image, seed, update_sampler)

    def forward(self, images, seed, image_base=0):
        ids = D.tags(images)
        self.passes.append((ids, seed, image_base))
        self.log_likelihood = torch.from_numpy(-RESIDUAL[ids])
        self._kl = torch.from_numpy(KL[ids])
        return images

    def kl_divergence(self):
        return self._kl


IDEAL_KEYS = {"residual", "kl", "lossless_bpp", "lossy_bpp", "bpd", "comp_kl", "overhead_bits"}


@pytest.mark.parametrize("packed", [True, False], ids=["packed_host_leg", "per_image"])
def test_compress_images_ideal_columns(tmp_path, packed):
    from irec import harness
    names = [f"im{i}" for i in range(5)]
    plain = harness.compress_images(IdealRVAE(fail={2}), D.tagged(range(5), D.HW), names, D.SEED, D.BLOCK, str(tmp_path / "plain"), batch=2, packed=packed)
    model = IdealRVAE(fail={2})
    rows = harness.compress_images(model, D.tagged(range(5), D.HW), names, D.SEED, D.BLOCK, str(tmp_path / "ideal"), batch=2, packed=packed, ideal=True)
    assert model.passes == [([0, 1], D.SEED, 0), ([4], D.SEED, 4)]           # image_base: the image's number in the call
    assert rows[2] == plain[2] and rows[3] == plain[3] and "error" in rows[2]
    ln2, hw = float(np.log(2.0)), D.HW * D.HW
    for i in (0, 1, 4):
        r, p = rows[i], plain[i]
        assert set(p) == D.KEYS and set(r) == D.KEYS | IDEAL_KEYS
        assert all(r[k] == p[k] for k in p if k != "comp_time")               # a row without the flag is the row it was
        assert r["residual"] == RESIDUAL[i] and r["kl"] == KL[i] and r["comp_kl"] == COMP_KL[i]
        assert r["lossless_bpp"] == (KL[i] + RESIDUAL[i]) / (hw * ln2) and r["lossy_bpp"] == KL[i] / (hw * ln2)
        assert r["bpd"] == (r["kl"] + r["residual"]) / (hw * 3 * ln2)
        assert r["overhead_bits"] == r["comp_codelength"] - COMP_KL[i] / ln2


class IdealLossy(D.StubLossy):
    def __init__(self, **kw):
        super().__init__(**kw)
        self.passes = []

    def compress_rec(self, images, *args, **kw):
        z = torch.zeros(images.shape[0], 1)                        # (what quality=True's kld column reads: unit distributions, KL 0)
        self.level_1_posterior = self.level_1_prior = self.level_2_posterior = self.level_2_prior = types.SimpleNamespace(loc=z, scale=z + 1)
        return super().compress_rec(images, *args, **kw)

    def forward(self, tensor, sampling_fn=None, seed=None, image_base=0):
        ids = D.tags(tensor)
        self.passes.append((ids, seed, image_base))
        self._kl = [torch.from_numpy(KL[ids]), torch.from_numpy(COMP_KL[ids])]
        return None, (tensor + 0.01).clamp(0, 1)

    def kl_divergence(self):
        return self._kl


def test_compress_images_lossy_ideal_columns(tmp_path):
    from irec import harness
    hw = 192
    images, names = D.tagged(range(3), hw), list("abc")
    plain = harness.compress_images_lossy(IdealLossy(), D.SAMPLER, images, names, D.SEED, D.BLOCK, str(tmp_path / "plain"), batch=2)
    model = IdealLossy()
    rows = harness.compress_images_lossy(model, D.SAMPLER, images, names, D.SEED, D.BLOCK, str(tmp_path / "ideal"), batch=2, ideal=True)
    assert model.passes == [([0, 1], D.SEED, 0), ([2], D.SEED, 2)]
    for i, (r, p) in enumerate(zip(rows, plain)):
        assert set(p) == D.KEYS and set(r) == D.KEYS | {"ideal_psnr", "ideal_ms_ssim", "ideal_kld", "ideal_lossy_bpp"}
        assert all(r[k] == p[k] for k in p if k != "comp_time")
        assert r["ideal_kld"] == KL[i] + COMP_KL[i] and r["ideal_lossy_bpp"] == r["ideal_kld"] / (hw * hw * float(np.log(2.0)))
        assert np.isfinite(r["ideal_psnr"]) and np.isfinite(r["ideal_ms_ssim"])
    both = harness.compress_images_lossy(IdealLossy(), D.SAMPLER, images, names, D.SEED, D.BLOCK, str(tmp_path / "both"), batch=2, quality=True, ideal=True)
    only = harness.compress_images_lossy(IdealLossy(), D.SAMPLER, images, names, D.SEED, D.BLOCK, str(tmp_path / "only"), batch=2, quality=True)
    for b, o, r in zip(both, only, rows):
        assert set(b) == set(o) | set(r) and all(b[k] == o[k] for k in o if k != "comp_time") and all(b[k] == r[k] for k in r if k != "comp_time")
