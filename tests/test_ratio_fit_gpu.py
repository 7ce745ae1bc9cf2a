"""The auxiliary-variance ratio fit on the GPU (csrc/irec_fit.hip behind irec_fit_aux_ratios) against its host twin
(irec_fit_aux_ratios_host, which tests/test_ratio_fit_host.py pins to the float64 referee): ratios, average counts and the
iterations of every fit step bit for bit -- and the coders that code with the fitted table, end to end on the device."""
import threading

import numpy as np
import pytest
import torch

import test_ratio_fit_host as H

pytestmark = pytest.mark.gpu

LN2 = np.log(2)


def _fit_both(stats, omega, **kw):
    host, dev = H.new_coder(omega), H.new_coder(omega)
    host.update_auxiliary_variance_ratios(*H.dists(stats), **kw)
    dev.update_auxiliary_variance_ratios(*H.dists(stats, "cuda"), **kw)
    assert host.last_path == "host" and dev.last_path == "device"
    return host, dev


def _same_fit(a, b, what=""):
    assert a.aux_variable_variance_ratios.tobytes() == b.aux_variable_variance_ratios.tobytes(), \
        (what, a.aux_variable_variance_ratios, b.aux_variable_variance_ratios)
    assert a.average_counts.tobytes() == b.average_counts.tobytes(), what
    assert a.last_fit_iters == b.last_fit_iters, (what, a.last_fit_iters, b.last_fit_iters)


@pytest.mark.parametrize("name", sorted(H.CASES))
def test_device_equals_host_twin(engine, name):
    make, omega = H.CASES[name]
    stats = make()
    host, dev = _fit_both(stats, omega, seed=H.SEED)
    _same_fit(host, dev, name)
    if name.startswith("reference"):                   # the reference's tests fit twice
        host.update_auxiliary_variance_ratios(*H.dists(stats), seed=H.SEED)
        dev.update_auxiliary_variance_ratios(*H.dists(stats, "cuda"), seed=H.SEED)
        _same_fit(host, dev, name + " (second call)")


@pytest.mark.parametrize("n_rows", [1, 255, 256, 257, 700])
def test_fewer_and_more_rows_than_compute_units(engine, n_rows):
    host, dev = _fit_both(H.survey_rows(n_rows, 1000, first=300), 3.)
    assert len(host.last_fit_iters) >= 5
    _same_fit(host, dev, f"{n_rows} rows")


def test_steps_that_stop_inside_at_the_end_of_and_one_past_a_launch_chunk(engine):
    """The launches of a fit step are enqueued in chunks; `done` is read between chunks.  survey-16x1000-om3 takes
    [2, 189, 322, 258, 295, 357, 523] iterations: chunks of 189 / 188 / 2 / 1 / 100 put stops at the end of a chunk, one past a
    chunk (the second chunk's first launch), and inside one."""
    from irec import _lib
    lib = _lib.load()
    stats = H.survey_rows(16, 1000)
    host = H.new_coder(3.)
    host.update_auxiliary_variance_ratios(*H.dists(stats))
    assert host.last_fit_iters == [2, 189, 322, 258, 295, 357, 523]
    try:
        for chunk in (189, 188, 2, 1, 100):
            assert lib.irec_test_fit_chunk(chunk) > 0
            dev = H.new_coder(3.)
            dev.update_auxiliary_variance_ratios(*H.dists(stats, "cuda"))
            _same_fit(host, dev, f"chunk {chunk}")
    finally:
        lib.irec_test_fit_chunk(0)
    assert lib.irec_test_fit_chunk(0) == 64


def test_max_iters_on_the_device(engine):
    host, dev = _fit_both(H.survey_rows(16, 1000), 3., max_iters=5)
    assert max(dev.last_fit_iters) == 5
    _same_fit(host, dev, "max_iters=5")
    host, dev = _fit_both(H.survey_rows(16, 1000), 3., max_iters=1)
    assert dev.last_fit_iters == [1] * len(dev.last_fit_iters)
    _same_fit(host, dev, "max_iters=1")


def test_two_fits_in_flight_on_two_streams(engine):
    cases = [(H.survey_rows(16, 1000), 3.), (H.survey_rows(12, 1000, first=50), 5.)]
    want = []
    for stats, omega in cases:
        c = H.new_coder(omega)
        c.update_auxiliary_variance_ratios(*H.dists(stats))
        want.append(c)
    got, errors = [H.new_coder(om) for _, om in cases], []
    dev = [H.dists(stats, "cuda") for stats, _ in cases]
    torch.cuda.synchronize()

    def work(i):
        try:
            with torch.cuda.stream(torch.cuda.Stream()):
                for _ in range(2):       # (twice: the second fit averages, both stay in flight longer)
                    got[i].update_auxiliary_variance_ratios(*dev[i])
        except Exception as e:           # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for (stats, _), c in zip(cases, want):
        c.update_auxiliary_variance_ratios(*H.dists(stats))
    for i in range(2):
        _same_fit(want[i], got[i], f"stream {i}")


def _tensor(oracle, image_id=5150, n=8192):
    stats = oracle.synthetic_latent(image_id, n)
    dev = [torch.from_numpy(a[None]).cuda() for a in stats]
    return stats, H._Dist(dev[0], dev[1]), H._Dist(dev[2], dev[3])


def test_fit_then_beam_search_round_trip_and_oracle_indices(engine, oracle):
    import irec
    from irec.coding import CodingError
    stats, q, p = _tensor(oracle)
    c = irec.BeamSearchCoder(kl_per_partition=3., n_beams=20, extra_samples=1.2, extrapolate_auxiliary_ratios=False, block_size=1000)
    with pytest.raises(CodingError, match="has not been initialized yet"):
        c.encode(q, p, seed=42)
    c.update_auxiliary_variance_ratios(q, p, seed=42)
    assert c.last_path == "device" and c.average_counts[-1] >= 1 and c.average_counts[1] == 8    # 9 blocks, the last one left off
    ratios = c.aux_variable_variance_ratios.copy()
    idx, sample = c.encode(q, p, seed=42)
    assert c._engine_for(q.loc).max_partitions == ratios.size
    assert torch.equal(c.decode(p, idx, seed=42), sample)
    oracle.set_aux_ratios(ratios)
    try:
        ridx, rs = oracle.encode_tensor(*stats, 42, 3.0, 36, 20, block_size=1000)
    finally:
        oracle.set_aux_ratios(None)
    assert idx == ridx and np.array_equal(sample.cpu().numpy()[0], rs)
    # a second fit replaces the table: the next encode runs over a context of the new one
    c.update_auxiliary_variance_ratios(q, p, seed=43)
    assert c.aux_variable_variance_ratios.tobytes() != ratios.tobytes()
    idx2, sample2 = c.encode(q, p, seed=42)
    oracle.set_aux_ratios(c.aux_variable_variance_ratios)
    try:
        ridx2, rs2 = oracle.encode_tensor(*stats, 42, 3.0, 36, 20, block_size=1000)
    finally:
        oracle.set_aux_ratios(None)
    assert idx2 == ridx2 and np.array_equal(sample2.cpu().numpy()[0], rs2)
    # a block whose K exceeds the fitted table: the reference's message
    sharp = oracle.synthetic_latent(5151, 8192)
    sq = torch.from_numpy((sharp[1] * 0.25).astype(np.float32)[None]).cuda()
    with pytest.raises(CodingError, match=f"Maximum possible number of partitions is {c.aux_variable_variance_ratios.size}"):
        c.encode(H._Dist(torch.from_numpy(sharp[0][None]).cuda(), sq),
                 H._Dist(torch.from_numpy(sharp[2][None]).cuda(), torch.from_numpy(sharp[3][None]).cuda()), seed=42)


def test_fit_then_importance_coder_round_trip(engine, oracle):
    import irec
    stats, q, p = _tensor(oracle, 5152)
    c = irec.GaussianCoder(kl_per_partition=3., sampler=irec.ImportanceSampler(coding_bits=3. / LN2),
                           extrapolate_auxiliary_ratios=False, block_size=1000)
    c.update_auxiliary_variance_ratios(q, p, seed=42)
    assert c.last_path == "device"
    idx, sample = c.encode(q, p, seed=42)
    assert c.last_path == "device" and len(idx) == 9
    assert torch.equal(c.decode(p, idx, seed=42), sample)
    host = irec.GaussianCoder(kl_per_partition=3., sampler=irec.ImportanceSampler(coding_bits=3. / LN2),
                              extrapolate_auxiliary_ratios=False, block_size=1000)
    host.set_auxiliary_variance_ratios(c.aux_variable_variance_ratios, average_counts=c.average_counts)
    cpu = [torch.from_numpy(a[None]) for a in stats]
    idx_h, sample_h = host.encode(H._Dist(cpu[0], cpu[1]), H._Dist(cpu[2], cpu[3]), seed=42)
    assert [[int(v) for v in ix] for ix in idx] == [[int(v) for v in ix] for ix in idx_h] and torch.equal(sample.cpu(), sample_h)


def test_model_update_coders_then_compress(engine):
    from irec.models import BidirectionalResNetVAE
    torch.manual_seed(0)
    m = BidirectionalResNetVAE(num_res_blocks=2, sampler="beam_search", sampler_args={"n_beams": 20, "extra_samples": 1.2},
                               coder_args={"block_size": 1000, "extrapolate_auxiliary_ratios": False},
                               deterministic_filters=16, stochastic_filters=8, kl_per_partition=3.)
    with torch.no_grad():
        for b in m.residual_blocks:
            for head in (b.gen_posterior_loc_head, b.gen_posterior_log_scale_head, b.infer_posterior_loc_head,
                         b.infer_posterior_log_scale_head, b.prior_loc_head, b.prior_log_scale_head):
                head.weight.mul_(0.3)
        m._generative_base.normal_(0, 0.5)
    m = m.cuda().eval()
    torch.manual_seed(1)
    images = torch.rand(4, 3, 64, 64, device="cuda") - 0.5
    assert not any(b.coder._initialized for b in m.residual_blocks)
    m.update_coders(images, seed=42)
    for b in m.residual_blocks:
        assert b.coder._initialized and b.coder.last_path == "device"
        assert b.coder.average_counts[-1] >= 1 and b.coder.aux_variable_variance_ratios.size >= 2
        assert b.coder.average_counts[1] <= 4 * 8           # 8192 dims a tensor: eight full blocks of 1000 each, the ninth left off
    block_indices, recon = m.compress(images[:1], seed=42)
    assert len(block_indices) == 2 and recon.shape == (1, 3, 64, 64) and torch.isfinite(recon).all()
    assert torch.equal(m.decompress(block_indices, 42, (1, 3, 64, 64)), recon)
