"""GPU tests of the ideal half of a results row: irec_posterior_draw_device / irec_loglik_device (csrc/irec_ideal.hip) against the host
twins bit for bit on every shape of tests/ideal_cases.py, the properties include/irec.h promises (stores only into the outputs and
the sized workspace, a NaN stays in its image, capturable in a graph), and the model and harness layers on small shims."""
import functools
import types

import numpy as np
import pytest
import torch

import guarded as G
import ideal_cases as C

pytestmark = pytest.mark.gpu
N = types.SimpleNamespace


def _cuda(a):
    return torch.from_numpy(np.array(a)).cuda()


def _device_draw(mq, sq, mp, sp, seed=C.SEED, tag=C.TAG, base=C.BASE):
    from irec import ideal
    mq, sq, mp, sp = (_cuda(a) for a in (mq, sq, mp, sp))
    sample, kl = ideal.posterior_draw(N(loc=mq, scale=sq), N(loc=mp, scale=sp), seed, tag, base)
    return sample.cpu().numpy(), kl.cpu().numpy()


def _device_loglik(x, loc, log_scales):
    from irec import ideal
    n, c, plane = x.shape
    return ideal.log_likelihood(_cuda(x).reshape(n, c, plane, 1), _cuda(loc).reshape(n, c, plane, 1), _cuda(log_scales)).cpu().numpy()


@pytest.mark.parametrize("dims,n", C.CASES, ids=[C.case_id(c) for c in C.CASES])
def test_draw_equals_the_host_twin(engine, dims, n):
    sample, kl = _device_draw(*C.stats(dims, n))
    want = C.host_draw_of(dims, n)
    assert sample.tobytes() == want[0].tobytes()
    assert kl.tobytes() == want[1].tobytes(), (kl, want[1])


@pytest.mark.parametrize("case", C.LOGLIK_CASES, ids=C.case_id)
def test_loglik_equals_the_host_twin(engine, case):
    ll = _device_loglik(*C.images(*case))
    assert ll.tobytes() == C.host_loglik_of(case).tobytes(), (ll, C.host_loglik_of(case))


@pytest.mark.parametrize("dims,n,align", [(5, 3, None), (4097, 3, None), (8193, 1, None), (4096, 3, None), (4096, 3, 0), (256, 3, 0)],
                         ids=lambda v: "natural" if v is None else str(v))
def test_draw_memory_contract(engine, dims, n, align):
    """One call inside a guarded arena: the float32 arrays at the natural offset (4 bytes past a 16-byte boundary: no 16-byte access
    is aligned) or on the boundary (the 16-byte runs), outputs pre-filled, the workspace exactly the sized bytes and filled with
    0xFFFFFFFF (NaNs: whatever the call reads of it, it must have written first), inputs unchanged, the host twin's bits."""
    import irec
    lib = engine.lib
    need = lib.irec_ideal_workspace_bytes(n, dims)
    assert need == 8 * n * -(-dims // C.TILE)
    arena = G.Arena(G.slack(8) + need + 5 * 4 * n * dims + 8 * n + 4096, "cuda")
    ins = [arena.put(np.array(a), name=nm, align=align) for a, nm in zip(C.stats(dims, n), ("mq", "sq", "mp", "sp"))]
    sample = arena.region(torch.float32, (n, dims), "out", name="sample", align=align)
    kl = arena.region(torch.int64, (n,), "out", name="kl")                     # (float64 bits)
    ws = arena.workspace(need, 0xFFFFFFFF)
    arena.arm()
    call = lambda nbytes: lib.irec_posterior_draw_device(*(t.data_ptr() for t in ins), n, dims, C.SEED, C.TAG, C.BASE, sample.data_ptr(),  # noqa: E731
                                                         kl.data_ptr(), ws.data_ptr(), nbytes, engine._stream())
    irec._lib.check(call(need), "irec_posterior_draw_device")
    torch.cuda.synchronize()
    arena.check()
    want = C.host_draw_of(dims, n)
    assert sample.cpu().numpy().tobytes() == want[0].tobytes() and kl.cpu().numpy().tobytes() == want[1].tobytes()
    # a workspace one byte short: refused, nothing launched, nothing written
    ws.fill_(0xFF)
    sample.fill_(-7.0)
    assert call(need - 1) == irec._lib.IREC_E_WORKSPACE
    torch.cuda.synchronize()
    assert bool((ws == 0xFF).all()) and bool((sample == -7.0).all())


@pytest.mark.parametrize("case,align", [((3, 1366, 1, 3), None), ((3, 2731, 3, 3), None), ((3, 1024, 2, 1), 0), ((1, 5, 3, 1), None)],
                         ids=lambda v: "natural" if v is None else (str(v) if isinstance(v, int) else C.case_id(v)))
def test_loglik_memory_contract(engine, case, align):
    import irec
    lib = engine.lib
    x, loc, ls = C.images(*case)
    n, c, plane = x.shape
    need = lib.irec_ideal_workspace_bytes(n, c * plane)
    arena = G.Arena(G.slack(6) + need + 2 * 4 * x.size + 8 * n + 4096, "cuda")
    tx, tl, ts = arena.put(np.array(x), name="x", align=align), arena.put(np.array(loc), name="loc", align=align), arena.put(np.array(ls), name="log_scales")
    ll = arena.region(torch.int64, (n,), "out", name="ll")
    ws = arena.workspace(need, 0xFFFFFFFF)
    arena.arm()
    call = lambda nbytes: lib.irec_loglik_device(tx.data_ptr(), tl.data_ptr(), ts.data_ptr(), ls.size, n, c, plane, C.BINSIZE, ll.data_ptr(),  # noqa: E731
                                                 ws.data_ptr(), nbytes, engine._stream())
    irec._lib.check(call(need), "irec_loglik_device")
    torch.cuda.synchronize()
    arena.check()
    assert ll.cpu().numpy().tobytes() == C.host_loglik_of(case).tobytes()
    ws.fill_(0xFF)
    assert call(need - 1) == irec._lib.IREC_E_WORKSPACE
    torch.cuda.synchronize()
    assert bool((ws == 0xFF).all())


def test_nan_stays_in_its_image(engine):
    mq, sq, mp, sp = (a.copy() for a in C.stats(4097, 3))
    sq[1, 4096] = np.nan
    sample, kl = _device_draw(mq, sq, mp, sp)
    want = C.host_draw_of(4097, 3)
    assert np.isnan(kl[1]) and kl[[0, 2]].tobytes() == want[1][[0, 2]].tobytes()
    assert sample[[0, 2]].tobytes() == want[0][[0, 2]].tobytes() and np.isnan(sample[1, 4096]) and sample[1, :4096].tobytes() == want[0][1, :4096].tobytes()
    case = (3, 2731, 3, 3)
    x, loc, ls = (a.copy() for a in C.images(*case))
    x[1, 0, 0] = np.nan
    ll = _device_loglik(x, loc, ls)
    assert np.isnan(ll[1]) and ll[[0, 2]].tobytes() == C.host_loglik_of(case)[[0, 2]].tobytes()


def test_graph_capture(engine):
    """posterior_draw and log_likelihood captured by torch.cuda.graph on one stream: replays on fresh inputs equal eager, bit for bit."""
    from irec import ideal
    first = tuple(_cuda(a) for a in C.stats(8193, 3))
    stats = [first, tuple(t.flip(0).contiguous() for t in first)]              # two input sets: the images in either order
    x, loc, ls = (_cuda(a) for a in C.images(3, 2731, 3, 3))
    pix = [(x, loc, ls), (x.flip(0).contiguous(), loc.flip(0).contiguous(), ls)]
    shape4 = (3, 3, 2731, 1)

    def run(st, px):
        sample, kl = ideal.posterior_draw(N(loc=st[0], scale=st[1]), N(loc=st[2], scale=st[3]), C.SEED, C.TAG, C.BASE)
        return sample, kl, ideal.log_likelihood(px[0].reshape(shape4), px[1].reshape(shape4), px[2])
    eager = [run(st, px) for st, px in zip(stats, pix)]
    static_st, static_px = tuple(torch.zeros_like(t) + 1 for t in stats[0]), tuple(torch.zeros_like(t) for t in pix[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(static_st, static_px)                                # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run(static_st, static_px)
    for st, px, want in zip(stats, pix, eager):
        for dst, src in zip(static_st + static_px, st + px):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        for g, w in zip(out, want):
            assert g.cpu().numpy().tobytes() == w.cpu().numpy().tobytes()


# ---- the models ---------------------------------------------------------------------------------------------------------------------------
SEED = 42


@functools.lru_cache(maxsize=None)
def _rvae():
    from irec.models import BidirectionalResNetVAE
    torch.manual_seed(0)
    m = BidirectionalResNetVAE(num_res_blocks=2, sampler="beam_search", sampler_args={"n_beams": 20, "extra_samples": 1.2},
                               coder_args={"block_size": 1000}, deterministic_filters=8, stochastic_filters=4, kl_per_partition=3.)
    with torch.no_grad():
        m._generative_base.normal_(0, 0.5)
        m.likelihood_log_scale.fill_(-3.0)
    m = m.cuda().eval()
    torch.manual_seed(7)
    return m, torch.rand(3, 3, 32, 32, device="cuda") - 0.5


@functools.lru_cache(maxsize=None)
def _lossy(hw):
    import irec
    from irec.models import Large2LevelVAE
    torch.manual_seed(3)
    model = Large2LevelVAE(level_1_filters=8, level_2_filters=4).cuda().eval()
    sampler = irec.BeamSearchCoder(kl_per_partition=3., n_beams=10, extra_samples=1., block_size=100)
    torch.manual_seed(11)
    return model, sampler, (torch.rand(2, 3, hw, hw) - 0.5).cuda()


class _Reconstructions:
    """The clipped reconstructions that the model's passes form while this is open (forward returns them + 0.5, which does not
    round-trip), in order."""

    def __init__(self, model):
        self.model, self.seen = model, []

    def __enter__(self):
        finish = self.model._finish
        self.model._finish = lambda tensor: self.seen.append(finish(tensor)) or self.seen[-1]
        return self.seen

    def __exit__(self, *exc):
        del self.model._finish
        return False


def _cpu_kl(posterior, prior, tag, base):
    from irec import ideal
    cpu = lambda d: N(loc=d.loc.cpu(), scale=d.scale.cpu())  # noqa: E731
    return ideal.posterior_draw(cpu(posterior), cpu(prior), SEED, tag, base)


def test_rvae_forward(engine):
    from irec import ideal
    m, images = _rvae()
    with _Reconstructions(m) as seen:
        first = m.forward(images, seed=SEED, image_base=4)
    ll, kls = m.log_likelihood.clone(), [k.clone() for k in m.kl_divergence(reduce=False)]
    assert torch.equal(first, seen[0] + 0.5)
    again = m.forward(images, seed=SEED, image_base=4)
    assert torch.equal(first, again) and torch.equal(ll, m.log_likelihood) and first.shape == images.shape
    assert float(first.min()) >= 1. / 512. and float(first.max()) <= 1. - 1. / 512.
    assert len(kls) == 2 and all(k.shape == (3,) and k.dtype == torch.float64 for k in kls) and ll.shape == (3,) and ll.dtype == torch.float64
    assert torch.equal(m.kl_divergence(), kls[0] + kls[1])
    for r, block in enumerate(m.residual_blocks):
        sample, kl = _cpu_kl(block.posterior, block.prior, r, 4)
        assert torch.equal(kl, block.kl.cpu()) and torch.equal(kl, kls[r].cpu())
    # the likelihood of the clipped reconstruction, on the host twin
    assert torch.equal(ideal.log_likelihood(images.cpu(), seen[0].cpu(), -3.0), ll.cpu())
    one = m.forward(images[1:2], seed=SEED, image_base=5)
    assert one.shape == (1, 3, 32, 32) and torch.isfinite(m.kl_divergence()).all()
    assert not torch.equal(m.forward(images, seed=SEED + 1, image_base=4), first)
    assert not torch.equal(m.forward(images, seed=SEED, image_base=5), first)


def test_rvae_forward_per_channel_scales(engine):
    from irec import ideal
    m, images = _rvae()
    try:
        m.set_likelihood_scales([-3.0, -3.5, -2.5])
        with _Reconstructions(m) as seen:
            m.forward(images, seed=SEED)
        want = ideal.log_likelihood(images.cpu(), seen[0].cpu(), torch.tensor([-3.0, -3.5, -2.5]))
        assert torch.equal(want, m.log_likelihood.cpu())
    finally:
        m.set_likelihood_scales(None)


def test_two_level_forward(engine):
    model, _, images = _lossy(64)
    none, first = model.forward(images, seed=SEED, image_base=2)
    kls = [k.clone() for k in model.kl_divergence()]
    _, again = model.forward(images, seed=SEED, image_base=2)
    assert none is None and torch.equal(first, again) and first.shape == images.shape
    assert len(kls) == 2 and all(k.shape == (2,) and k.dtype == torch.float64 for k in kls)
    for kl, got in zip((_cpu_kl(model.level_2_posterior, model.level_2_prior, 2, 2)[1], _cpu_kl(model.level_1_posterior, model.level_1_prior, 1, 2)[1]), kls):
        assert torch.equal(kl, got.cpu())
    with pytest.raises(NotImplementedError):
        model.forward(images)


@pytest.mark.parametrize("leg", ["packed", "device", "lists"])
def test_compress_images_ideal_rows(engine, tmp_path, leg):
    from irec import harness
    m, images = _rvae()
    names = ["a", "b", "c"]
    kw = {"packed": dict(), "device": dict(rec_on_device=True), "lists": dict(packed=False)}[leg]
    plain = harness.compress_images(m, images, names, SEED, 1000, str(tmp_path / "plain"), batch=2, **kw)
    rows = harness.compress_images(m, images, names, SEED, 1000, str(tmp_path / "ideal"), batch=2, ideal=True, **kw)
    new = {"residual", "kl", "lossless_bpp", "lossy_bpp", "bpd", "comp_kl", "overhead_bits"}
    ln2 = float(np.log(2.0))
    ll, kl = [], []
    for lo, hi in ((0, 2), (2, 3)):                               # the batches' own passes: image_base is the image's number in the call
        m.forward(images[lo:hi], seed=SEED, image_base=lo)
        ll += m.log_likelihood.cpu().tolist()
        kl += m.kl_divergence().cpu().tolist()
    for i, (r, p) in enumerate(zip(rows, plain)):
        assert set(r) - set(p) == new and all(r[k] == p[k] for k in p if k != "comp_time") and r["indices_recovered"]
        assert r["bpd"] == (r["kl"] + r["residual"]) / (32 * 32 * 3 * ln2)
        assert r["lossless_bpp"] == (r["kl"] + r["residual"]) / (32 * 32 * ln2) and r["lossy_bpp"] == r["kl"] / (32 * 32 * ln2)
        assert r["overhead_bits"] == r["comp_codelength"] - r["comp_kl"] / ln2
        assert np.isfinite(r["residual"]) and r["kl"] > 0 and r["comp_kl"] > 0
        assert r["kl"] == kl[i] and r["residual"] == -ll[i]


def test_lossy_rows_carry_ideal_quality(engine, tmp_path):
    from irec import harness
    model, sampler, images = _lossy(192)
    names = ["q0", "q1"]
    only = harness.compress_images_lossy(model, sampler, images, names, SEED, 100, str(tmp_path / "quality"), quality=True, image_range=(-0.5, 0.5))
    rows = harness.compress_images_lossy(model, sampler, images, names, SEED, 100, str(tmp_path / "ideal"), quality=True, ideal=True,
                                         image_range=(-0.5, 0.5))
    model.forward(images, seed=SEED)
    kl = sum(model.kl_divergence()).cpu().numpy()
    for i, (r, o) in enumerate(zip(rows, only)):
        assert set(r) - set(o) == {"ideal_psnr", "ideal_ms_ssim", "ideal_kld", "ideal_lossy_bpp"}
        assert all(r[k] == o[k] for k in o if k != "comp_time")
        assert np.isfinite(r["ideal_psnr"]) and np.isfinite(r["ideal_ms_ssim"]) and 0.0 <= r["ideal_ms_ssim"] <= 1.0
        assert r["ideal_kld"] == kl[i] and r["ideal_lossy_bpp"] == r["ideal_kld"] / (192 * 192 * float(np.log(2.0)))
