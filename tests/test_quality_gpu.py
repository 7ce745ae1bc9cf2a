"""GPU tests of the quality metrics (irec_quality_device through irec.metrics, harness.compress_images_lossy(quality=True)) against the
float64 referee of tests/quality_cases.py under its tolerance rule, and the properties the header promises: the same bits from run to
run and for an image alone or inside a batch, stores only into the outputs and the sized workspace, capturable in a graph."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import guarded as G
import quality_cases as Q

pytestmark = pytest.mark.gpu


def _quality(a, b, power_factors, device="cuda", **kw):
    from irec import metrics
    out = metrics.quality(torch.from_numpy(np.array(a)).to(device), torch.from_numpy(np.array(b)).to(device), power_factors, **kw)
    return tuple(t.cpu().numpy() for t in out)


@functools.lru_cache(maxsize=None)
def _device(shape_name, family):
    a, b = Q.fixture(shape_name, family)
    return _quality(a, b, Q.SHAPES[shape_name][1], **Q.UNIT)


@pytest.mark.parametrize("shape_name,family", Q.CASES)
def test_device_against_referee(engine, shape_name, family):
    y = Q.yardstick(shape_name, family)
    psnr, ms, per_scale = _device(shape_name, family)
    who = f"device {shape_name}/{family}"
    y.check("per_scale", per_scale, who)
    y.check("psnr", psnr, who)
    y.check("ms_ssim", ms, who, flat=family == "flat")
    if family == "bad":
        assert (ms == 0.0).all()


@pytest.mark.parametrize("shape_name,family", Q.CASES)
def test_device_against_host_twin(engine, shape_name, family):
    """The device against the host twin under the same rule (the two share the core header but not the compiler: not bitwise)."""
    a, b = Q.fixture(shape_name, family)
    y = Q.yardstick(shape_name, family)
    dev, host = _device(shape_name, family), _quality(a, b, y.power_factors, device="cpu", **Q.UNIT)
    for kind, d, h in zip(("psnr", "ms_ssim", "per_scale"), dev, host):
        e = y.e_ref32[kind]
        for g, w in zip(np.asarray(d, np.float64).reshape(-1), np.asarray(h, np.float64).reshape(-1)):
            tol = max(2.0 * e, 16.0 * Q.ulp32(w))
            assert abs(g - w) <= tol, f"{shape_name}/{family} {kind}: device {g!r}, host twin {w!r}, tolerance {tol:.3e}"


def test_identical_images_on_the_device(engine):
    a, _ = Q.fixture("odd_every_scale", "noise")
    psnr, ms, per_scale = _quality(a, a, Q.POWER_FACTORS, **Q.UNIT)
    assert (ms == 1.0).all() and (per_scale == 1.0).all() and np.isposinf(psnr).all()


def test_run_to_run_bitwise(engine):
    a, b = Q.fixture("odd_every_scale", "noise")
    first = _device("odd_every_scale", "noise")
    again = _quality(a, b, Q.POWER_FACTORS, **Q.UNIT)
    for u, v in zip(first, again):
        assert u.tobytes() == v.tobytes()


def test_batch_independence_bitwise(engine):
    """An image alone and the same image third of five: the same bits; a NaN in another image of the batch changes nothing."""
    rng = np.random.default_rng(21)
    shape, pf = (5, 3, 75, 139), Q.POWER_FACTORS[:3]
    b = Q._structured(rng, shape).astype(np.float32)
    a = (b + rng.normal(0, 5, size=shape)).astype(np.float32)
    batch = _quality(a, b, pf, **Q.UNIT)
    alone = _quality(a[2:3], b[2:3], pf, **Q.UNIT)
    for u, v in zip(batch, alone):
        assert u[2:3].tobytes() == v.tobytes()
    a2 = a.copy()
    a2[1, 0, 40, 70] = np.nan
    dirty = _quality(a2, b, pf, **Q.UNIT)
    for u, v in zip(batch, dirty):
        assert u[[0, 2, 3, 4]].tobytes() == v[[0, 2, 3, 4]].tobytes()
    assert not np.isfinite(dirty[0][1]) and not np.isfinite(dirty[1][1])


@pytest.mark.parametrize("shape_name", ["odd_every_scale", "straddles_tiles", "single_11"])
def test_memory_contract(engine, shape_name):
    """One call inside a guarded arena: inputs at the natural (4 mod 256) offset, outputs pre-filled, the workspace exactly the sized
    bytes and filled with 0xFFFFFFFF (NaNs: whatever the call reads of it, it must have written first)."""
    import irec
    lib = engine.lib
    a, b = Q.fixture(shape_name, "noise")
    (n, c, h, w), pf = a.shape, Q.SHAPES[shape_name][1]
    need = lib.irec_quality_workspace_bytes(n, c, h, w, len(pf))
    assert need > 0
    arena = G.Arena(G.slack(6) + need + 8 * a.size + 4096, "cuda")
    ta, tb = arena.put(np.array(a), name="a"), arena.put(np.array(b), name="b")
    per_scale = arena.region(torch.float32, (n, c, len(pf), 2), "out", name="per_scale")
    sse = arena.region(torch.float32, (n,), "out", name="sse")
    ws = arena.workspace(need, 0xFFFFFFFF)
    arena.arm()
    p = irec._lib.IrecQualityParams(1.0, 0.0, 1.0, 0.0, 0, 0, 255.0, 0.01, 0.03)
    irec._lib.check(lib.irec_quality_device(ta.data_ptr(), tb.data_ptr(), n, c, h, w, len(pf), ctypes.byref(p), per_scale.data_ptr(), sse.data_ptr(),
                                            ws.data_ptr(), need, engine._stream()), "irec_quality_device")
    torch.cuda.synchronize()
    arena.check()
    from irec import metrics
    plain = metrics.moments(torch.from_numpy(np.array(a)).cuda(), torch.from_numpy(np.array(b)).cuda(), len(pf), **Q.UNIT)
    assert per_scale.cpu().numpy().tobytes() == plain[0].cpu().numpy().tobytes()
    assert sse.cpu().numpy().tobytes() == plain[1].cpu().numpy().tobytes()
    # a workspace one byte short: refused, nothing launched, nothing written
    ws.fill_(0xFF)
    assert lib.irec_quality_device(ta.data_ptr(), tb.data_ptr(), n, c, h, w, len(pf), ctypes.byref(p), per_scale.data_ptr(), sse.data_ptr(),
                                   ws.data_ptr(), need - 1, engine._stream()) == irec._lib.IREC_E_WORKSPACE
    torch.cuda.synchronize()
    assert bool((ws == 0xFF).all())


def test_graph_capture(engine):
    """metrics.quality captured by torch.cuda.graph on one stream: two replays on fresh inputs equal eager, bit for bit."""
    from irec import metrics
    pf = Q.POWER_FACTORS[:3]
    pairs = [tuple(torch.from_numpy(np.array(v)).cuda() for v in Q.fixture("straddles_tiles", family)) for family in ("noise", "blur")]
    eager = [metrics.quality(a, b, pf, **Q.UNIT) for a, b in pairs]
    sa, sb = torch.zeros_like(pairs[0][0]), torch.zeros_like(pairs[0][1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        metrics.quality(sa, sb, pf, **Q.UNIT)                   # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = metrics.quality(sa, sb, pf, **Q.UNIT)
    for (a, b), want in zip(pairs, eager):
        sa.copy_(a)
        sb.copy_(b)
        graph.replay()
        torch.cuda.synchronize()
        for g, w in zip(out, want):
            assert g.cpu().numpy().tobytes() == w.cpu().numpy().tobytes()


# ---- the lossy harness's results row ---------------------------------------------------------------------------------------------
H, W = 192, 256


@functools.lru_cache(maxsize=None)
def _lossy():
    import irec
    from irec import harness
    from irec.models import Large2LevelVAE
    torch.manual_seed(3)
    model = Large2LevelVAE(level_1_filters=8, level_2_filters=4).cuda().eval()
    sampler = irec.BeamSearchCoder(kl_per_partition=3., n_beams=10, extra_samples=1., block_size=100)
    torch.manual_seed(11)
    images = (torch.rand(2, 3, H, W) - 0.5).cuda()
    return model, sampler, images, harness


def test_lossy_rows_carry_quality(engine, tmp_path):
    model, sampler, images, harness = _lossy()
    names = ["q0", "q1"]
    plain = harness.compress_images_lossy(model, sampler, images, names, 42, 100, str(tmp_path / "plain"))
    rows = harness.compress_images_lossy(model, sampler, images, names, 42, 100, str(tmp_path / "quality"), quality=True, image_range=(-0.5, 0.5))
    assert [set(r) for r in plain] == [{"name", "comp_codelength", "comp_lossy_bpp", "comp_code_bpd", "code_nats", "n_indices",
                                        "indices_recovered", "comp_time"}] * 2
    assert [set(r) - set(p) for r, p in zip(rows, plain)] == [{"psnr", "ms_ssim", "kld", "lossy_bpp"}] * 2
    for r, p in zip(rows, plain):
        assert all(r[k] == p[k] for k in p if k != "comp_time") and r["indices_recovered"]
    # the same pass once more, for what the columns were computed from
    _, _, recon = model.compress_rec(images, 42, sampler, block_size=100)
    a = Q.transformed(recon.cpu().numpy(), 255.0, 127.5, True).astype(np.float32)
    b = Q.transformed(images.cpu().numpy(), 255.0, 127.5, False).astype(np.float32)
    y = Q.Yardstick(a, b)
    y.check("psnr", np.array([r["psnr"] for r in rows]), "lossy rows")
    y.check("ms_ssim", np.array([r["ms_ssim"] for r in rows]), "lossy rows")
    kld = np.zeros(2)
    for post, prior in ((model.level_1_posterior, model.level_1_prior), (model.level_2_posterior, model.level_2_prior)):
        mq, sq, mp, sp = (t.cpu().numpy().astype(np.float64) for t in (post.loc, post.scale, prior.loc, prior.scale))
        kl = np.log(sp / sq) + (sq * sq + (mq - mp) ** 2) / (2.0 * sp * sp) - 0.5
        kld += kl.reshape(2, -1).sum(axis=1)
    for i, r in enumerate(rows):
        assert abs(r["kld"] - kld[i]) <= 1e-9 * abs(kld[i]), (r["kld"], kld[i])
        assert r["lossy_bpp"] == r["kld"] / (H * W * float(np.log(2.0)))
