"""The seed domain on the device, bit for bit against the oracle (tests/seed_cases.py has the ladder, the rules and the inputs): every
encoder family, every decode mode, table reuse across seeds that differ by 2^32 or by M = 2^31 - 1, the importance coder and the
ratio fit, and the .rec / .recs files of both models from compress to decompress at the first and last seeds a header field can tell
apart from a wrapped one.  Every call keeps a table window of seed_cases.TABLE_STEPS = 4 steps and blocks of K >= 8 partitions, so the
zero step (seed + t = 0 mod M, the Philox pair (0, M)) of M - 1 and M - 3 is drawn by the table kernels and that of M - 6 by the fused
draw behind the window."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import kernel_names as kn
import seed_cases as SC

pytestmark = pytest.mark.gpu

_ids = [SC.seed_id(s) for s in SC.SEEDS]
_bad_ids = [SC.seed_id(s) for s in SC.HEADER_BAD]
M = SC.M


@pytest.fixture(autouse=True)
def _stop_the_session_on_a_gpu_error():
    """A call that left the device in an error state ends the run: nothing more is started on it."""
    yield
    if torch.cuda.is_available():
        try:
            torch.cuda.synchronize()
        except Exception as e:          # noqa: BLE001
            pytest.exit(f"GPU error after a seed-domain test: {e}", returncode=3)


def _cuda(*arrays):
    return [torch.from_numpy(np.array(a, copy=True)).cuda() for a in arrays]           # (a copy: the shared inputs are read-only)


def _n_cu(engine):
    return engine.plan(engine.params(3.0, 36, 20), engine.layout(1, 192, 192, 42), 8)["n_cu"]


def _same(a, b):
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


# ==== encoders: one call per family, every seed of the ladder ===================================================================================
def _family_params():
    return [pytest.param(family, id=kn.family_id(family)) for family in kn.FAMILIES]


@pytest.mark.parametrize("seed", SC.SEEDS, ids=_ids)
@pytest.mark.parametrize("family", _family_params())
def test_every_encoder_family_at_every_seed(engine, oracle, family, seed):
    from irec import _lib
    n_cu = _n_cu(engine)
    c = SC.family_cases(n_cu)[family]
    assert c is not None, "the planner names no kernel of this family that serves the seed call"
    ridx, rs = SC.encoder_reference(family, seed, n_cu)
    n_blocks, dim, max_K = c["n_blocks"], c["dim"], c["max_K"]
    margins = bool(c["flags"] & _lib.IREC_FLAG_MARGINS)
    lay = engine.layout(n_blocks, dim, dim, seed)                      # one block per tensor, shuffled under the coding seed (coder.py:62-83)
    params = engine.params(c["omega"], c["S"], c["B"], c["flags"] & ~_lib.IREC_FLAG_MARGINS, table_steps=SC.TABLE_STEPS)
    plan = engine.plan(params, lay, max_K, margins=margins)
    assert kn.canonical(plan["kernel"], plan["split"]) == c["name"], (plan, c)
    assert plan["table_steps"] in (0, SC.TABLE_STEPS), plan           # (0: the generic kernel draws every step itself)
    q = _cuda(*SC.inputs(dim, n_blocks))
    if margins:
        K, idx, sample, _ = engine.encode_blocks_margins(params, lay, *q, seed, max_K)
    else:
        K, idx, sample = engine.encode_blocks(params, lay, *q, seed, max_K)
    torch.cuda.synchronize()
    Kh, ih, sh = K.cpu().numpy(), idx.cpu().numpy(), sample.cpu().numpy().reshape(n_blocks, dim)
    for i in range(n_blocks):
        row = lay.natural[i]
        assert Kh[row] == len(ridx[i]) and ih[row, :Kh[row]].tolist() == ridx[i], (family, SC.seed_id(seed), i, int(Kh[row]), len(ridx[i]))
    assert np.array_equal(sh, rs), (family, SC.seed_id(seed))


def test_congruent_seeds_code_a_block_identically(oracle):
    """TensorFlow truncates both halves of a seed pair mod M, so the draws of seed and seed + M are the same numbers; only the shuffle
    (CPython's random.Random(seed), every bit) tells them apart.  The oracle on one unshuffled block: the statement the device calls
    above are held to."""
    host = [a[0] for a in SC.inputs(64, 1)]
    for seed, twin in SC.CONGRUENT:
        a, b = oracle.encode_block(*host, seed, 1.0, 20, 10), oracle.encode_block(*host, twin, 1.0, 20, 10)
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and len(a[0]) >= SC.MIN_K


# ==== decoders: every mode, every seed =================================================================================================
# Omega of a layout: 1, the inputs' own -- except where the condition of seed_cases.check_partitions asks for less: at some seeds the
# shuffle puts a tensor's informative dim into the 64-dim tail of the 448-dim layout, whose block then has K = 7 at Omega = 1
_DECODE_OMEGA = {"3x448": 0.5, "4x1000": 1.0}
_DECODE_FAMILIES = ("team", "team, shared rows")      # the call whose rows are fed: the team family's (S = 1) and the shared rows' (S = 7)


@functools.lru_cache(maxsize=None)
def _decode_reference(layout_id, family, seed, n_cu):
    from oracle import oracle as O
    nt, n, bs = SC.DECODE_LAYOUTS[layout_id]
    c = SC.family_cases(n_cu)[family]
    host = SC.tensor_inputs(nt, n)
    ridx, rs, _ = O.encode_tensors_omp(*host, seed, _DECODE_OMEGA[layout_id], c["S"], c["B"], bs, max_K=32)
    SC.check_partitions([len(b) for t in ridx for b in t], (layout_id, family, SC.seed_id(seed)))
    dec = np.stack([O.decode_tensor(host[2][i], host[3][i], ridx[i], seed, c["S"], block_size=bs) for i in range(nt)])
    assert np.array_equal(dec, rs)
    return ridx, rs


@pytest.mark.parametrize("seed", SC.SEEDS, ids=_ids)
@pytest.mark.parametrize("family", _DECODE_FAMILIES, ids=[kn.family_id(f) for f in _DECODE_FAMILIES])
@pytest.mark.parametrize("layout_id", list(SC.DECODE_LAYOUTS))
def test_every_decode_mode_at_every_seed(engine, oracle, layout_id, family, seed):
    from irec import _lib
    from irec.engine import _ptr
    n_cu = _n_cu(engine)
    nt, n, bs = SC.DECODE_LAYOUTS[layout_id]
    c = SC.family_cases(n_cu)[family]
    ridx, rs = _decode_reference(layout_id, family, seed, n_cu)
    max_K = 32
    lay = engine.layout(nt, n, bs, seed)
    bpt = lay.blocks_per_tensor
    params = engine.params(_DECODE_OMEGA[layout_id], c["S"], c["B"], c["flags"] & ~_lib.IREC_FLAG_MARGINS, table_steps=SC.TABLE_STEPS)
    host = SC.tensor_inputs(nt, n)
    ql, qs, pl, ps = _cuda(*host)
    K, idx, sample = engine.encode_blocks(params, lay, ql, qs, pl, ps, seed, max_K)
    torch.cuda.synchronize()
    Kh, ih = K.cpu().numpy(), idx.cpu().numpy()
    for i in range(nt):
        for j in range(bpt):
            row = lay.natural[i * bpt + j]
            assert ih[row, :Kh[row]].tolist() == ridx[i][j], (layout_id, SC.seed_id(seed), i, j)
    assert np.array_equal(sample.cpu().numpy().reshape(nt, n), rs)
    # the decoders read exactly the K live slots of a row: what lies past them is set to another valid index (S - 1), not left as it came
    idx = torch.where(torch.arange(max_K, device="cuda")[None, :] < K[:, None], idx, torch.full_like(idx, c["S"] - 1)).contiguous()
    dparams = engine.params(params.kl_per_partition, params.n_samples, params.n_beams, 0, table_steps=SC.TABLE_STEPS)
    assert engine.lib.irec_decode_tensors_supported(ctypes.byref(dparams), n, bs)
    for mode in ("auto", "tensors", "tensors_fused", "tables", "fused", "legacy"):
        out = engine.decode_blocks(dparams, lay, pl, ps, seed, K, idx, mode=mode)
        assert torch.equal(out, sample), (mode, layout_id, SC.seed_id(seed))
    # irec_beam_decode_tensors through the C ABI: with the workspace its sizing function asks for, and without one
    tparams = engine.with_table_dims(dparams, lay)
    need = engine.lib.irec_decode_workspace_bytes(engine.ctx, ctypes.byref(tparams), max_K)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    for workspace, nbytes in ((ws, need), (None, 0)):
        out = torch.full_like(pl, float("nan"))
        _lib.check(engine.lib.irec_beam_decode_tensors(engine.ctx, ctypes.byref(tparams), nt, n, bs, _ptr(lay.natural_dev()), _ptr(lay.perm),
                                                       _ptr(pl), _ptr(ps), seed, max_K, _ptr(K), _ptr(idx), _ptr(out), _ptr(workspace), nbytes,
                                                       engine._stream()), "irec_beam_decode_tensors")
        assert torch.equal(out, sample), (nbytes, layout_id, SC.seed_id(seed))


# ==== table reuse: the stamps hold all 64 bits of the seed =============================================================================
_REUSE = dict(n_tensors=4, n=256, block_size=192, omega=1.0, S=20, B=10, max_K=32, layout_seed=5)    # blocks of 192 and 64 dims: two tables


@functools.lru_cache(maxsize=None)
def _reuse_reference(seed):
    """The oracle on the blocks of the reuse layout -- cut under the LAYOUT's seed, coded under `seed`: (indices per (tensor, block),
    sample [n_tensors, n])."""
    from oracle import oracle as O
    r = _REUSE
    host = SC.tensor_inputs(r["n_tensors"], r["n"])
    perm = O.tf_shuffle_perm(r["layout_seed"], r["n"])
    indices, sample = [], np.zeros((r["n_tensors"], r["n"]), np.float32)
    for i in range(r["n_tensors"]):
        for lo, hi in O.split_blocks(r["n"], r["block_size"]):
            g = perm[lo:hi]
            ix, z = O.encode_block(*(a[i][g] for a in host), seed, r["omega"], r["S"], r["B"], max_K=r["max_K"])
            indices.append(ix)
            sample[i, g] = z
    SC.check_partitions([len(ix) for ix in indices], ("reuse", SC.seed_id(seed)))
    return indices, sample


def _keep_words(engine):
    """keep[0..1] of the current stream's scratch after the last call (irec_kernels.h, head of the workspace): one word a table."""
    ws = engine._ws[int(torch.cuda.current_stream(engine.device).cuda_stream)]
    return ws[:512].view(torch.int32)[8:10].cpu().tolist()


def _reuse_call(engine, seed):
    """One call of the reuse layout under `seed`, checked against the oracle: (keep words, K, idx, sample on the host)."""
    from irec import _lib
    r = _REUSE
    lay = engine.layout(r["n_tensors"], r["n"], r["block_size"], r["layout_seed"])
    params = engine.params(r["omega"], r["S"], r["B"], _lib.IREC_FLAG_REUSE_TABLES | _lib.IREC_FLAG_TEAM, table_steps=SC.TABLE_STEPS)
    plan = engine.plan(params, lay, r["max_K"])
    assert plan["n_tables"] == 2 and plan["table_steps"] == SC.TABLE_STEPS, plan
    q = _cuda(*SC.tensor_inputs(r["n_tensors"], r["n"]))
    K, idx, sample = engine.encode_blocks(params, lay, *q, seed, r["max_K"])
    torch.cuda.synchronize()
    Kh, ih, sh = K.cpu().numpy(), idx.cpu().numpy(), sample.cpu().numpy().reshape(r["n_tensors"], r["n"])
    ridx, rs = _reuse_reference(seed)
    for b, want in enumerate(ridx):
        row = lay.natural[b]
        assert ih[row, :Kh[row]].tolist() == want, (SC.seed_id(seed), b)
    assert np.array_equal(sh, rs), SC.seed_id(seed)
    return _keep_words(engine), [ih[lay.natural[b], :Kh[lay.natural[b]]].tolist() for b in range(len(ridx))], sh


def _fresh_scratch(engine):
    engine._ws.pop(int(torch.cuda.current_stream(engine.device).cuda_stream), None)      # the next call gets a zero-headed one


def test_seeds_2_pow_32_apart_never_share_a_table(engine, oracle):
    s = 5
    _fresh_scratch(engine)
    assert _reuse_call(engine, s)[0] == [0, 0]                  # built
    assert _reuse_call(engine, s + 2 ** 32)[0] == [0, 0]        # the low words of the stamps are equal, the high words are not: rebuilt
    assert _reuse_call(engine, s)[0] == [0, 0]                  # ... and s's tables are gone
    assert _reuse_call(engine, s)[0] == [1, 1]                  # (the flag does keep a table whose stamp is the call's)
    assert _reuse_reference(s)[0] != _reuse_reference(s + 2 ** 32)[0]


def test_congruent_seeds_rebuild_their_tables(engine, oracle):
    """s and s + M demand the same bits, but a stamp compares seeds, not residues: the tables are rebuilt, which is safe."""
    s = 5
    _fresh_scratch(engine)
    first = _reuse_call(engine, s)
    assert first[0] == [0, 0]
    assert _reuse_call(engine, s)[0] == [1, 1]
    last = _reuse_call(engine, s + M)
    assert last[0] == [0, 0]
    assert last[1] == first[1] and np.array_equal(last[2], first[2])


def test_table_session_tells_seeds_2_pow_32_apart(engine, oracle):
    """Inside Engine.table_session() a twin of the previous call is told its tables are present and launches no table kernel: a call
    that differs from it only by 2^32 in the seed is no twin -- told so, it would code under s's tables and miss the oracle."""
    s = 5
    _fresh_scratch(engine)
    with engine.table_session():
        assert _reuse_call(engine, s)[0] == [0, 0]
        assert _reuse_call(engine, s + 2 ** 32)[0] == [0, 0]
        assert _reuse_call(engine, s)[0] == [0, 0]
        first = _reuse_call(engine, s)                          # the twin: tables present
        assert first[0] == [1, 1]
        assert _reuse_call(engine, s)[0] == [1, 1]
        last = _reuse_call(engine, s + M)
        assert last[0] == [0, 0] and last[1] == first[1] and np.array_equal(last[2], first[2])
    assert getattr(engine._tls, "session", None) is None


# ==== the importance coder and the ratio fit ========================================================================================
GC_SEEDS = (0, M - 3, 2 ** 32 + 5, -1, SC.SEED_BOUND)
_gc_ids = [SC.seed_id(s) for s in GC_SEEDS]
LN2 = np.log(2)


class _D:
    def __init__(self, loc, scale):
        self.loc, self.scale = loc, scale


def _gc_block(D):
    """One block of D dims whose KL is about 11 nats spread evenly (K = 4 at Omega = 3): float32 (mq, sq, mp, sp), each [1, D]."""
    rng = np.random.default_rng(4000 + D)
    mp = rng.normal(0.0, 1.0, D)
    sp = np.exp(rng.normal(0.0, 0.25, D))
    mq = mp + sp * np.sqrt(2.0 * 11.0 / D) * rng.choice([-1.0, 1.0], D)
    sq = sp * np.exp(-np.abs(rng.normal(0.0, 0.02, D)))
    return tuple(np.asarray(v, np.float32)[None] for v in (mq, sq, mp, sp))


@pytest.mark.parametrize("seed", GC_SEEDS, ids=_gc_ids)
@pytest.mark.parametrize("alpha", [np.inf, 2.5], ids=["argmax", "alpha2.5"])
@pytest.mark.parametrize("D", [37, 1100], ids=["narrow37", "wide1100"])
def test_importance_coder_at_the_seed_corners(engine, oracle, D, alpha, seed):
    """The device coder (the narrow kernel at 37 dims, the wide one at 1100) equals the host coder and the numpy referee of the gc
    tests (tests/gc_referee_alpha.py; at alpha = inf its selection is the arg-max), encode and decode."""
    import gc_referee as R
    import gc_referee_alpha as RA
    from gc_alpha_cases import coder_of
    host = _gc_block(D)
    omega, bits = 3.0, 3.0 / LN2
    dev_coder, host_coder = coder_of(omega, bits, alpha), coder_of(omega, bits, alpha)
    dev_coder.table_steps = dev_coder._max_K_hint = 8
    S = dev_coder.sampler.n_samples()
    K = oracle.num_aux(oracle.block_kl(*(a[0] for a in host)), omega)
    assert K >= 4
    if np.isinf(alpha):
        ridx, rz = R.encode_block(*(a[0] for a in host), seed, S, K, oracle.tf_random_normal)
    else:
        ridx, rz = RA.encode_block(*(a[0] for a in host), seed, S, K, oracle.tf_random_normal, alpha)
    ql, qs, pl, ps = _cuda(*host)
    idx, z = dev_coder.encode_block(_D(ql, qs), _D(pl, ps), seed)
    assert dev_coder.last_path == "device" and [int(i) for i in idx] == ridx and _same(z.cpu().numpy(), rz)
    cpu = [torch.from_numpy(a) for a in host]
    idx_h, z_h = host_coder.encode_block(_D(cpu[0], cpu[1]), _D(cpu[2], cpu[3]), seed)
    assert host_coder.last_path == "host" and [int(i) for i in idx_h] == ridx and _same(z_h.numpy(), rz)
    dec = dev_coder.decode_block(_D(pl, ps), idx, seed)
    assert dev_coder.last_path == "device" and torch.equal(dec, z)
    dec_h = host_coder.decode_block(_D(cpu[2], cpu[3]), idx_h, seed)
    assert torch.equal(dec_h, z_h) and _same(dec.cpu().numpy(), dec_h.numpy())
    assert _same(dec_h.numpy(), R.decode_block(host[2][0], host[3][0], ridx, seed, S, oracle.tf_random_normal))


@pytest.mark.parametrize("seed", GC_SEEDS, ids=_gc_ids)
def test_ratio_fit_at_the_seed_corners(engine, seed):
    """One update_auxiliary_variance_ratios of two 192-dim rows: the device fit equals its host twin bit for bit (ratios, counts and
    the iterations of every step), as in tests/test_ratio_fit_gpu.py; Omega = 1 gives the fit several steps, each with a seed + j."""
    import test_ratio_fit_host as H
    from test_ratio_fit_gpu import _same_fit
    stats = H.survey_rows(2, 192)
    host, dev = H.new_coder(1.0), H.new_coder(1.0)
    host.update_auxiliary_variance_ratios(*H.dists(stats), seed=seed)
    dev.update_auxiliary_variance_ratios(*H.dists(stats, "cuda"), seed=seed)
    assert host.last_path == "host" and dev.last_path == "device" and len(host.last_fit_iters) >= 3, host.last_fit_iters
    _same_fit(host, dev, SC.seed_id(seed))


def test_the_coders_refuse_what_int64_or_the_bound_cannot_hold(engine):
    import irec
    from irec import _lib
    c = irec.BeamSearchCoder(kl_per_partition=1., n_beams=10, extra_samples=1., block_size=None)
    ql, qs, pl, ps = _cuda(*(a[:1] for a in SC.inputs(64, 1)))
    idx, z = c.encode(_D(ql, qs), _D(pl, ps), seed=SC.SEED_BOUND)
    assert torch.equal(c.decode(_D(pl, ps), idx, seed=SC.SEED_BOUND), z)
    for seed in (2 ** 63, -2 ** 63 - 1):
        with pytest.raises(ValueError, match="seed %d is out of range" % seed):
            c.encode(_D(ql, qs), _D(pl, ps), seed=seed)
        with pytest.raises(ValueError, match="seed %d is out of range" % seed):
            c.decode(_D(pl, ps), idx, seed=seed)
    with pytest.raises(_lib.IrecLibraryError, match="IREC_SEED_MAX"):
        c.encode(_D(ql, qs), _D(pl, ps), seed=SC.SEED_BOUND + 1)
    with pytest.raises(_lib.IrecLibraryError, match="IREC_SEED_MAX"):
        c.decode(_D(pl, ps), idx, seed=SC.SEED_BOUND + 1)


# ==== files: compress -> .rec / .recs -> decompress ===================================================================================
HW = 64


@functools.lru_cache(maxsize=None)
def _lossy_setup():
    from test_quality_gpu import _lossy
    model, sampler, _, harness = _lossy()
    torch.manual_seed(11)
    return model, sampler, (torch.rand(2, 3, HW, HW) - 0.5).cuda(), harness


@functools.lru_cache(maxsize=None)
def _rvae_setup():
    from test_models_shim import _model
    model = _model("cuda")
    torch.manual_seed(12)
    return model, (torch.rand(2, 3, HW, HW) - 0.5).cuda()


def _files(blob, off):
    blob = blob.cpu().numpy() if hasattr(blob, "cpu") else np.asarray(blob)
    off = off.cpu().numpy() if hasattr(off, "cpu") else np.asarray(off)
    return [blob[int(off[i]):int(off[i + 1])].tobytes() for i in range(len(off) - 1)]


def _header_seeds(blob, off, segmented):
    from irec.io import rec_header_words, segmented_header_words
    read = segmented_header_words if segmented else rec_header_words
    return [read(f)["seed"] for f in _files(blob, off)]


@pytest.mark.parametrize("seed", SC.HEADER_GOOD, ids=[SC.seed_id(s) for s in SC.HEADER_GOOD])
def test_lossy_model_files_round_trip(engine, seed):
    """Large2LevelVAE: host and device writers, plain and segmented; one image a call, so that compress and decompress run the same
    convolution shapes and their pixels are equal exactly (a batch may change convolution bits: tests/test_lossy_packed_gpu.py)."""
    model, sampler, images, _ = _lossy_setup()
    image = images[:1]
    shape = tuple(image.shape)
    seen = {}
    for on_device in (False, True):
        for g in (None, 1):
            blob, off, recon = model.compress_rec(image, seed, sampler, rec_on_device=on_device, segment_blocks=g)
            assert _header_seeds(blob, off, g is not None) == [seed]
            back = model.decompress_rec(blob, off, seed, shape, sampler, rec_on_device=on_device, segment_blocks=g)
            print(f"lossy seed {SC.seed_id(seed)} device {on_device} segments {g}: max |decompress - compress| = {float((back - recon).abs().max())}")
            assert torch.equal(back, recon), (on_device, g)
            seen.setdefault(g, []).append(_files(blob, off))
            # a reader given another seed -- the file's plus 2^32 included, whose low word is the header's -- refuses the file
            for other in (seed - 1, seed + 2 ** 32):
                _, status = model.decompress_rec(blob, off, other, shape, sampler, rec_on_device=on_device, segment_blocks=g, strict=False)
                assert status.tolist() != [0], (other, on_device, g)
    assert all(a == b for a, b in seen.values())                # host and device wrote the same bytes


@pytest.mark.parametrize("seed", SC.HEADER_GOOD, ids=[SC.seed_id(s) for s in SC.HEADER_GOOD])
def test_resnet_model_files_round_trip(engine, seed):
    """BidirectionalResNetVAE: the device writer, plain and segmented, and the host writer over compress_packed's rows; one image a
    call (see above: tests/test_decompress_device_gpu.py bounds a batch's gap by 1e-5, and one image is exact)."""
    from irec.io import encode_files
    model, images = _rvae_setup()
    image = images[:1]
    shape = tuple(image.shape)
    blob, off, recon = model.compress_rec(image, seed=seed)
    assert _header_seeds(blob, off, False) == [seed]
    back = model.decompress_rec(blob, off, seed, shape)
    print(f"resnet seed {SC.seed_id(seed)}: max |decompress - compress| = {float((back - recon).abs().max())}")
    assert torch.equal(back, recon)
    for other in (seed - 1, seed + 2 ** 32):
        _, status = model.decompress_rec(blob, off, other, shape, strict=False)
        assert status.tolist() != [0], other
    blob_s, off_s, recon_s = model.compress_rec(image, seed=seed, segment_blocks=2)
    assert _header_seeds(blob_s, off_s, True) == [seed] and torch.equal(recon_s, recon)
    assert torch.equal(model.decompress_rec_segmented(blob_s, off_s, seed, shape), recon)
    K, idx, recon_p = model.compress_packed(image, seed=seed)
    coder = model.residual_blocks[0].coder
    blob_h, off_h = encode_files(seed, (HW, HW, 3), coder.block_size, K, idx, max_index=coder.n_samples)
    assert _files(blob_h, off_h) == _files(blob, off) and torch.equal(recon_p, recon)
    assert torch.equal(model.decompress_rec(torch.from_numpy(np.array(blob_h)).cuda(), off_h, seed, shape), recon)


def _no_coding(monkeypatch):
    """Any coder launch from here on fails the test: a refused seed must be refused before anything is coded."""
    from irec.engine import Engine

    def launched(*a, **k):
        raise AssertionError("a coder was launched under a seed no header holds")
    for name in ("encode_blocks", "encode_blocks_margins", "gc_encode_blocks", "decode_blocks"):
        monkeypatch.setattr(Engine, name, launched)


@pytest.mark.parametrize("seed", SC.HEADER_BAD, ids=_bad_ids)
def test_models_and_drivers_refuse_a_seed_no_header_holds(engine, tmp_path, monkeypatch, seed):
    model, sampler, images, harness = _lossy_setup()
    rvae, rimages = _rvae_setup()
    _no_coding(monkeypatch)
    match = r"seed %d .*\[0, 2\^32\)" % seed
    for on_device in (False, True):
        for g in (None, 1):
            with pytest.raises(ValueError, match=match):
                model.compress_rec(images, seed, sampler, rec_on_device=on_device, segment_blocks=g)
    path = str(tmp_path / "one.rec")
    with pytest.raises(ValueError, match=match):
        model.compress(path, images[0].permute(1, 2, 0).contiguous(), seed=seed, sampler=sampler, block_size=100, max_index=sampler.n_samples)
    assert not os.path.exists(path)
    for g in (None, 2):
        with pytest.raises(ValueError, match=match):
            rvae.compress_rec(rimages, seed=seed, segment_blocks=g)
    with pytest.raises(ValueError, match=match):
        rvae.compress_lossless(((rimages + 0.5) * 255).to(torch.uint8), seed=seed)
    names = ["a", "b"]
    out = tmp_path / "out"
    for kw in ({}, {"rec_on_device": True}, {"segment_blocks": 1}):
        with pytest.raises(ValueError, match=match):
            harness.compress_images_lossy(model, sampler, images, names, seed, 100, str(out), **kw)
    for kw in ({}, {"packed": False}, {"rec_on_device": True}):
        with pytest.raises(ValueError, match=match):
            harness.compress_images(rvae, rimages, names, seed, 1000, str(out), **kw)
    with pytest.raises(ValueError, match=match):
        harness.compress_images(rvae, ((rimages + 0.5) * 255).to(torch.uint8), names, seed, 1000, str(out), lossless=True)
    assert not out.exists() and os.listdir(tmp_path) == []


@pytest.mark.parametrize("seed", SC.HEADER_BAD, ids=_bad_ids)
def test_device_writers_refuse_a_seed_no_header_holds(engine, seed):
    """The device entry points irec_rec_encode_files_device* take a uint32 and cannot see a wrapped value: their guard is
    irec.io.header_seed, in the one launch function every device writer goes through.  The caller's buffer stays as it was."""
    from irec import io as IO
    rng = np.random.default_rng(5)
    bpr = (3, 2)
    K = torch.from_numpy(rng.integers(1, 5, (2, 5)).astype(np.int32)).cuda()
    idx = torch.from_numpy(rng.integers(0, 20, (2, 5, 4)).astype(np.int32)).cuda()
    K3, idx4 = K[:, :4].reshape(2, 2, 2).contiguous(), idx[:, :4].reshape(2, 2, 2, 4).contiguous()
    tables = IO.SymbolTables(np.ones(21, dtype=np.int64), None)
    out = torch.full((4096,), 0xAB, dtype=torch.uint8, device="cuda")
    shape = (32, 48, 3)
    calls = {
        "encode_files_device": lambda s: IO.encode_files_device(s, shape, 1000, K3, idx4, 20, out=out),
        "encode_files_device_tables": lambda s: IO.encode_files_device(s, shape, 1000, K3, idx4, 20, out=out, tables=tables),
        "encode_files_device_ragged": lambda s: IO.encode_files_device_ragged(s, shape, 1000, K, idx, 20, bpr, out=out),
        "encode_files_device_ragged_tables": lambda s: IO.encode_files_device_ragged(s, shape, 1000, K, idx, 20, bpr, out=out, tables=tables),
        "encode_files_device_segmented": lambda s: IO.encode_files_device_segmented(s, shape, 1000, K, idx, 20, bpr, 2, out=out),
    }
    for name, call in calls.items():
        with pytest.raises(ValueError, match=r"seed %d .*\[0, 2\^32\)" % seed):
            call(seed)
        assert bool((out == 0xAB).all()), name
    if seed == SC.HEADER_BAD[0]:                     # (once: the calls themselves are valid ones, and the last header seed reads back)
        for name, call in calls.items():
            blob, off = call(2 ** 32 - 1)
            assert _header_seeds(blob, off, name.endswith("segmented")) == [2 ** 32 - 1] * 2, name
            out.fill_(0xAB)
