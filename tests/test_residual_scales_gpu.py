"""One likelihood scale per channel, on the device: the version-2 .res writer and reader against the host forms byte for byte and
status for status (the shapes and the damaged files of tests/residual_scales_cases.py), scale_bits_device against scale_bits, both
device calls once inside the canary arena of tests/guarded.py, and the fit through the model and the harness."""
import numpy as np
import pytest
import torch

import guarded as G
import residual_cases as RC
import residual_scales_cases as SC

pytestmark = pytest.mark.gpu

SEED = 42
CASES = SC.make_cases()
U8, I32, I64 = torch.uint8, torch.int32, torch.int64


@pytest.fixture(scope="module")
def res(engine):
    from irec.io import residual
    return residual


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


# ---- the version-2 container ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_device_writer_and_reader_equal_the_host_forms(res, name):
    pixels, loc, scales, L = CASES[name]
    blob_h, off_h = res.encode_residuals(pixels, loc, scales, stream_len=L)
    for s in (scales, _dev(scales)):                                 # host scales are uploaded; a CUDA tensor is read where it is
        blob, off = res.encode_residuals_device(_dev(pixels), _dev(loc), s, stream_len=L)
        assert np.array_equal(off.cpu().numpy(), off_h) and np.array_equal(blob.cpu().numpy(), blob_h)
    back = res.decode_residuals_device(blob, off, _dev(loc), _dev(scales))                    # stream_len from the header
    assert back.dtype == torch.uint8 and np.array_equal(back.cpu().numpy(), pixels)
    # a short buffer costs a second run and gives the same bytes
    blob2, off2 = res.encode_residuals_device(_dev(pixels), _dev(loc), scales, stream_len=L, out=torch.empty(5, dtype=U8, device="cuda"))
    assert torch.equal(blob2, blob) and torch.equal(off2, off)


@pytest.mark.parametrize("name", list(CASES))
def test_device_reader_answers_damage_as_the_host_reader(res, name):
    pixels, loc, scales, L = CASES[name]
    files = SC.split(*res.encode_residuals(pixels, loc, scales, stream_len=L))
    v1 = SC.split(*res.encode_residuals(pixels, loc, float(scales[0]), stream_len=L))
    sets = [(label, damaged, loc) for label, damaged, _ in SC.damaged_sets(files, v1, pixels.shape[1:], L, scales)]
    sets.append(("another_loc", files, SC.another_loc(loc)))
    stream_byte = bytearray(files[1])
    stream_byte[-1] ^= 0x10
    sets.append(("stream_byte", [files[0], bytes(stream_byte)] + files[2:], loc))
    loc_d = {}
    for label, damaged, lc in sets:
        blob, off = SC.join(damaged)
        want, want_status = res.decode_residuals(blob, off, lc, scales, stream_len=L, strict=False)
        got, status = res.decode_residuals_device(_dev(blob), off, loc_d.setdefault(id(lc), _dev(lc)), _dev(scales), stream_len=L, strict=False)
        assert status.tolist() == want_status.tolist(), (label, status, want_status)
        assert not want_status[0], label
        if label == "another_loc":          # (under the wide last scale of the one- and four-channel cases the same pixel may decode)
            assert want_status[1] == RC.E_CHECKSUM or name not in ("cross_3x5x7_L16", "wide_3x80x81_L64"), want_status
        elif label != "stream_byte":        # (a padding bit carries nothing)
            assert want_status[1] != 0, label
        assert np.array_equal(got.cpu().numpy(), want), label
    # a version-2 file under the version-1 device reader
    blob, off = SC.join([v1[0], files[1]] + v1[2:])
    got, status = res.decode_residuals_device(_dev(blob), off, _dev(loc), float(scales[0]), stream_len=L, strict=False)
    assert status.tolist() == [RC.E_MAGIC if i == 1 else 0 for i in range(len(files))]
    assert np.array_equal(got.cpu().numpy()[0], pixels[0]) and not got[1].any()


def test_a_bad_scale_in_one_channel_on_the_device(res):
    pixels, loc, scales, L = CASES["cross_3x5x7_L16"]
    bad = scales.copy()
    bad[2] = np.nan
    with pytest.raises(ValueError, match=r"likelihood scale.*\(image 0\)"):
        res.encode_residuals_device(_dev(pixels), _dev(loc), _dev(bad), stream_len=L)
    blob, off = res.encode_residuals(pixels, loc, scales, stream_len=L)
    got, status = res.decode_residuals_device(_dev(blob), off, _dev(loc), _dev(bad), stream_len=L, strict=False)
    assert status.tolist() == [RC.E_SCALE_WORD] * 3 and not got.any()


# ---- scale_bits -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bits_case():
    pixels, loc, _ = SC.make(SC.BITS_SHAPE[0], SC.BITS_SHAPE[1:], 77)
    loc = loc.copy()
    loc[1, 1, 60, 3] = np.nan                                       # one pixel left out, in a second tile
    return pixels, loc


@pytest.mark.parametrize("n_cand", [1, 2, 64])
def test_scale_bits_device_equals_the_host_form(res, bits_case, n_cand):
    pixels, loc = bits_case
    scales = SC.candidates(3, n_cand)
    if n_cand > 1:
        scales[2, 1] = 0.0                                          # a refused candidate: INT64_MAX
    want, want_skipped = res.scale_bits(pixels, loc, scales)
    bits, skipped = res.scale_bits_device(_dev(pixels), _dev(loc), _dev(scales))
    assert bits.dtype == torch.int64 and tuple(bits.shape) == want.shape
    assert np.array_equal(bits.cpu().numpy(), want) and int(skipped.sum()) == want_skipped == 1
    assert n_cand == 1 or (want[:, 2, 1] == SC.INT64_MAX).all()
    one, _ = res.scale_bits_device(_dev(pixels[1:]), _dev(loc[1:]), scales)                   # a row alone; host candidates
    assert np.array_equal(one.cpu().numpy()[0], want[1])


@pytest.mark.parametrize("name", list(CASES))
def test_scale_bits_device_on_the_container_shapes(res, name):
    pixels, loc, scales, _ = CASES[name]
    cand = np.stack([scales, scales[::-1]], axis=1)
    want, _ = res.scale_bits(pixels, loc, cand)
    bits, skipped = res.scale_bits_device(_dev(pixels), _dev(loc), cand)
    assert np.array_equal(bits.cpu().numpy(), want) and not skipped.any()


def test_scale_bits_device_with_no_images(res):
    bits, skipped = res.scale_bits_device(torch.zeros((0, 3, 4, 4), dtype=U8, device="cuda"), torch.zeros((0, 3, 4, 4), device="cuda"),
                                          np.float32([0.05, 0.1]))
    assert tuple(bits.shape) == (0, 3, 2) and tuple(skipped.shape) == (0, 3)


def test_model_bits_on_the_device(res, bits_case):
    pixels, loc = bits_case
    loc = np.nan_to_num(loc, nan=0.0)
    scales = np.float32([0.02, 0.05, 0.11])
    for s in (0.05, scales, _dev(scales)):
        got = res.residual_model_bits_device(_dev(pixels), _dev(loc), s)
        assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (2,)
        want = res.residual_model_bits(pixels, loc, s.cpu().numpy() if hasattr(s, "cpu") else s)
        assert (np.abs(got.cpu().numpy() - want) <= pixels[0].size * 2.0 ** -17).all()


def test_fit_scales_on_the_device_is_the_host_fit(res):
    pixels, loc = SC.logistic_images(n=4, size=16)
    host = res.fit_scales([(pixels[:3], loc[:3]), (pixels[3:], loc[3:])], per_channel=True, start=0.0)
    dev = res.fit_scales([(_dev(pixels[:3]), _dev(loc[:3])), (_dev(pixels[3:]), _dev(loc[3:]))], per_channel=True, start=0.0)
    assert np.array_equal(host[0], dev[0]) and np.array_equal(host[1], dev[1]) and host[2]["channels"] == dev[2]["channels"]


# ---- the memory contract --------------------------------------------------------------------------------------------------------------
def test_device_calls_in_the_arena(engine, res):
    """Both new device paths once inside the canary arena: outputs pre-filled, a workspace of exactly the sized bytes filled with
    0xFF, inputs compared as bytes afterwards."""
    from irec import _lib
    lib = engine.lib
    stream = engine._stream()
    pixels, loc, scales, L = CASES["cross_3x5x7_L16"]
    n, ch, h, w = pixels.shape
    ns = -(-(ch * h * w) // L)
    blob_h, off_h = res.encode_residuals(pixels, loc, scales, stream_len=L)
    total = int(off_h[-1])
    need = lib.irec_res_device_workspace_bytes(n, ns)
    arena = G.Arena(G.slack(20) + 2 * need + 16 * pixels.size + 2 * total + 64 * (n + 1) + 64, "cuda")
    px, lc, sc = arena.put(pixels, name="pixels"), arena.put(loc, name="loc"), arena.put(scales, name="scales")
    out = arena.region(U8, (total,), "out", name="out")
    offsets = arena.region(I64, (n + 1,), "out", name="offsets")
    status = arena.region(I32, (n,), "out", name="status")
    ws = arena.workspace(need, 0xFFFFFFFF)
    arena.arm()
    _lib.check(lib.irec_res_encode_files_device_scales(px.data_ptr(), lc.data_ptr(), sc.data_ptr(), n, h, w, ch, L, out.data_ptr(), total,
                                                       offsets.data_ptr(), status.data_ptr(), ws.data_ptr(), need, stream),
               "irec_res_encode_files_device_scales")
    torch.cuda.synchronize()
    arena.check()
    assert not status.any() and np.array_equal(offsets.cpu().numpy(), off_h) and np.array_equal(out.cpu().numpy(), blob_h[:total])
    blob, off = arena.put(np.ascontiguousarray(blob_h[:total]), name="bytes"), arena.put(np.ascontiguousarray(off_h, dtype=np.int64), name="offsets (in)")
    back = arena.region(U8, tuple(pixels.shape), "out", name="pixels (decoded)")
    st2 = arena.region(I32, (n,), "out", name="status (decoded)")
    ws2 = arena.workspace(need, 0xFFFFFFFF, name="workspace (decode)")
    arena.arm()
    _lib.check(lib.irec_res_decode_files_device_scales(blob.data_ptr(), off.data_ptr(), lc.data_ptr(), sc.data_ptr(), n, h, w, ch, L,
                                                       back.data_ptr(), st2.data_ptr(), ws2.data_ptr(), need, stream),
               "irec_res_decode_files_device_scales")
    torch.cuda.synchronize()
    arena.check()
    assert not st2.any() and np.array_equal(back.cpu().numpy(), pixels)
    # a buffer one byte short: offsets and status are written, the buffer is not
    arena2 = G.Arena(G.slack(12) + need + 16 * pixels.size + total + 64 * (n + 1) + 64, "cuda")
    px, lc, sc = arena2.put(pixels, name="pixels"), arena2.put(loc, name="loc"), arena2.put(scales, name="scales")
    out = arena2.region(U8, (total - 1,), "out", name="out")
    offsets = arena2.region(I64, (n + 1,), "out", name="offsets")
    status = arena2.region(I32, (n,), "out", name="status")
    ws = arena2.workspace(need, 0xFFFFFFFF)
    arena2.arm()
    _lib.check(lib.irec_res_encode_files_device_scales(px.data_ptr(), lc.data_ptr(), sc.data_ptr(), n, h, w, ch, L, out.data_ptr(), total - 1,
                                                       offsets.data_ptr(), status.data_ptr(), ws.data_ptr(), need, stream),
               "irec_res_encode_files_device_scales")
    torch.cuda.synchronize()
    arena2.check()
    assert (out == G.PREFILL_U8).all() and np.array_equal(offsets.cpu().numpy(), off_h) and not status.any()


def test_scale_bits_device_in_the_arena(engine, res, bits_case):
    from irec import _lib
    lib = engine.lib
    pixels, loc = bits_case
    n, ch, h, w = pixels.shape
    n_cand = 5
    scales = SC.candidates(ch, n_cand)
    scales[0, 3] = np.inf
    want, want_skipped = res.scale_bits(pixels, loc, scales)
    need = lib.irec_res_scale_bits_workspace_bytes(n, h, w, ch, n_cand)
    assert need >= 8 * n * ch * 2 * (n_cand + 1)
    cost = res.cost_table()
    arena = G.Arena(G.slack(12) + need + 8 * pixels.size + cost.nbytes + 16 * want.size + 4096, "cuda")
    px, lc = arena.put(pixels, name="pixels"), arena.put(loc, name="loc")
    sc, ct = arena.put(scales, name="scales"), arena.put(cost, name="cost")
    bits = arena.region(I64, want.shape, "out", name="bits")
    skipped = arena.region(I64, (n, ch), "out", name="skipped")
    ws = arena.workspace(need, 0xFFFFFFFF)
    arena.arm()
    _lib.check(lib.irec_res_scale_bits_device(px.data_ptr(), lc.data_ptr(), sc.data_ptr(), ct.data_ptr(), n, h, w, ch, n_cand, bits.data_ptr(),
                                              skipped.data_ptr(), ws.data_ptr(), need, engine._stream()), "irec_res_scale_bits_device")
    torch.cuda.synchronize()
    arena.check()
    assert np.array_equal(bits.cpu().numpy(), want) and int(skipped.sum()) == want_skipped
    # a workspace one byte short is refused before any launch
    assert lib.irec_res_scale_bits_device(px.data_ptr(), lc.data_ptr(), sc.data_ptr(), ct.data_ptr(), n, h, w, ch, n_cand, bits.data_ptr(),
                                          skipped.data_ptr(), ws.data_ptr(), need - 1, engine._stream()) != 0


# ---- the model and the harness ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lossless(engine):
    import test_lossless_model_gpu as T
    return T


@pytest.fixture(scope="module")
def images(lossless):
    return lossless._images(4, seed=21)


@pytest.fixture(scope="module")
def fitted(engine, lossless, images):
    """(the model fitted per channel, the model bits of `images` before the fit, fit_likelihood_scale's return)."""
    from irec.io import residual
    m = lossless._model()
    recon = m.compress_lossless(images, SEED)[4]
    before = residual.residual_model_bits_device(images, recon, m.residual_scale()).sum().item()
    result = m.fit_likelihood_scale(images, SEED, per_channel=True)
    return m, before, result


def test_unfitted_model_keeps_its_state_dict_keys(lossless):
    m = lossless._model()
    keys = list(m.state_dict())
    assert "likelihood_log_scale" in keys and not [k for k in keys if "likelihood_log_scales" in k]
    assert m.likelihood_log_scales is None and isinstance(m.residual_scale(), float)
    m.set_likelihood_scales([-1.0, -2.0, -3.0])
    assert set(m.state_dict()) == set(keys) | {"likelihood_log_scales"}
    m.set_likelihood_scales(None)
    assert list(m.state_dict()) == keys


def test_per_channel_fit_round_trips_in_version_2_and_costs_no_more(res, fitted, images):
    m, before, (log_scales, bits, _) = fitted
    assert m.likelihood_log_scales is not None and tuple(m.likelihood_log_scales.shape) == (3,) and m.likelihood_log_scales.dtype == torch.float32
    assert np.allclose(m.likelihood_log_scales.cpu().numpy(), log_scales)
    rec_blob, rec_off, res_blob, res_off, recon = m.compress_lossless(images, SEED)
    for i in range(images.shape[0]):
        assert res.version_of(res_blob[int(res_off[i]):int(res_off[i + 1])].cpu().numpy()) == 2
    out = m.decompress_lossless(rec_blob, rec_off, res_blob, res_off, SEED, images.shape)
    assert out.dtype == torch.uint8 and torch.equal(out, images)
    after = res.residual_model_bits_device(images, recon, m.residual_scale()).sum().item()
    print("model bits before", before, "after", after, "fitted log-scales", log_scales)
    assert after <= before
    assert abs(after - int(bits.sum()) / 65536.0) < 1e-6                                        # the fit's own figure
    # without the scales the files are refused, image by image
    plain = m.likelihood_log_scales.clone()
    m.set_likelihood_scales(None)
    _, status = m.decompress_lossless(rec_blob, rec_off, res_blob, res_off, SEED, images.shape, strict=False)
    m.set_likelihood_scales(plain)
    from irec.models.resnet_vae import STATUS_RESIDUAL
    assert status.tolist() == [STATUS_RESIDUAL + RC.E_MAGIC] * images.shape[0]


def test_single_scale_fit_still_writes_version_1(res, lossless, images):
    m = lossless._model()
    recon = m.compress_lossless(images, SEED)[4]
    before = res.residual_model_bits_device(images, recon, m.residual_scale()).sum().item()
    log_scale, bits, ev = m.fit_likelihood_scale(images, SEED)
    assert m.likelihood_log_scales is None and abs(float(m.likelihood_log_scale.detach()) - log_scale) < 1e-6
    assert bits <= dict(ev["single"])[0.0]                                                     # the scale it had was a candidate
    rec_blob, rec_off, res_blob, res_off, recon = m.compress_lossless(images, SEED)
    assert res.version_of(res_blob[:int(res_off[1])].cpu().numpy()) == 1
    assert res.residual_model_bits_device(images, recon, m.residual_scale()).sum().item() <= before
    # the unfitted reader path: a model that was only told the scalar
    other = lossless._model()
    with torch.no_grad():
        other.likelihood_log_scale.fill_(log_scale)
    assert torch.equal(other.decompress_lossless(rec_blob, rec_off, res_blob, res_off, SEED, images.shape), images)
    want_blob, want_off = res.encode_residuals_device(images, recon, m.likelihood_scale())
    assert torch.equal(res_blob, want_blob) and torch.equal(res_off, want_off)


def test_harness_round_trip_with_a_per_channel_model(lossless, images, tmp_path):
    from irec import harness
    m = lossless._model()
    log_scales, bits = harness.fit_likelihood_scale(m, images, SEED, per_channel=True, batch=3)       # batches of 3 and 1
    assert log_scales.shape == (3,) and bits.shape == (3,) and m.likelihood_log_scales is not None
    names = [f"im{i}" for i in range(images.shape[0])]
    rows = harness.compress_images(m, images, names, SEED, 1000, str(tmp_path), lossless=True)
    for i, row in enumerate(rows):
        assert row["pixels_recovered"] and row["indices_recovered"]
        assert row["residual_model_bits"] <= row["comp_residual"]
        assert open(tmp_path / f"im{i}.res", "rb").read(6)[4:6] == b"\x02\x00"
    out, drows = harness.decompress_images_lossless(m, [str(tmp_path / f"{nm}.rec") for nm in names])
    assert out.dtype == torch.uint8 and torch.equal(out, images) and all(r["status"] == 0 for r in drows)
