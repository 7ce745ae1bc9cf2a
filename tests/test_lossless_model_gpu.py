"""The lossless pair through the model and the harness: compress_lossless -> decompress_lossless gives the uint8 images back exactly,
the .rec files are compress_rec's, damage is a status per image in first-cause order, and harness.compress_images(lossless=True)
reports the reference's code + residual figures from bits that were written."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEED = 42


def _model(blocks=2):
    """tests/test_decompress_device_gpu.py's model with two residual blocks: 16 x 16 images give 512-dim latents, one coder block."""
    from irec.models import BidirectionalResNetVAE
    torch.manual_seed(0)
    m = BidirectionalResNetVAE(num_res_blocks=blocks, sampler="beam_search", sampler_args={"n_beams": 20, "extra_samples": 1.2},
                               coder_args={"block_size": 1000}, deterministic_filters=16, stochastic_filters=8, kl_per_partition=3.)
    with torch.no_grad():
        for b in m.residual_blocks:
            for head in (b.gen_posterior_loc_head, b.gen_posterior_log_scale_head, b.infer_posterior_loc_head,
                         b.infer_posterior_log_scale_head, b.prior_loc_head, b.prior_log_scale_head):
                head.weight.mul_(0.3)
        m._generative_base.normal_(0, 0.5)
    return m.cuda().eval()


def _images(n, seed=1, size=16):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, 3, size, size), generator=g, dtype=torch.uint8).cuda()


@pytest.fixture(scope="module")
def model(engine):
    return _model()


@pytest.fixture(scope="module")
def coded(model):
    """Three images coded once: (images, the five of compress_lossless)."""
    x = _images(3)
    return x, model.compress_lossless(x, SEED)


@pytest.mark.parametrize("n", [1, 3])
def test_round_trip_is_exact(model, n):
    x = _images(n, seed=n)
    rec_blob, rec_off, res_blob, res_off, recon = model.compress_lossless(x, SEED)
    assert recon.shape == x.shape and recon.dtype == torch.float32
    out = model.decompress_lossless(rec_blob, rec_off, res_blob, res_off, SEED, x.shape)
    assert out.dtype == torch.uint8 and torch.equal(out, x)


def test_rec_files_are_compress_recs(model, coded):
    x, (rec_blob, rec_off, _, _, _) = coded
    blob, off, _ = model.compress_rec(x.to(torch.float32) / 256 - 0.5, SEED)
    assert torch.equal(rec_blob, blob) and torch.equal(rec_off, off)


def test_a_sharper_scale_round_trips_and_is_smaller_near_the_reconstruction(model):
    """An image made of its own reconstruction's pixels: at exp(-2) the residual costs less than at exp(0)."""
    x0 = _images(1, seed=7)
    m = _model()
    recon = m.compress_lossless(x0, SEED)[4]
    x = torch.floor((recon + 0.5) * 256).clamp(0, 255).to(torch.uint8)
    sizes = {}
    for log_scale in (0.0, -2.0):
        with torch.no_grad():
            m.likelihood_log_scale.fill_(log_scale)
        rec_blob, rec_off, res_blob, res_off, _ = m.compress_lossless(x, SEED)
        assert torch.equal(m.decompress_lossless(rec_blob, rec_off, res_blob, res_off, SEED, x.shape), x)
        sizes[log_scale] = int(res_off[-1])
    assert abs(m.likelihood_scale() - np.exp(-2.0)) < 1e-7
    assert sizes[-2.0] < sizes[0.0]


def test_damaged_res_is_a_status_for_that_image(model, coded):
    from irec.models.resnet_vae import STATUS_RESIDUAL, status_text
    x, (rec_blob, rec_off, res_blob, res_off, _) = coded
    bad = res_blob.clone()
    bad[int(res_off[1])] ^= 0xFF                                    # the magic word of image 1
    out, status = model.decompress_lossless(rec_blob, rec_off, bad, res_off, SEED, x.shape, strict=False)
    assert status.tolist() == [0, STATUS_RESIDUAL + 4, 0]
    assert torch.equal(out[0], x[0]) and torch.equal(out[2], x[2]) and not out[1].any()
    assert "magic" in status_text(status[1])
    from irec.coding import CodingError
    with pytest.raises(CodingError, match=r"\(image 1\)"):
        model.decompress_lossless(rec_blob, rec_off, bad, res_off, SEED, x.shape)
    # a stream byte: the reader's own cause, or the checksum
    bad = res_blob.clone()
    bad[int(res_off[2]) - 3] ^= 0x40
    out, status = model.decompress_lossless(rec_blob, rec_off, bad, res_off, SEED, x.shape, strict=False)
    assert status[0] == 0 and status[2] == 0 and status[1] in (STATUS_RESIDUAL + 8, STATUS_RESIDUAL + 9)
    assert torch.equal(out[0], x[0]) and torch.equal(out[2], x[2]) and not out[1].any()


def test_damaged_rec_reports_the_rec_cause_first(model, coded):
    x, (rec_blob, rec_off, res_blob, res_off, _) = coded
    bad_rec, bad_res = rec_blob.clone(), res_blob.clone()
    bad_rec[int(rec_off[1]) + 22] = 1                               # .rec: "uses count files" (IREC_REC_E_COUNT_FILES = 5)
    bad_res[int(res_off[1])] ^= 0xFF                                # and its .res damaged too
    out, status = model.decompress_lossless(bad_rec, rec_off, bad_res, res_off, SEED, x.shape, strict=False)
    assert status.tolist() == [0, 5, 0]
    assert torch.equal(out[0], x[0]) and torch.equal(out[2], x[2]) and not out[1].any()
    out, status = model.decompress_lossless(bad_rec, rec_off, res_blob, res_off, SEED, x.shape, strict=False)
    assert status.tolist() == [0, 5, 0] and not out[1].any()       # a whole .res on a refused .rec: zero, not garbage


def test_harness_through_files(model, tmp_path):
    from irec import harness
    x = _images(3, seed=11)
    names = [f"im{i}" for i in range(3)]
    rows = harness.compress_images(model, x, names, SEED, 1000, str(tmp_path), lossless=True)
    for i, row in enumerate(rows):
        rec_bits = os.path.getsize(tmp_path / f"im{i}.rec") * 8
        res_bits = os.path.getsize(tmp_path / f"im{i}.res") * 8
        assert row["pixels_recovered"] and row["indices_recovered"]
        assert row["comp_codelength"] == rec_bits and row["comp_residual"] == res_bits
        assert row["comp_lossless_bpp"] == (rec_bits + res_bits) / (16 * 16) and row["comp_bpd"] == (rec_bits + res_bits) / (16 * 16 * 3)
        assert row["residual_model_bits"] <= res_bits
    out, drows = harness.decompress_images_lossless(model, [str(tmp_path / f"{nm}.rec") for nm in names])
    assert out.dtype == torch.uint8 and torch.equal(out, x) and all(r["status"] == 0 for r in drows)
    # the default rows are untouched by the new argument
    plain = harness.compress_images(model, x.to(torch.float32) / 256 - 0.5, names, SEED, 1000, str(tmp_path / "plain"), rec_on_device=True)
    assert "comp_residual" not in plain[0] and plain[0]["comp_codelength"] == rows[0]["comp_codelength"]
