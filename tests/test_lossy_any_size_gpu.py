"""GPU tests of the lossy drivers over images of any size (harness.compress_images_lossy(resize=True) / decompress_images_lossy), for
both lossy models: five images of sizes 65 x 67, 64 x 64, 130 x 201, 127 x 64 and 64 x 64 (float32 and uint8 among them) are brought
to 64 x 64, 64 x 64, 128 x 192, 64 x 64, 64 x 64 by irec.image.resize_bilinear, coded in two groups, and come back in the order given."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEED, BLOCK = 42, 5
SIZES = [(65, 67), (64, 64), (130, 201), (127, 64), (64, 64)]
CODED = [(64, 64), (64, 64), (128, 192), (64, 64), (64, 64)]
NAMES = ["a", "b", "c", "d", "e"]
BATCH_TOL = 1e-5                                   # (a batch against an image alone: tests/test_lossy_packed_gpu.py's bound)


def _sampler():
    import irec
    return irec.BeamSearchCoder(kl_per_partition=3., n_beams=10, extra_samples=1., block_size=BLOCK)


@functools.lru_cache(maxsize=None)
def _model(levels):
    from irec.models import Large1LevelVAE, Large2LevelVAE
    torch.manual_seed(3)
    with torch.no_grad():                         # the heads of the posteriors' locs scaled: K above 1
        if levels == 1:
            m = Large1LevelVAE(num_filters=8).cuda().eval()
            m.analysis_transform[-1].weight[:8].mul_(16.)
            m.analysis_transform[-1].bias[:8].mul_(16.)
        else:
            m = Large2LevelVAE(level_1_filters=8, level_2_filters=4).cuda().eval()
            for mod in (m.hyper_analysis_transform[-1], m._level_1_posterior_loc_combiner):
                mod.weight.mul_(16.)
                mod.bias.mul_(16.)
    return m


@functools.lru_cache(maxsize=None)
def _images():
    """The five images in [0, 1]: the second and the fourth as uint8."""
    g = torch.Generator().manual_seed(11)
    out = []
    for i, (h, w) in enumerate(SIZES):
        x = torch.rand(3, h, w, generator=g)
        out.append(((x * 255).round().to(torch.uint8) if i in (1, 3) else x).cuda())
    return out


@functools.lru_cache(maxsize=None)
def _alone(levels):
    """Per image, alone: the resized image, and the file and the reconstruction model.compress gives for it.  Computed once."""
    import tempfile
    from irec import image
    m, sampler = _model(levels), _sampler()
    resized, files, recons = [], [], []
    with tempfile.TemporaryDirectory() as tmp:
        for i, (x, size) in enumerate(zip(_images(), CODED)):
            r = image.resize_bilinear(x[None], size)[0]
            path = f"{tmp}/{i}.rec"
            recons.append(m.compress(path, r.permute(1, 2, 0).contiguous(), seed=SEED, sampler=sampler, block_size=BLOCK, max_index=m._max_index(sampler))[0])
            resized.append(r)
            files.append(open(path, "rb").read())
    return resized, files, recons


@pytest.mark.parametrize("levels", [1, 2], ids=["one_level", "two_level"])
def test_five_sizes_round_trip(engine, levels, tmp_path):
    from irec import harness, image, metrics
    m, sampler = _model(levels), _sampler()
    resized, files, recons = _alone(levels)
    assert [tuple(r.shape[1:]) for r in resized] == CODED and [image.driver_size(h, w) for h, w in SIZES] == CODED
    rows = harness.compress_images_lossy(m, sampler, _images(), NAMES, SEED, BLOCK, str(tmp_path), resize=True, quality=True)
    assert [r["name"] for r in rows] == NAMES and all(r["indices_recovered"] is True for r in rows)
    assert [(r["orig_h"], r["orig_w"], r["h"], r["w"]) for r in rows] == [(*a, *b) for a, b in zip(SIZES, CODED)]
    paths = [str(tmp_path / f"{nm}.rec") for nm in NAMES]
    assert [open(p, "rb").read() for p in paths] == files
    pixels, drows = harness.decompress_images_lossy(m, sampler, paths)
    assert isinstance(pixels, list) and [tuple(p.shape) for p in pixels] == [(3, *s) for s in CODED] and all(r["status"] == 0 for r in drows)
    for i, row in enumerate(rows):
        err = float((pixels[i] - recons[i]).abs().max())
        psnr = float(metrics.psnr(pixels[i][None], resized[i][None], **metrics.transform_for((0., 1.)))[0])
        print(f"{levels} level(s), image {i}: max |decoded - alone| = {err:.3g}, psnr row {row['psnr']:.6f} / decoded vs resized {psnr:.6f}")
        assert err <= BATCH_TOL
        assert row["comp_lossy_bpp"] == 8 * len(files[i]) / (CODED[i][0] * CODED[i][1]) and row["kld"] > 0
        assert np.isnan(row["ms_ssim"])                                     # (below 161 on a side: no five-scale MS-SSIM)
    # psnr: metrics.psnr of the batch's own reconstruction against the resized images, exactly
    groups = {}
    for i, size in enumerate(CODED):
        groups.setdefault(size, []).append(i)
    for members in groups.values():
        chunk = torch.stack([resized[i] for i in members])
        _, _, recon = m.compress_rec(chunk, SEED, sampler)
        want = metrics.psnr(recon, chunk, **metrics.transform_for((0., 1.))).cpu().numpy()
        assert [rows[i]["psnr"] for i in members] == [float(v) for v in want]
    # the decoded images are the reconstructions the compress side measured
    for members in groups.values():
        chunk = torch.stack([resized[i] for i in members])
        assert torch.equal(torch.stack([pixels[i] for i in members]), m.compress_rec(chunk, SEED, sampler)[2])


@pytest.mark.parametrize("levels", [1, 2], ids=["one_level", "two_level"])
def test_a_list_of_other_sizes_without_resize_is_refused_before_any_file(engine, levels, tmp_path):
    from irec import harness
    out = tmp_path / "never"
    with pytest.raises(ValueError, match="multiples of 64"):
        harness.compress_images_lossy(_model(levels), _sampler(), _images(), NAMES, SEED, BLOCK, str(out))
    assert not os.path.exists(out)
    with pytest.raises(ValueError, match="driver_size"):
        harness.compress_images_lossy(_model(levels), _sampler(), [torch.zeros(3, 63, 80).cuda()], ["x"], SEED, BLOCK, str(out), resize=True)
    assert not os.path.exists(out)


@pytest.mark.parametrize("levels", [1, 2], ids=["one_level", "two_level"])
def test_the_four_d_call_is_what_it_was(engine, levels, tmp_path):
    """One 4-D tensor, resize=False: the rows' keys are compress_images', the files compress_rec's on the same tensor."""
    from irec import harness
    m, sampler = _model(levels), _sampler()
    torch.manual_seed(5)
    images = (torch.rand(3, 3, 64, 128) - 0.5).cuda()
    names = ["p", "q", "r"]
    rows = harness.compress_images_lossy(m, sampler, images, names, SEED, BLOCK, str(tmp_path))
    (blob, off, _), (K, _, _) = m.compress_rec(images, SEED, sampler, block_size=BLOCK, return_pendings=True)
    assert [r["name"] for r in rows] == names
    assert all(set(r) == {"name", "comp_codelength", "comp_lossy_bpp", "comp_code_bpd", "code_nats", "n_indices", "indices_recovered", "comp_time"}
               for r in rows)
    assert [open(tmp_path / f"{nm}.rec", "rb").read() for nm in names] == [blob[off[i]:off[i + 1]].tobytes() for i in range(3)]
    assert [r["n_indices"] for r in rows] == K.sum(axis=1).tolist() and [r["comp_codelength"] for r in rows] == (8 * np.diff(off)).tolist()
    # the same images as a list of multiples of 64: the same files, the size keys added
    rows_l = harness.compress_images_lossy(m, sampler, list(images), names, SEED, BLOCK, str(tmp_path / "list"))
    assert [open(tmp_path / "list" / f"{nm}.rec", "rb").read() for nm in names] == [blob[off[i]:off[i + 1]].tobytes() for i in range(3)]
    assert all((r["orig_h"], r["orig_w"], r["h"], r["w"]) == (64, 128, 64, 128) for r in rows_l)
