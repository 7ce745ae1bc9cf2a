"""CPU tests of what harness.compress_images_lossy does with images of any size -- the resize to the driver's size, the groups by coded
size, the batches inside a group, the order of the rows, the passes of ideal=True -- over the stub model of
tests/test_harness_drivers_host.py (constant images carry their number as their value, which a bilinear resize keeps exactly)."""
import os

import numpy as np
import pytest
import torch

import test_harness_drivers_host as D

SIZES = [(65, 67), (64, 64), (130, 201), (127, 64), (64, 64)]
CODED = [(64, 64), (64, 64), (128, 192), (64, 64), (64, 64)]
NAMES = ["a", "b", "c", "d", "e"]


def _images():
    return [torch.full((3, h, w), i / 100) for i, (h, w) in enumerate(SIZES)]


class Recording(D.StubLossy):
    def __init__(self, **kw):
        super().__init__(**kw)
        self.coded, self.passes = [], []

    def compress_rec(self, images, *args, **kw):
        self.coded.append((D.tags(images), tuple(images.shape[2:])))
        z = torch.zeros(images.shape[0], 1)
        self.posterior = self.prior = D.types.SimpleNamespace(loc=z, scale=z + 1)          # a one-level model's distributions: KL 0
        return super().compress_rec(images, *args, **kw)

    def forward(self, tensor, sampling_fn=None, seed=None, image_base=0):
        self.passes.append((D.tags(tensor), image_base))
        self._kl = [torch.ones(tensor.shape[0], dtype=torch.float64)]
        return None, tensor

    def kl_divergence(self):
        return self._kl


@pytest.mark.parametrize("batch,want", [(None, [([0, 1, 3, 4], (64, 64)), ([2], (128, 192))]),
                                        (3, [([0, 1, 3], (64, 64)), ([4], (64, 64)), ([2], (128, 192))])], ids=["whole_groups", "batches_of_3"])
def test_groups_batches_and_order(tmp_path, batch, want):
    from irec import harness, io
    model = Recording()
    rows = harness.compress_images_lossy(model, D.SAMPLER, _images(), NAMES, D.SEED, D.BLOCK, str(tmp_path), batch=batch, resize=True)
    assert model.coded == want
    assert [r["name"] for r in rows] == NAMES
    assert [(r["orig_h"], r["orig_w"], r["h"], r["w"]) for r in rows] == [(*a, *b) for a, b in zip(SIZES, CODED)]
    K, idx = D.canned(sum(D.BPR))
    for i, (row, (h, w)) in enumerate(zip(rows, CODED)):
        assert set(row) == D.KEYS | {"orig_h", "orig_w", "h", "w"} and row["indices_recovered"] is True
        seed, shape, _, blocks = io.read_compressed_code(str(tmp_path / f"{NAMES[i]}.rec"))
        assert (seed, tuple(shape)) == (D.SEED, (h, w, 3)) and blocks == D.lists_of(K[i], idx[i], D.BPR)       # image i's own rows
        assert row["comp_lossy_bpp"] == row["comp_codelength"] / (h * w)


def test_ideal_passes_number_the_images_as_the_call_does(tmp_path):
    from irec import harness
    model = Recording()
    rows = harness.compress_images_lossy(model, D.SAMPLER, _images(), NAMES, D.SEED, D.BLOCK, str(tmp_path), resize=True, ideal=True, quality=True)
    assert model.passes == [([0, 1], 0), ([3, 4], 3), ([2], 2)]
    assert all(r["ideal_kld"] == 1.0 and r["kld"] == 0.0 for r in rows)
    # (every side below 161: no five-scale MS-SSIM; the stub's reconstruction is the image itself)
    assert all(np.isnan(r["ms_ssim"]) and np.isnan(r["ideal_ms_ssim"]) and r["psnr"] == float("inf") for r in rows)


def test_a_refused_batch_is_the_error_rows_of_its_images(tmp_path):
    from irec import harness
    rows = harness.compress_images_lossy(Recording(fail={3}), D.SAMPLER, _images(), NAMES, D.SEED, D.BLOCK, str(tmp_path), batch=2, resize=True)
    assert [r["name"] for r in rows] == NAMES
    assert ["error" in r for r in rows] == [False, False, False, True, True]                 # the batch (3, 4) of the 64 x 64 group
    assert rows[3] == {"name": "d", "error": "cannot code [3]"}
    assert not os.path.exists(tmp_path / "d.rec") and os.path.exists(tmp_path / "c.rec")


def test_without_resize_a_list_wants_multiples_of_64(tmp_path):
    from irec import harness
    out = tmp_path / "never"
    with pytest.raises(ValueError, match="image 0 is 65 x 67"):
        harness.compress_images_lossy(Recording(), D.SAMPLER, _images(), NAMES, D.SEED, D.BLOCK, str(out))
    with pytest.raises(ValueError, match="driver_size"):
        harness.compress_images_lossy(Recording(), D.SAMPLER, [torch.zeros(3, 63, 64)], ["x"], D.SEED, D.BLOCK, str(out), resize=True)
    with pytest.raises(ValueError, match=r"not a \[3, h, w\]"):
        harness.compress_images_lossy(Recording(), D.SAMPLER, [torch.zeros(1, 64, 64)], ["x"], D.SEED, D.BLOCK, str(out), resize=True)
    assert not os.path.exists(out)
    model = Recording()
    rows = harness.compress_images_lossy(model, D.SAMPLER, [_images()[1], torch.full((3, 128, 64), 0.05)], ["b", "f"], D.SEED, D.BLOCK, str(out))
    assert model.coded == [([1], (64, 64)), ([5], (128, 64))] and [(r["h"], r["w"]) for r in rows] == [(64, 64), (128, 64)]


def test_uint8_images_are_converted_by_the_resize():
    from irec import harness
    for resize in (False, True):
        h = 70 if resize else 64
        images = [torch.full((3, 64, 64), 51, dtype=torch.uint8), torch.full((3, h, 64), 0.25), torch.full((3, 64, 64), 102, dtype=torch.uint8)]
        groups, sizes = harness._lossy_groups(images, resize)
        assert len(groups) == 1 and groups[0][1] == [0, 1, 2] and sizes == [(64, 64, 64, 64), (h, 64, 64, 64), (64, 64, 64, 64)]
        group = groups[0][0]
        assert group.dtype == torch.float32 and group.shape == (3, 3, 64, 64)
        assert torch.equal(group[:, 0, 0, 0], torch.tensor([51, 0, 102], dtype=torch.float32) / 255.0 + torch.tensor([0, 0.25, 0]))


def test_one_four_d_tensor_passes_through():
    from irec import harness
    images = D.tagged(range(3), 64)
    groups, sizes = harness._lossy_groups(images, False)
    assert sizes is None and len(groups) == 1 and groups[0][0] is images and groups[0][1] == [0, 1, 2]
    groups, sizes = harness._lossy_groups(images, True)
    assert sizes == [(64, 64, 64, 64)] * 3 and torch.equal(groups[0][0], images)
