"""GPU tests of the one-level lossy model (irec.models.Large1LevelVAE) on every path the two-level model has: the list path
(compress / decompress through a file), the packed and .rec paths on host threads and on the device, symbol tables, the segmented
container, both coders, the seeded sampling pass, and files of the other model.

Large1LevelVAE(num_filters=8) has 4 x 4 x 8 = 128 latent dims on a 64 x 64 image and 8 x 4 x 8 = 256 on 128 x 64; block_size = 5 cuts
them into 26 blocks (tail of 3) and 52 (tail of 1).  Files are compared byte for byte; pixels with torch.equal where both sides run the
same batch, and within 1e-5 between a batch of three and an image alone (the bound tests/test_lossy_packed_gpu.py uses there: batch
size may change convolution bits)."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEED, BLOCK, FILTERS = 42, 5, 8
SHAPES = {"64x64": (64, 64), "128x64": (128, 64)}
BATCH_TOL = 1e-5


def _beam():
    import irec
    return irec.BeamSearchCoder(kl_per_partition=3., n_beams=10, extra_samples=1., block_size=BLOCK)


def _importance():
    import irec
    return irec.GaussianCoder(kl_per_partition=3., sampler=irec.ImportanceSampler(coding_bits=3. / math.log(2.)), block_size=BLOCK)


CODERS = {"beam": _beam, "importance": _importance}
LADDER = (1., 4., 16., 64., 256., 1024.)


def _model(scale):
    from irec.models import Large1LevelVAE
    torch.manual_seed(3)
    m = Large1LevelVAE(num_filters=FILTERS).cuda().eval()
    with torch.no_grad():                         # the loc half of the posterior's head: a larger scale, a larger KL
        head = m.analysis_transform[-1]
        head.weight[:FILTERS].mul_(scale)
        head.bias[:FILTERS].mul_(scale)
    return m


def _files(blob, off):
    blob, off = (blob.cpu().numpy(), off.cpu().numpy()) if hasattr(blob, "cpu") else (blob, off)
    return [blob[off[i]:off[i + 1]].tobytes() for i in range(len(off) - 1)]


@functools.lru_cache(maxsize=None)
def _setup(kind, shape_name):
    """The model with its posterior head scaled until a block has K >= 3 and K is not constant, three images, and per image the file
    and the reconstruction of the LIST path (compress(file_path, ...)): computed once, never changed."""
    import tempfile
    h, w = SHAPES[shape_name]
    torch.manual_seed(11)
    images = (torch.rand(3, 3, h, w) - 0.5).cuda()
    for scale in LADDER:
        m, sampler = _model(scale), CODERS[kind]()
        K = m.compress_packed(images, SEED, sampler)[0]
        print(f"{kind} {shape_name}: head scale {scale}: K {K.min()}..{K.max()}")
        if K.max() >= 3 and K.min() != K.max():
            break
    else:
        raise AssertionError("no head scale gave a block with K >= 3 and a K that is not constant")
    bpr = m.blocks_per_res(images.shape, BLOCK)
    assert bpr == [-(-(h // 16) * (w // 16) * FILTERS // BLOCK)] and K.shape == (3, bpr[0])
    S = m._max_index(sampler)
    files, recons, backs = [], [], []
    with tempfile.TemporaryDirectory() as tmp:
        for i in range(3):
            path = f"{tmp}/{i}.rec"
            recons.append(m.compress(path, images[i].permute(1, 2, 0).contiguous(), seed=SEED, sampler=sampler, block_size=BLOCK, max_index=S))
            backs.append(m.decompress(path, sampler))
            files.append(open(path, "rb").read())
    return {"model": m, "sampler": sampler, "images": images, "files": files, "recons": recons, "backs": backs, "S": S, "shape": (3, 3, h, w)}


class _ReadBacks:
    """Counts the device-to-host reads of CUDA tensors while open (Tensor.cpu / .item / .tolist)."""

    def __enter__(self):
        self.count, self._saved = 0, {}
        for name in ("cpu", "item", "tolist"):
            original = getattr(torch.Tensor, name)
            self._saved[name] = original

            def counted(t, *a, _original=original, **kw):
                self.count += bool(t.is_cuda)
                return _original(t, *a, **kw)
            setattr(torch.Tensor, name, counted)
        return self

    def __exit__(self, *exc):
        for name, original in self._saved.items():
            setattr(torch.Tensor, name, original)
        return False


@pytest.mark.parametrize("shape_name", list(SHAPES))
@pytest.mark.parametrize("kind", list(CODERS))
def test_list_path_round_trip(engine, kind, shape_name):
    """compress(file) then decompress(file) returns the reconstruction compress returned, under either coder."""
    s = _setup(kind, shape_name)
    for recon, back in zip(s["recons"], s["backs"]):
        assert recon.shape == (1, *s["shape"][1:]) and torch.equal(recon, back)
    import irec
    import tempfile
    with tempfile.NamedTemporaryFile(suffix=".rec") as fh:
        fh.write(s["files"][0])
        fh.flush()
        seed, shape, block_size, blocks = irec.io.read_compressed_code(fh.name)
    assert (seed, tuple(shape), block_size) == (SEED, (*s["shape"][2:], 3), BLOCK) and len(blocks) == 1      # R = 1


@pytest.mark.parametrize("shape_name", list(SHAPES))
@pytest.mark.parametrize("kind", list(CODERS))
def test_compress_rec_writes_the_list_path_files(engine, kind, shape_name):
    """A batch of 3: image by image exactly the bytes compress(file_path, ...) writes, on host threads and on the device; and
    decompress_rec gives the list path's pixels with one status read-back."""
    s = _setup(kind, shape_name)
    m, sampler, images, shape = s["model"], s["sampler"], s["images"], s["shape"]
    blob_h, off_h, recon_h = m.compress_rec(images, SEED, sampler)
    blob_d, off_d, recon_d = m.compress_rec(images, SEED, sampler, rec_on_device=True)
    assert isinstance(blob_h, np.ndarray) and blob_d.is_cuda
    assert _files(blob_h, off_h) == s["files"] and _files(blob_d, off_d) == s["files"]
    assert torch.equal(recon_h, recon_d)
    max_K = int(m.compress_packed(images, SEED, sampler)[1].shape[2])
    off_host = off_d.cpu().numpy()
    with _ReadBacks() as reads:
        back_d = m.decompress_rec(blob_d, off_host, SEED, shape, sampler, rec_on_device=True, max_K=max_K)
    assert reads.count == 1, reads.count                                     # the per-image status
    back_h = m.decompress_rec(blob_h, off_h, SEED, shape, sampler)
    assert torch.equal(back_h, back_d) and torch.equal(back_h, recon_h)
    K, idx, bpr, recon_p = m.compress_packed(images, SEED, sampler)
    assert torch.equal(recon_p, recon_h) and torch.equal(m.decompress_packed(K, idx, SEED, shape, sampler), back_h)
    for i in range(3):
        err = max(float((back_h[i] - s["backs"][i][0]).abs().max()), float((recon_h[i] - s["recons"][i][0]).abs().max()))
        print(f"{kind} {shape_name}: image {i}: max |alone - batch| = {err:.3g}")
        assert err <= BATCH_TOL
    # one image: the same batch on both sides, the same bits
    blob, off, recon = m.compress_rec(images[1:2], SEED, sampler, rec_on_device=True)
    assert _files(blob, off) == s["files"][1:2] and torch.equal(recon, s["recons"][1])
    assert torch.equal(m.decompress_rec(blob, off, SEED, (1, *shape[1:]), sampler, rec_on_device=True), s["backs"][1])


@pytest.mark.parametrize("on_device", [False, True], ids=["host_leg", "device_leg"])
def test_segmented_and_tables_round_trip(engine, on_device):
    from irec import harness
    s = _setup("beam", "128x64")
    m, sampler, images, shape = s["model"], s["sampler"], s["images"], s["shape"]
    plain = m.decompress_rec(*m.compress_rec(images, SEED, sampler)[:2], SEED, shape, sampler)
    blob, off, recon = m.compress_rec(images, SEED, sampler, rec_on_device=on_device, segment_blocks=7)
    assert _files(blob, off) != s["files"]
    assert torch.equal(m.decompress_rec(blob, off, SEED, shape, sampler, rec_on_device=on_device, segment_blocks=7), plain)
    tables = harness.fit_symbol_tables_lossy(m, sampler, images, SEED, BLOCK)
    assert tables.n_res_blocks == 1
    blob, off, recon_t = m.compress_rec(images, SEED, sampler, rec_on_device=on_device, tables=tables)
    assert torch.equal(recon_t, recon)
    assert torch.equal(m.decompress_rec(blob, off, SEED, shape, sampler, rec_on_device=on_device, tables=tables), plain)
    _, status = m.decompress_rec(blob, off, SEED, shape, sampler, rec_on_device=on_device, strict=False)
    assert status.tolist() == [5, 5, 5]                                     # files under tables, read without them
    with pytest.raises(ValueError, match="tables= with segment_blocks="):
        m.compress_rec(images, SEED, sampler, rec_on_device=on_device, tables=tables, segment_blocks=7)
    with pytest.raises(ValueError, match="tables= with segment_blocks="):
        m.decompress_rec(blob, off, SEED, shape, sampler, rec_on_device=on_device, tables=tables, segment_blocks=7)


def test_forward_with_a_seed(engine):
    """The same seed gives the same bits; image i of a batch is that image alone under image_base + i (up to the convolutions' batch
    bound); kl_divergence() is the closed-form KL (float64 torch) within the bound the ideal tests use for a sum of n terms,
    n 2^-53 sum |term|."""
    from irec import ideal
    from irec.models.resnet_vae import ModelError
    s = _setup("beam", "128x64")
    m, images = s["model"], s["images"]
    fresh = _model(1.)
    with pytest.raises(ModelError):
        fresh.kl_divergence()
    none, first = m.forward(images, seed=SEED, image_base=2)
    kls = [k.clone() for k in m.kl_divergence()]
    post, prior = m.posterior, m.prior
    _, again = m.forward(images, seed=SEED, image_base=2)
    assert none is None and torch.equal(first, again) and first.shape == images.shape
    assert len(kls) == 1 and kls[0].shape == (3,) and kls[0].dtype == torch.float64 and torch.equal(kls[0], m.kl_divergence()[0])
    # the draw is tag 3 of irec.ideal: the host twin on the same statistics gives the KL's bits
    cpu = lambda d: type(d)(d.loc.cpu(), d.scale.cpu())  # noqa: E731
    assert torch.equal(ideal.posterior_draw(cpu(post), cpu(prior), SEED, 3, 2)[1], kls[0].cpu())
    # closed form, float64 torch
    mq, sq, mp, sp = (t.double().reshape(3, -1) for t in (post.loc, post.scale, prior.loc, prior.scale))
    terms = torch.log(sp / sq) + (sq * sq + (mq - mp) ** 2) / (2.0 * sp * sp) - 0.5
    want, bound = terms.sum(dim=1), terms.shape[1] * 2.0 ** -53 * terms.abs().sum(dim=1)
    print("kl", kls[0].tolist(), "closed form", want.tolist(), "bound", bound.tolist())
    assert ((kls[0] - want).abs() <= bound).all() and (kls[0] > 0).all()
    # independent of the batch: image 1 alone, as image number 3
    _, alone = m.forward(images[1:2], seed=SEED, image_base=3)
    kl_alone = m.kl_divergence()[0]
    assert float((alone[0] - first[1]).abs().max()) <= BATCH_TOL
    assert float((kl_alone[0] - kls[0][1]).abs()) <= 2 * float(bound[1]) + 1e-4 * float(kls[0][1])      # (the statistics carry the convolutions' batch bits)
    assert not torch.equal(m.forward(images, seed=SEED + 1, image_base=2)[1], first)
    assert not torch.equal(m.forward(images, seed=SEED, image_base=3)[1], first)
    with pytest.raises(NotImplementedError):
        m.forward(images)


@functools.lru_cache(maxsize=None)
def _two_level():
    from irec.models import Large2LevelVAE
    torch.manual_seed(3)
    m = Large2LevelVAE(level_1_filters=8, level_2_filters=4).cuda().eval()
    with torch.no_grad():
        for mod in (m.hyper_analysis_transform[-1], m._level_1_posterior_loc_combiner):
            mod.weight.mul_(16.)
            mod.bias.mul_(16.)
    return m


@pytest.mark.parametrize("on_device", [False, True], ids=["host_reader", "device_reader"])
def test_files_of_the_other_model_are_refused_with_a_status(engine, on_device, tmp_path):
    from irec import harness
    from irec.coding import CodingError
    s = _setup("beam", "128x64")
    one, sampler, images, shape = s["model"], s["sampler"], s["images"], s["shape"]
    two = _two_level()
    blob_1, off_1, _ = one.compress_rec(images, SEED, sampler, rec_on_device=on_device)
    blob_2, off_2, _ = two.compress_rec(images, SEED, sampler, rec_on_device=on_device)
    for model, blob, off in ((one, blob_2, off_2), (two, blob_1, off_1)):
        _, status = model.decompress_rec(blob, off, SEED, shape, sampler, strict=False, rec_on_device=on_device)
        print(type(model).__name__, "on the other model's files:", status.tolist())
        assert status.shape == (3,) and (status != 0).all()
        with pytest.raises(CodingError, match=r"\(image 0\)"):
            model.decompress_rec(blob, off, SEED, shape, sampler, rec_on_device=on_device)
    # and through the harness: status 17, the block structure is not the model's
    names = ["a", "b", "c"]
    harness.compress_images_lossy(two, sampler, images, names, SEED, BLOCK, str(tmp_path / "two"), rec_on_device=on_device)
    harness.compress_images_lossy(one, sampler, images, names, SEED, BLOCK, str(tmp_path / "one"), rec_on_device=on_device)
    for model, files in ((one, "two"), (two, "one")):
        paths = [str(tmp_path / files / f"{nm}.rec") for nm in names]
        pixels, rows = harness.decompress_images_lossy(model, sampler, paths, strict=False, rec_on_device=on_device)
        assert [r["status"] for r in rows] == [17, 17, 17] and not pixels.any()
    pixels, rows = harness.decompress_images_lossy(one, sampler, [str(tmp_path / "one" / f"{nm}.rec") for nm in names], rec_on_device=on_device)
    assert all(r["status"] == 0 for r in rows) and pixels.shape == shape
