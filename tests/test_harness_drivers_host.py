"""CPU tests of the drivers of irec.harness (compress_images, compress_images_lossy, decompress_images and its three siblings) with a
stub model: an nn.Module with one CPU parameter whose coding calls hand back canned rows and whose decoding calls read the bytes they
are given with irec.io's host readers.  What is held here is the drivers' own work -- batches, files on disk, the read-back check, the
rows, header groups, the order of `paths`, the status rows and texts, strict -- on shapes of a few blocks: R = 3 residual blocks of 4
blocks, max_K = 5, S = 36, 8 x 8 images for the ResNet VAE's drivers; blocks_per_res = [1, 5] (a residual block of one block, and a
segment size of 2 that does not divide 5) on 64 x 64 images for the two-level model's."""
import functools
import os
import types

import numpy as np
import pytest
import torch

SEED, S, MAX_K, BLOCK = 42, 36, 5, 1000
R, BPT, HW = 3, 4, 8
BPR, LHW = [1, 5], 64
KEYS = {"name", "comp_codelength", "comp_lossy_bpp", "comp_code_bpd", "code_nats", "n_indices", "indices_recovered", "comp_time"}


@functools.lru_cache(maxsize=None)
def canned(T, n=8):
    """K [n, T] in [0, MAX_K] and idx [n, T, MAX_K] with garbage past K; image i's first row is K = 1, idx = i: its name tag."""
    rng = np.random.default_rng(7 + T)
    K = rng.integers(0, MAX_K + 1, (n, T)).astype(np.int32)
    idx = rng.integers(0, S, (n, T, MAX_K)).astype(np.int32)
    K[:, 0], K[:, 1] = 1, MAX_K
    idx[:, 0, 0] = np.arange(n)
    for a in (K, idx):
        a.setflags(write=False)
    return K, idx


def lists_of(K, idx, bpr):
    first = np.concatenate([[0], np.cumsum(bpr)])
    return [[idx[t, :K[t]].tolist() for t in range(first[r], first[r + 1])] for r in range(len(bpr))]


def tags(images):
    return [int(round(float(v) * 100)) for v in images[:, 0, 0, 0]]


def tagged(ids, hw, dtype=torch.float32):
    return torch.stack([torch.full((3, hw, hw), i / 100 if dtype.is_floating_point else i, dtype=dtype) for i in ids])


class StubRVAE(torch.nn.Module):
    """BidirectionalResNetVAE as the drivers see it.  fail: tags whose batch cannot be coded; bad: tags whose image has status 8."""

    def __init__(self, fail=(), bad=()):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.residual_blocks = [types.SimpleNamespace(coder=types.SimpleNamespace(n_samples=S))]
        self.num_res_blocks, self.fail, self.bad, self.calls = R, set(fail), set(bad), []

    def blocks_per_tensor(self, image_shape):
        return BPT

    def _rows(self, chunk):
        from irec.coding import CodingError
        ids = tags(chunk)
        if self.fail & set(ids):
            raise CodingError(f"cannot code {sorted(self.fail & set(ids))}")
        K, idx = canned(R * BPT)
        return K[ids].reshape(-1, R, BPT), idx[ids].reshape(-1, R, BPT, MAX_K)

    def compress_packed(self, image, seed, update_sampler=False):
        K, idx = self._rows(image)
        return K, idx, None

    def compress(self, image, seed, update_sampler=False):
        K, idx = self._rows(image)
        per_image = [lists_of(K[i].reshape(-1), idx[i].reshape(-1, MAX_K), [BPT] * R) for i in range(K.shape[0])]
        return (per_image[0] if len(per_image) == 1 else per_image), None

    def status_text(self, status, K_image=None):
        from irec.models.resnet_vae import status_text
        return status_text(status)

    def _decompress_rec_status(self, blob, offsets, seed, image_shape, max_K=None, tables=None, segment_blocks=None):
        from irec.io import decode_files
        assert blob.dtype == torch.uint8 and blob.device == self.p.device
        hdr, K, idx = decode_files(blob.numpy(), offsets, R, BPT, max_K)
        ids = idx[:, 0, 0, 0].tolist()
        assert (hdr[:, 0] == seed).all() and image_shape == (len(ids), 3, HW, HW)
        self.calls.append((seed, ids, max_K, tables))
        status = np.array([8 if i in self.bad else 0 for i in ids], dtype=np.int32)
        return tagged(ids, HW), status, torch.from_numpy(K)

    def _decompress_lossless_status(self, rec_blob, rec_offsets, res_blob, res_offsets, seed, image_shape, max_K=None, stream_len=None):
        from irec.models.resnet_vae import STATUS_RESIDUAL
        _, status, K = self._decompress_rec_status(rec_blob, rec_offsets, seed, image_shape, max_K)
        ids = self.calls[-1][1]
        assert stream_len == 7 and res_blob.dtype == torch.uint8
        for k, i in enumerate(ids):
            res = res_blob[int(res_offsets[k]):int(res_offsets[k + 1])]
            assert res.numel() == 0 or int(res[12]) == i                    # every image beside its own .res bytes
            if status[k] == 0 and res.numel() == 0:
                status[k] = STATUS_RESIDUAL + 1
        return tagged(ids, HW, torch.uint8), status, K


class StubLossy(torch.nn.Module):
    """Large2LevelVAE as the drivers see it: compress_rec over the real host writers, decompress_rec over the real host readers."""

    def __init__(self, fail=(), bad=(), pendings=None):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.fail, self.bad, self.calls, self.pendings = set(fail), set(bad), [], pendings

    @staticmethod
    def _max_index(sampler):
        return S

    def blocks_per_res(self, image_shape, block_size):
        return list(BPR)

    def compress_rec(self, images, seed, sampler, block_size=None, rec_on_device=False, return_pendings=False, tables=None, segment_blocks=None):
        from irec.coding import CodingError
        from irec.io import encode_files_ragged, encode_files_segmented
        ids = tags(images)
        if self.fail & set(ids):
            raise CodingError(f"cannot code {sorted(self.fail & set(ids))}")
        assert not rec_on_device and return_pendings
        K, idx = (a[ids] for a in canned(sum(BPR)))
        h, w = images.shape[2:]
        if segment_blocks is None:
            blob, off = encode_files_ragged(seed, (h, w, 3), block_size, K, idx, S, BPR, tables=tables)
        else:
            blob, off = encode_files_segmented(seed, (h, w, 3), block_size, K, idx, S, BPR, segment_blocks)
        if self.pendings is not None:                                       # rows other than the files were built from
            K, idx = self.pendings(K.copy(), idx.copy())
        return (blob, off, images), (K, idx, list(BPR))

    def decompress_rec(self, blob, offsets, seed, image_shape, sampler, max_K=None, strict=True, rec_on_device=False, tables=None,
                       segment_blocks=None):
        from irec.io import decode_files_ragged, decode_files_segmented
        assert isinstance(blob, np.ndarray) and not rec_on_device and not strict
        if segment_blocks is None:
            hdr, K, idx = decode_files_ragged(blob, offsets, BPR, max_K, tables=tables)
        else:
            hdr, K, idx = decode_files_segmented(blob, offsets, BPR, max_K, segment_blocks)
        ids = idx[:, 0, 0].tolist()
        assert (hdr[:, 0] == seed).all() and image_shape == (len(ids), 3, LHW, LHW)
        self.calls.append((seed, ids, max_K, segment_blocks))
        return tagged(ids, LHW), np.array([8 if i in self.bad else 0 for i in ids], dtype=np.int32)


SAMPLER = types.SimpleNamespace(block_size=BLOCK)


def read(path):
    with open(path, "rb") as fh:
        return fh.read()


def files_of(blob, off):
    return [bytes(blob[off[i]:off[i + 1]]) for i in range(len(off) - 1)]


def check_rows(rows, names, sizes, n_idx, hw):
    assert [r["name"] for r in rows] == names
    for r, size, n in zip(rows, sizes, n_idx):
        assert set(r) == KEYS and r["indices_recovered"] is True
        assert r["comp_codelength"] == 8 * size and r["comp_lossy_bpp"] == 8 * size / (hw * hw) and r["comp_code_bpd"] == 8 * size / (hw * hw * 3)
        assert r["n_indices"] == n and r["code_nats"] == n * float(np.log(S)) and r["comp_time"] >= 0


# ---- compress_images -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("packed", [True, False], ids=["packed_host_leg", "per_image"])
def test_compress_images(tmp_path, packed):
    """Five images in batches of two, the second batch refused by the coder: error rows for exactly that batch, the others in order, all
    seven keys, and on disk the bytes of encode_files (packed) / write_compressed_code (per image) for the canned rows."""
    from irec import harness
    from irec.io import encode_files, write_compressed_code
    K, idx = canned(R * BPT)
    names = [f"im{i}" for i in range(5)]
    rows = harness.compress_images(StubRVAE(fail={2}), tagged(range(5), HW), names, SEED, BLOCK, str(tmp_path), batch=2, packed=packed)
    assert [r["name"] for r in rows] == names
    assert rows[2] == {"name": "im2", "error": "cannot code [2]"} and rows[3] == {"name": "im3", "error": "cannot code [2]"}
    good = [0, 1, 4]
    if packed:
        blob, off = encode_files(SEED, (HW, HW, 3), BLOCK, K[good].reshape(-1, R, BPT), idx[good].reshape(-1, R, BPT, MAX_K), max_index=S)
        want = files_of(blob, off)
    else:
        want = []
        for i in good:
            path = str(tmp_path / f"want{i}.rec")
            write_compressed_code(path, SEED, (HW, HW, 3), BLOCK, lists_of(K[i], idx[i], [BPT] * R), S)
            want.append(read(path))
    assert [read(tmp_path / f"im{i}.rec") for i in good] == want
    assert not os.path.exists(tmp_path / "im2.rec") and not os.path.exists(tmp_path / "im3.rec")
    check_rows([rows[i] for i in good], [names[i] for i in good], [len(f) for f in want], K[good].sum(axis=1).tolist(), HW)


def test_compress_images_refuses_tables_off_the_packed_legs(tmp_path):
    from irec import harness
    with pytest.raises(ValueError, match="tables go with the packed host leg or rec_on_device"):
        harness.compress_images(StubRVAE(), tagged(range(2), HW), ["a", "b"], SEED, BLOCK, str(tmp_path), packed=False, tables=object())


# ---- compress_images_lossy, host reader -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", [None, 2], ids=["rec", "recs"])
def test_compress_images_lossy(tmp_path, g):
    from irec import harness
    from irec.io import encode_files_ragged, encode_files_segmented, is_segmented
    K, idx = canned(sum(BPR))
    names = [f"im{i}" for i in range(5)]
    rows = harness.compress_images_lossy(StubLossy(fail={3}), SAMPLER, tagged(range(5), HW), names, SEED, BLOCK, str(tmp_path), batch=2, segment_blocks=g)
    assert [r["name"] for r in rows] == names
    assert rows[2] == {"name": "im2", "error": "cannot code [3]"} and rows[3] == {"name": "im3", "error": "cannot code [3]"}
    good = [0, 1, 4]
    if g is None:
        blob, off = encode_files_ragged(SEED, (HW, HW, 3), BLOCK, K[good], idx[good], S, BPR)
    else:
        blob, off = encode_files_segmented(SEED, (HW, HW, 3), BLOCK, K[good], idx[good], S, BPR, g)
    want = files_of(blob, off)
    ext = "rec" if g is None else "recs"
    assert sorted(os.listdir(tmp_path)) == [f"im{i}.{ext}" for i in good]
    assert [read(tmp_path / f"im{i}.{ext}") for i in good] == want and all(is_segmented(f) == (g is not None) for f in want)
    check_rows([rows[i] for i in good], [names[i] for i in good], [len(f) for f in want], K[good].sum(axis=1).tolist(), HW)
    with pytest.raises(ValueError, match=r"default symbol models only \(tables= with segment_blocks=\)"):
        harness.compress_images_lossy(StubLossy(), SAMPLER, tagged(range(2), HW), names[:2], SEED, BLOCK, str(tmp_path), tables=object(), segment_blocks=2)


@pytest.mark.parametrize("g", [None, 2], ids=["rec", "recs"])
def test_the_read_back_check_of_a_batch(tmp_path, g):
    """indices_recovered through the driver: rows that differ from the files' past K only are recovered; one wrong live index, one wrong
    K and one wrong header word (the seed the files carry) are not, each in its own image."""
    from irec import harness

    def pendings(K, idx):
        idx[0, 2, K[0, 2]:] += 1                          # image 0: garbage past K
        idx[1, 1, MAX_K - 1] += 1                         # image 1: a live index (row 1 has K = MAX_K)
        K[2, 3] += 1                                      # image 2: a count
        return K, idx
    rows = harness.compress_images_lossy(StubLossy(pendings=pendings), SAMPLER, tagged(range(4), HW), list("abcd"), SEED, BLOCK, str(tmp_path), segment_blocks=g)
    assert [r["indices_recovered"] for r in rows] == [True, False, False, True]
    model = StubLossy()
    encode = model.compress_rec
    model.compress_rec = lambda images, seed, *a, **kw: encode(images, seed + 1, *a, **kw)
    rows = harness.compress_images_lossy(model, SAMPLER, tagged(range(2), HW), list("ab"), SEED, BLOCK, str(tmp_path), segment_blocks=g)
    assert [r["indices_recovered"] for r in rows] == [False, False]


def rows_match_case():
    K, idx = (a[:5].copy() for a in canned(sum(BPR)))
    hdr = np.tile(np.array([SEED, BLOCK, S, HW, HW, 3, 0, 0, 2], dtype=np.uint32), (5, 1))
    K2, idx2 = K.copy(), np.where(np.arange(MAX_K)[None, None, :] < K[..., None], idx, 0).astype(np.int32)   # a reader's rows: zero past K
    idx2[1, 1, MAX_K - 1] += 1                            # image 1: a live index
    K2[2, 3] += 1                                         # image 2: a count
    hdr[3, 4] += 1                                        # image 3: the width word
    hdr[4, 2] += 1                                        # image 4: max_index, which the check does not read
    return hdr, K2, idx2, K, idx, [SEED, BLOCK, HW, HW, 3]


def test_rows_match_numpy_and_torch_agree():
    from irec import harness
    hdr, K2, idx2, K, idx, want = rows_match_case()
    same = harness._rows_match(hdr, K2, idx2, K, idx, want)
    assert isinstance(same, np.ndarray) and same.tolist() == [True, False, False, False, True]
    t = [torch.from_numpy(a.astype(np.int64) if a.dtype == np.uint32 else a) for a in (hdr, K2, idx2, K, idx)]
    same_t = harness._rows_match(*t, want)
    assert isinstance(same_t, torch.Tensor) and same_t.tolist() == same.tolist()


# ---- the read drivers ---------------------------------------------------------------------------------------------------------------------------
def write_rvae(tmp_path, res):
    """Two header groups interleaved (seed 42: images 0, 1, 2; seed 43: images 3, 4), then a file of another block structure and one
    shorter than its header.  res: NAME.res beside every NAME.rec but image 1's."""
    from irec.io import encode_files
    K, idx = canned(R * BPT)
    paths, order = [], [0, 3, 1, 4, 2]
    for i in order:
        blob, _ = encode_files(SEED + (i >= 3), (HW, HW, 3), BLOCK, K[i:i + 1].reshape(1, R, BPT), idx[i:i + 1].reshape(1, R, BPT, MAX_K), max_index=S)
        paths.append(str(tmp_path / f"im{i}.rec"))
        blob.tofile(paths[-1])
        if res and i != 1:
            with open(tmp_path / f"im{i}.res", "wb") as fh:
                fh.write(bytes(8) + (7).to_bytes(4, "little") + bytes([i]))
    other, _ = encode_files(SEED, (HW, HW, 3), BLOCK, K[:1, :R * 2].reshape(1, R, 2), idx[:1, :R * 2].reshape(1, R, 2, MAX_K), max_index=S)
    paths += [str(tmp_path / "other.rec"), str(tmp_path / "short.rec")]
    other.tofile(paths[-2])
    other[:10].tofile(paths[-1])
    return paths, order


DRIVERS = ["plain", "tables", "lossless"]


def run_rvae(kind, model, paths, **kw):
    from irec import harness
    if kind == "tables":
        return harness.decompress_images_tables(model, paths, types.SimpleNamespace(max_K=7), **kw)
    return (harness.decompress_images_lossless if kind == "lossless" else harness.decompress_images)(model, paths, **kw)


@pytest.mark.parametrize("kind", DRIVERS)
def test_decompress_images_groups_and_order(tmp_path, kind):
    from irec.coding import CodingError
    from irec.models.resnet_vae import STATUS_RESIDUAL, status_text
    lossless = kind == "lossless"
    paths, order = write_rvae(tmp_path, lossless)
    model = StubRVAE()
    good = [p for p in paths[:5] if not (lossless and p.endswith("im1.rec"))]
    ids = [i for i in order if not (lossless and i == 1)]
    images, rows = run_rvae(kind, model, good, batch=2)
    assert isinstance(images, torch.Tensor) and images.dtype == (torch.uint8 if lossless else torch.float32)
    assert torch.equal(images, tagged(ids, HW, images.dtype))                          # the order of `paths`
    first, second = [i for i in ids if i < 3], [i for i in ids if i >= 3]
    assert [(c[0], c[1]) for c in model.calls] == [(SEED, first[:2])] + ([(SEED, first[2:])] if first[2:] else []) + [(SEED + 1, second)]
    assert all(c[2] == (7 if kind == "tables" else MAX_K) for c in model.calls)      # the headers' largest word, or the tables' K
    assert all((c[3] is not None) == (kind == "tables") for c in model.calls)
    for p, i, row in zip(good, ids, rows):
        assert set(row) == {"name", "seed", "image_shape", "block_size", "status", "decomp_time"}
        assert (row["name"], row["seed"], row["image_shape"], row["block_size"], row["status"]) == (os.path.basename(p), SEED + (i >= 3), (HW, HW, 3), BLOCK, 0)
    # every kind of refusal in one call: a list, the refused images zero or None, each row with its text
    model = StubRVAE(bad={4})
    images, rows = run_rvae(kind, model, paths, batch=2, strict=False)
    want_status = [0, 0, STATUS_RESIDUAL + 1 if lossless else 0, 8, 0, 17, 4]
    assert isinstance(images, list) and [r["status"] for r in rows] == want_status
    assert images[6] is None and rows[6] == {"name": "short.rec", "status": 4, "error": status_text(4)}
    assert rows[5]["error"] == f"{status_text(17)}: 3 residual blocks of 2 blocks for a 8 x 8 x 3 image do not match the model"
    assert rows[3]["error"] == status_text(8) and "error" not in rows[0]
    for im, i, st in zip(images[:6], order + [0], want_status):
        assert im.dtype == (torch.uint8 if lossless else torch.float32) and im.shape == (3, HW, HW)
        assert torch.equal(im, tagged([i], HW, im.dtype)[0]) if st == 0 else not im.any()
    first_bad = 2 if lossless else 3
    with pytest.raises(CodingError) as e:
        run_rvae(kind, StubRVAE(bad={4}), paths, batch=2)
    assert str(e.value) == f"{rows[first_bad]['error']} (image {first_bad})"


def test_decompress_images_lossy_groups_and_order(tmp_path):
    from irec import harness
    from irec.coding import CodingError
    from irec.io import encode_files_ragged, encode_files_segmented
    from irec.models.resnet_vae import status_text
    K, idx = canned(sum(BPR))
    paths, order = [], [0, 3, 5, 1, 4, 6, 2]                  # seed 42 plain: 0, 1, 2; seed 43 plain: 3, 4; seed 42, g = 2: 5, 6
    for i in order:
        if i >= 5:
            blob, _ = encode_files_segmented(SEED, (LHW, LHW, 3), BLOCK, K[i:i + 1], idx[i:i + 1], S, BPR, 2)
        else:
            blob, _ = encode_files_ragged(SEED + (i >= 3), (LHW, LHW, 3), BLOCK, K[i:i + 1], idx[i:i + 1], S, BPR)
        paths.append(str(tmp_path / f"im{i}.{'recs' if i >= 5 else 'rec'}"))
        blob.tofile(paths[-1])
    model = StubLossy()
    images, rows = harness.decompress_images_lossy(model, SAMPLER, paths, batch=2)
    assert torch.equal(images, tagged(order, LHW)) and [r["status"] for r in rows] == [0] * 7
    assert [r["name"] for r in rows] == [os.path.basename(p) for p in paths]
    assert model.calls == [(SEED, [0, 1], MAX_K, None), (SEED, [2], MAX_K, None), (SEED + 1, [3, 4], MAX_K, None), (SEED, [5, 6], MAX_K, 2)]
    other, _ = encode_files_ragged(SEED, (LHW, LHW, 3), BLOCK, K[:1, :5], idx[:1, :5], S, [1, 4])
    paths += [str(tmp_path / "other.rec"), str(tmp_path / "short.recs")]
    other.tofile(paths[-2])
    np.fromfile(paths[2], dtype=np.uint8)[:30].tofile(paths[-1])
    images, rows = harness.decompress_images_lossy(StubLossy(bad={1, 6}), SAMPLER, paths, batch=2, strict=False)
    assert isinstance(images, list) and [r["status"] for r in rows] == [0, 0, 0, 8, 0, 8, 0, 17, 4]
    assert images[8] is None and rows[8] == {"name": "short.recs", "status": 4, "error": status_text(4)}
    assert rows[7]["error"] == f"{status_text(17)}: 2 residual blocks of (1, 4) blocks for a 64 x 64 x 3 image do not match the model"
    assert rows[3]["error"] == rows[5]["error"] == status_text(8)
    for im, i, row in zip(images[:8], order + [0], rows):
        assert torch.equal(im, tagged([i], LHW)[0]) if row["status"] == 0 else (not im.any() and im.shape == (3, LHW, LHW))
    with pytest.raises(CodingError) as e:
        harness.decompress_images_lossy(StubLossy(bad={1, 6}), SAMPLER, paths, batch=2)
    assert str(e.value) == f"{status_text(8)} (image 3)"
