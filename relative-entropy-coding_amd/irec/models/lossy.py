"""PyTorch-ROCm host shims of the reference's lossy VAE call surfaces: the two-level model
(rec/models/lossy/large_2_level_vae.py:320-456) and the one-level model, the lossy driver's default
(rec/models/lossy/large_1_level_vae.py:120-244) -- `call(tensor, sampling_fn)`, `compress(file_path, image, seed, sampler,
block_size, max_index)` and `decompress(file_path, sampler)`: one `sampler.encode` call per level and image, SEQUENTIAL where there
are two (level 2, then level 1 whose prior is synthesised from the coded level-2 latent), followed by `write_compressed_code`.

As with the RVAE shim, only the hand-off is modelled: the Balle-style analysis / synthesis transforms are plain strided
(transposed) convolutions with random-init weights (GDN, SignalConv2D and the trained checkpoints are out of scope,
SURVEY.md §2 rows 12-14).  Latent shapes follow the reference: two levels, level 1 = [1, H/16, W/16, 196], level 2 = [1, H/64, W/64, 128]
(large_2_level_vae.py:313, compress_with_lossy_model.py:36-37); one level, [1, H/16, W/16, num_filters], 192 by default
(large_1_level_vae.py:155, compress_with_lossy_model.py:26-35) -- handed to the coder in NHWC order.

What the two models share -- everything but their transforms and the order of their levels -- is _LevelsVAE: a model names its levels
in file order (`_latent_dims`, `_ideal_tags`), codes them (`_code_levels`) and decodes them (`_decode_levels`); the list path, the
packed path and the .rec paths are written once over those.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from ..coding.pending import PendingCode, recode
from ..io import header_seed, read_compressed_code, write_compressed_code
from ._rec_rows import STATUS_ROWS, finish, header_want, join_status, packed_rows, read_rows
from .resnet_vae import ModelError, _Normal, _nchw, _nhwc, deterministic_transforms


def _down(cin, cout, n):
    layers, c = [], cin
    for i in range(n):
        layers += [nn.Conv2d(c, cout, 5, stride=2, padding=2)] + ([nn.ELU()] if i < n - 1 else [])
        c = cout
    return nn.Sequential(*layers)


def _up(cin, cmid, cout, n):
    layers, c = [], cin
    for i in range(n):
        last = i == n - 1
        layers += [nn.ConvTranspose2d(c, cout if last else cmid, 5, stride=2, padding=2, output_padding=1)] + \
                  ([] if last else [nn.ELU()])
        c = cmid
    return nn.Sequential(*layers)


class _LevelsVAE(nn.Module):
    """The call surface of a lossy model of R = len(_ideal_tags) levels, the levels in FILE order (block_indices[r], the rows of residual
    block r).  A model supplies:
      _ideal_tags                    irec.ideal.posterior_draw's tag per level, in file order
      _latent_dims(h, w)             the latent elements per level of an h x w image
      _code_levels(tensor, sampling_fn) -> (block_indices, y NHWC): the inference and generative passes up to the coded last latent,
                                     one sampling_fn(target=posterior, coder=prior) call per level, the distributions left as attributes
      _decode_levels(n, h, w, decode) -> y NHWC: the generative pass, decode(prior, r) giving level r's latent
      synthesis_transform, _prior_base"""
    _ideal_tags = ()

    @property
    def n_levels(self):
        return len(self._ideal_tags)

    @torch.no_grad()
    def forward(self, tensor, sampling_fn=None, seed=None, image_base=0):
        """large_2_level_vae.py:320-404, large_1_level_vae.py:160-203.  tensor: [N, 3, H, W] (the reference's N = 1, or a batch that
        `sampling_fn` codes with batched=True); returns (block_indices, reconstruction), block_indices one entry per level.
        seed (instead of sampling_fn): the sampling pass of the reference's evaluation script (`model(image)`) -- every level is DRAWN
        from its posterior (irec.ideal.posterior_draw under the level's tag: 2 and 1 for the two levels of Large2LevelVAE, the level-1
        prior synthesised from the level-2 draw; 3 for the one level of Large1LevelVAE), image i drawing as image number
        image_base + i; nothing is coded or read back.  Returns (None, reconstruction) and leaves the levels' KL for kl_divergence()."""
        if sampling_fn is None and seed is None:
            raise NotImplementedError("training / sampling passes are outside the compression shim")
        if seed is not None:
            if sampling_fn is not None:
                raise ValueError("forward takes sampling_fn (a coded pass) or seed (a sampling pass), not both")
            from .. import ideal
            levels, kls = iter(self._ideal_tags), []

            def sampling_fn(target, coder):
                sample, kl = ideal.posterior_draw(target, coder, seed, next(levels), image_base)
                kls.append(kl)
                return None, sample
            _, y = self._code_levels(tensor, sampling_fn)
            self._kl = kls
            return None, self.synthesis_transform(_nchw(y))
        block_indices, y = self._code_levels(tensor, sampling_fn)
        return block_indices, self.synthesis_transform(_nchw(y))

    def kl_divergence(self):
        """The reference's kl_divergence for the last forward(tensor, seed=): one float64 [N] per level, in file order ([kl_level_2,
        kl_level_1]; [kl] for one level), nats."""
        if getattr(self, "_kl", None) is None:
            raise ModelError("kl_divergence needs a forward(tensor, seed=) pass first")
        return list(self._kl)

    def compress(self, file_path, image, seed, sampler, block_size, max_index):
        """large_2_level_vae.py:406-419, large_1_level_vae.py:205-218.  image: [H, W, 3] tensor (the reference's layout)."""
        seed = header_seed(seed, "compress")               # (before anything is coded: the file could not name another seed)
        sampling_fn = lambda target, coder: sampler.encode(target, coder, seed=seed)  # noqa: E731  (:408)
        x = image.permute(2, 0, 1)[None].contiguous()
        with deterministic_transforms():
            block_indices, reconstruction = self(x, sampling_fn=sampling_fn)
        write_compressed_code(file_path=file_path, seed=seed, image_shape=tuple(image.shape), block_size=block_size,
                              block_indices=block_indices, max_index=max_index)
        return reconstruction

    @torch.no_grad()
    def decompress(self, file_path, sampler):
        """large_2_level_vae.py:421-456, large_1_level_vae.py:220-244 (the reference unpacks image_shape as (batch, height, width);
        here (h, w, c))."""
        seed, image_shape, block_size, block_indices = read_compressed_code(file_path=file_path)
        height, width, _ = image_shape
        with deterministic_transforms():
            y = self._decode_levels(1, height, width, lambda prior, r: sampler.decode(prior, seed=seed, indices=block_indices[r]))
            return self.synthesis_transform(_nchw(y))

    # ---- the packed path: a batch per call, indices as rows (K [N, T], idx [N, T, max_K]), ragged .rec files ----------------------
    # The levels differ in size (a Kodak image under Large2LevelVAE: 13 coder blocks at level 2, 302 at level 1), so an image is
    # T = sum(blocks_per_res) rows in file order, block_indices = [level_2, level_1]; one level is R = 1 of the same containers.
    def blocks_per_res(self, image_shape, block_size):
        """The coder blocks of an image's levels, in file order (Coder.split, coder.py:69-83).  image_shape: [N, 3, H, W]."""
        _, _, h, w = image_shape
        return [1 if block_size is None else -(-n // int(block_size)) for n in self._latent_dims(h, w)]

    @staticmethod
    def _max_index(sampler):
        """The header's max_index word: the samples a step chooses among (the sequential coder's are its sampler's)."""
        return sampler.sampler.n_samples() if getattr(sampler, "sampler", None) is not None else sampler.n_samples

    def _compress_device(self, images, seed, sampler):
        """The coding half of a batched compress, on the device with no host synchronisation: (one PendingCode per level, y).  The
        calls are sequential (level 1's prior comes from the coded level-2 sample) and deferred."""
        sampling_fn = lambda target, coder: sampler.encode(target, coder, seed=seed, batched=True, defer=True)  # noqa: E731
        with deterministic_transforms():
            return self._code_levels(images, sampling_fn)

    def _compress_gather(self, images, seed, sampler, gather):
        """(gather(pendings), reconstruction).  The rows are read back BEFORE the synthesis transform is launched, so that what the caller
        does with them on the host (the files' arithmetic coder) runs while the device computes the reconstruction, as the list path's
        write_compressed_code does; a pass that has to be coded again has not paid for a reconstruction either."""
        gathered, y = recode(lambda: self._compress_device(images, seed, sampler), gather, [sampler])
        with deterministic_transforms():
            return gathered, self.synthesis_transform(_nchw(y))

    @torch.no_grad()
    def compress_packed(self, images, seed, sampler):
        """`compress` for a batch [N, 3, H, W], the indices left packed: (K [N, T], idx [N, T, max_K], blocks_per_res, reconstruction),
        K / idx int32 numpy -- ONE device-to-host copy, no Python object per index.  irec.io.encode_files_ragged takes them."""
        (K, idx, bpr), reconstruction = self._compress_gather(images, seed, sampler, PendingCode.gather_packed_ragged)
        return K, idx, bpr, reconstruction

    @torch.no_grad()
    def compress_rec(self, images, seed, sampler, block_size=None, rec_on_device=False, return_pendings=False, tables=None, segment_blocks=None):
        """A batch to its .rec files: (blob uint8, offsets int64 [N + 1], reconstruction), image i's file blob[offsets[i]:offsets[i + 1]]
        byte for byte what `compress(file_path, ...)` writes for it.  rec_on_device=False (the default: an arithmetic coder's stream is
        serial, and Kodak-size streams are long): one packed read-back, then irec.io.encode_files_ragged on host threads; blob and
        offsets are numpy.  rec_on_device=True: the rows stay on the device (PendingCode.gather_packed_ragged_device,
        irec.io.encode_files_device_ragged), only K, the offsets and the statuses are read back; blob and offsets are CUDA tensors.
        block_size: the header's block-size word (default: the coder's own; 0 for a coder without one).
        return_pendings: also the rows the files were built from, ((blob, offsets, reconstruction), (K, idx, blocks_per_res)).
        tables: an irec.io.SymbolTables (harness.fit_symbol_tables_lossy) -- the streams coded under its count tables on either leg, the
        files flagged as the reference's writer flags them; decompress_rec needs the same tables.
        segment_blocks: None for the reference's file; g >= 1 for the segmented container (NAME.recs, INTEGRATION.md §8: each level's rows
        in segments of g coder blocks, lanes and host threads over segments -- irec.io.encode_files_segmented on host threads,
        encode_files_device_segmented with rec_on_device), which decompress_rec reads under the same segment_blocks.  Default symbol
        models only: together with tables it is a ValueError."""
        from ..io import encode_files_device_ragged, encode_files_device_segmented, encode_files_ragged, encode_files_segmented
        seed = header_seed(seed, "compress_rec")           # (before anything is coded: the files could not name another seed)
        if segment_blocks is not None and tables is not None:
            raise ValueError("compress_rec: the segmented container codes under the default symbol models only (tables= with segment_blocks=)")
        _, _, height, width = images.shape
        gather = PendingCode.gather_packed_ragged_device if rec_on_device else PendingCode.gather_packed_ragged
        (K, idx, bpr), reconstruction = self._compress_gather(images, seed, sampler, gather)
        if block_size is None:
            block_size = sampler.block_size if sampler.block_size is not None else 0
        if segment_blocks is not None:
            encode = encode_files_device_segmented if rec_on_device else encode_files_segmented
            blob, offsets = encode(seed, (height, width, 3), block_size, K, idx, self._max_index(sampler), bpr, segment_blocks)
        else:
            encode = encode_files_device_ragged if rec_on_device else encode_files_ragged
            blob, offsets = encode(seed, (height, width, 3), block_size, K, idx, self._max_index(sampler), bpr, tables=tables)
        return ((blob, offsets, reconstruction), (K, idx, bpr)) if return_pendings else (blob, offsets, reconstruction)

    def _decompress_device(self, K, idx, seed, image_shape, sampler, status):
        """The generative pass driven by rows on the device: K [N, T], idx [N, T, max_K] int32 (contiguous, or the views of one joined
        tensor), each level's coder reading its rows in place and accumulating its verdict on them into `status` (int32 [N], device).
        No host synchronisation."""
        n, _, height, width = image_shape
        bpr = self.blocks_per_res(image_shape, sampler.block_size)
        if K.dim() != 2 or tuple(K.shape) != (n, sum(bpr)) or idx.dim() != 3 or tuple(idx.shape[:2]) != tuple(K.shape):
            raise ModelError(f"K {tuple(K.shape)} / idx {tuple(idx.shape)} are not [N = {n}, T = {sum(bpr)}] and [N, T, max_K]: images of shape "
                             f"{tuple(image_shape)} are coded in {bpr} blocks")
        rows = packed_rows(n, bpr, K.device)
        with deterministic_transforms():
            y = self._decode_levels(n, height, width, lambda prior, r: sampler.decode(prior, None, seed=seed, batched=True,
                                                                                      packed=(K, idx, rows[r]), status=status))
            return self.synthesis_transform(_nchw(y))

    @staticmethod
    def _to_device(a, device):
        return a.to(device) if hasattr(a, "is_cuda") else torch.from_numpy(np.ascontiguousarray(a)).to(device)

    @torch.no_grad()
    def decompress_packed(self, K, idx, seed, image_shape, sampler, strict=True):
        """`decompress` for packed rows (K [N, T], idx [N, T, max_K] int32: CUDA tensors read where they lie, or numpy arrays uploaded
        once): ONE read-back, the per-image status.  strict: CodingError naming the first image whose rows cannot be decoded;
        strict=False: (reconstruction, status int32 numpy [N]) -- 0, or STATUS_ROWS + irec_rows_status; the images with status 0 are
        what they would be without the others."""
        device = self._prior_base.device
        K, idx = self._to_device(K, device), self._to_device(idx, device)
        status = torch.zeros(int(image_shape[0]), dtype=torch.int32, device=device)
        reconstruction = self._decompress_device(K, idx, seed, image_shape, sampler, status)
        host = status.cpu().numpy()
        return finish(reconstruction, np.where(host != 0, host + STATUS_ROWS, 0).astype(np.int32), strict)

    @torch.no_grad()
    def decompress_rec(self, blob, offsets, seed, image_shape, sampler, max_K=None, strict=True, rec_on_device=False, tables=None,
                       segment_blocks=None):
        """The inverse of compress_rec: N .rec files (file i = blob[offsets[i]:offsets[i + 1]]) to reconstructions [N, 3, H, W].
        rec_on_device=False: the files are read on host threads (irec.io.decode_files_ragged; blob / offsets numpy or tensors) and the
        rows uploaded once; rec_on_device=True: blob is a CUDA tensor and the rows never leave the device
        (irec.io.decode_files_device_ragged's launch form).  Either way the headers are checked against seed, image_shape and the
        model's level count (R = 2 for Large2LevelVAE, R = 1 for Large1LevelVAE: a file of the other model is refused with a status),
        each level's coder reads its rows in place and checks them on the device, and there is ONE read-back, the per-image status, in
        the encoding of BidirectionalResNetVAE.decompress_rec: 0 ok; 1 .. 18 irec_rec_status; STATUS_HEADER; STATUS_ROWS +
        irec_rows_status; first cause in that order.  strict: CodingError with the cause, "(image i)" appended; strict=False:
        (reconstruction, status int32 numpy [N]), the images with status 0 being what they would be without the others.
        max_K: index slots per block (None: the largest max_partitions word of the files' headers; with count tables, their largest K).
        tables: the irec.io.SymbolTables the files were written under; a file whose header asks for tables the call did not bring has
        status 5 (IREC_REC_E_COUNT_FILES), one without flags decodes under the default models.
        segment_blocks: None for the reference's files; g for segmented files written with compress_rec(segment_blocks=g) (max_K None:
        the largest max_part word of their directories).  The segmented reader's own causes (irec_rec_status 20 .. 22: magic or
        version, directory, segment size) are STATUS_SEGMENTED + 0 .. 2 in the joined status; a plain file read as a segmented one has
        the first of them, and a segmented file read without segment_blocks has status 5."""
        n, _, height, width = image_shape
        bpr = self.blocks_per_res(image_shape, sampler.block_size)
        device = self._prior_base.device
        if segment_blocks is not None and tables is not None:
            raise ValueError("decompress_rec: the segmented container codes under the default symbol models only (tables= with segment_blocks=)")
        words, K, idx, rec_status = read_rows(blob, offsets, bpr, max_K, rec_on_device=rec_on_device, tables=tables, segment_blocks=segment_blocks,
                                              device=device)
        if len(rec_status) != n:
            raise ModelError(f"{len(rec_status)} files for images of shape {tuple(image_shape)}")
        rows_status = torch.zeros(n, dtype=torch.int32, device=device)
        reconstruction = self._decompress_device(K, idx, seed, image_shape, sampler, rows_status)
        joined = join_status(rec_status, words, header_want(seed, (n, 3, height, width), self.n_levels, device), rows_status)
        return finish(reconstruction, joined.cpu().numpy(), strict)


class Large2LevelVAE(_LevelsVAE):
    _ideal_tags = (2, 1)                                                       # file order: level 2, then level 1

    def __init__(self, level_1_filters=196, level_2_filters=128, name="large_level_2_vae", **kwargs):
        super().__init__()
        self.level_1_filters, self.level_2_filters = level_1_filters, level_2_filters
        f1, f2 = level_1_filters, level_2_filters
        self.analysis_transform = _down(3, 2 * f1, 4)                      # -> loc | log_scale, H/16
        self.hyper_analysis_transform = _down(f1, 2 * f2, 2)               # -> loc | log_scale, H/64
        self.hyper_synthesis_transform = _up(f2, f1, 2 * f1, 2)            # -> level-1 prior loc | log_scale
        self.synthesis_transform = _up(f1, f1, 3, 4)
        self._prior_base = nn.Parameter(torch.zeros(1, f2, 1, 1))
        self._prior_conv = nn.Conv2d(f2, f2, 3, padding=1)
        self._prior_loc_head = nn.Conv2d(f2, f2, 3, padding=1)
        self._prior_log_scale_head = nn.Conv2d(f2, f2, 3, padding=1)
        self._level_1_posterior_loc_combiner = nn.Conv2d(2 * f1, f1, 1)
        self._level_1_posterior_log_scale_combiner = nn.Conv2d(2 * f1, f1, 1)

    def prior_base(self, batch_size, height, width):
        """large_2_level_vae.py:312-313."""
        return self._prior_base.expand(batch_size, -1, height // 64, width // 64).contiguous()

    def _latent_dims(self, h, w):
        return [(h // 64) * (w // 64) * self.level_2_filters, (h // 16) * (w // 16) * self.level_1_filters]

    def _level_2_prior(self, batch_size, height, width):
        t = F.elu(self._prior_conv(self.prior_base(batch_size, height, width)))
        return self._prior_loc_head(t), F.softplus(self._prior_log_scale_head(t)) + 1e-7

    def _level_1_prior(self, level_2_latent):
        loc, log_scale = torch.chunk(self.hyper_synthesis_transform(level_2_latent), 2, dim=1)
        return loc, F.softplus(log_scale) + 1e-7, log_scale

    def _code_levels(self, tensor, sampling_fn):
        """`forward` up to the coded level-1 sample: ([level_2_indices, level_1_indices], y NHWC)."""
        batch_size, _, height, width = tensor.shape
        l1_post_loc, l1_post_log_scale = torch.chunk(self.analysis_transform(tensor), 2, dim=1)
        l2_post_loc, l2_post_log_scale = torch.chunk(self.hyper_analysis_transform(l1_post_loc), 2, dim=1)
        self.level_2_posterior = _Normal(_nhwc(l2_post_loc), _nhwc(F.softplus(l2_post_log_scale) + 1e-7))
        l2_prior_loc, l2_prior_scale = self._level_2_prior(batch_size, height, width)
        self.level_2_prior = _Normal(_nhwc(l2_prior_loc), _nhwc(l2_prior_scale))
        level_2_indices, z = sampling_fn(target=self.level_2_posterior, coder=self.level_2_prior)            # :359-360
        l1_prior_loc, l1_prior_scale, l1_prior_log_scale = self._level_1_prior(_nchw(z))
        loc = self._level_1_posterior_loc_combiner(F.elu(torch.cat([l1_post_loc, l1_prior_loc], dim=1)))
        log_scale = self._level_1_posterior_log_scale_combiner(F.elu(torch.cat([l1_post_log_scale, l1_prior_log_scale], dim=1)))
        self.level_1_prior = _Normal(_nhwc(l1_prior_loc), _nhwc(l1_prior_scale))
        self.level_1_posterior = _Normal(_nhwc(loc), _nhwc(F.softplus(log_scale) + 1e-7))
        level_1_indices, y = sampling_fn(target=self.level_1_posterior, coder=self.level_1_prior)            # :394-395
        return [level_2_indices, level_1_indices], y

    def _decode_levels(self, n, height, width, decode):
        """large_2_level_vae.py:430-451."""
        l2_prior_loc, l2_prior_scale = self._level_2_prior(n, height, width)
        self.level_2_prior = _Normal(_nhwc(l2_prior_loc), _nhwc(l2_prior_scale))
        z = decode(self.level_2_prior, 0)                                                                     # :441
        l1_prior_loc, l1_prior_scale, _ = self._level_1_prior(_nchw(z))
        self.level_1_prior = _Normal(_nhwc(l1_prior_loc), _nhwc(l1_prior_scale))
        return decode(self.level_1_prior, 1)                                                                  # :451


class Large1LevelVAE(_LevelsVAE):
    """The lossy driver's default model (compress_with_lossy_model.py:26, :137-140): one latent [N, H/16, W/16, num_filters].  Plain
    strided convolutions stand in for the reference's SignalConv2D / GDN stacks (only the hand-off is modelled): four stride-2 layers
    down to H/16 ending in the loc | log-scale heads, four up."""
    _ideal_tags = (3,)                                                         # (the two-level model's levels draw under 2 and 1)

    def __init__(self, num_filters=192, name="large_1_level_vae", **kwargs):
        super().__init__()
        self.num_filters = f = num_filters
        self.analysis_transform = _down(3, 2 * f, 4)                           # -> posterior loc | log_scale, H/16 (:63-70)
        self.synthesis_transform = _up(f, f, 3, 4)
        self._prior_base = nn.Parameter(torch.zeros(1, f, 1, 1))               # :125
        self._prior_conv = nn.Conv2d(f, f, 3, padding=1)
        self._prior_loc_head = nn.Conv2d(f, f, 3, padding=1)
        self._prior_log_scale_head = nn.Conv2d(f, f, 3, padding=1)

    def prior_base(self, batch_size, height, width):
        """large_1_level_vae.py:154-155."""
        return self._prior_base.expand(batch_size, -1, height // 16, width // 16).contiguous()

    def _latent_dims(self, h, w):
        return [(h // 16) * (w // 16) * self.num_filters]

    def _prior(self, batch_size, height, width):
        """large_1_level_vae.py:177-186 (and :229-237)."""
        t = F.elu(self._prior_conv(self.prior_base(batch_size, height, width)))
        return _Normal(_nhwc(self._prior_loc_head(t)), _nhwc(F.softplus(self._prior_log_scale_head(t))))

    def _code_levels(self, tensor, sampling_fn):
        """`forward` up to the coded sample: ([indices], y NHWC) (:168-194)."""
        batch_size, _, height, width = tensor.shape
        loc, log_scale = torch.chunk(self.analysis_transform(tensor), 2, dim=1)
        self.posterior = _Normal(_nhwc(loc), _nhwc(F.softplus(log_scale)))
        self.prior = self._prior(batch_size, height, width)
        indices, y = sampling_fn(target=self.posterior, coder=self.prior)                                     # :193-194
        return [indices], y

    def _decode_levels(self, n, height, width, decode):
        self.prior = self._prior(n, height, width)
        return decode(self.prior, 0)                                                                          # :240
