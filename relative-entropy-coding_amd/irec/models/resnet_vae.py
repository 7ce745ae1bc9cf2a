"""PyTorch-ROCm host shim of the reference's bidirectional ResNet VAE (rec/models/resnet_vae.py) -- ONLY what the
compression path touches: the block / model constructors with the reference's keyword surface, the inference pass,
and the sequential generative pass that hands each residual block's posterior and prior to `coder.encode`
(resnet_vae.py:462-476, 803-836) or `coder.decode`.

Not a re-implementation of the model family: the convolutions are stock `torch.nn.Conv2d` (the reference's
weight-normalised `ReparameterizedConv2D` with data-dependent init, IAF posteriors, likelihoods, EMA and training are
out of scope -- no checkpoints or datasets exist in the reference tree), so weights are random-init.  What
the shim pins is the hand-off: tensors are presented to the coder in the reference's NHWC order, the residual blocks
are coded strictly in sequence (the prior of block n+1 depends on the coded latent of block n), and the keyword
arguments (`sampler`, `sampler_args`, `coder_args`, `kl_per_partition`, `encoder_args`, `decoder_args`) keep their
names and meaning.  Beside the compression path there is the evaluation script's sampling pass, `forward(images, seed)` with
`kl_divergence()` and `log_likelihood` (resnet_vae.py:687-750), its draws seeded and made on the device (irec.ideal).
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib
from ..coding import BeamSearchCoder, CodingError, GaussianCoder, ImportanceSampler
from ..coding.beam_search_coder import MorePartitionsNeeded, PendingCode, SplitNotResident
from ..coding.pending import recode
from ._rec_rows import STATUS_HEADER, STATUS_SEGMENTED, STATUS_TABLE  # noqa: F401  (the joined status's names are read from this module)
from ._rec_rows import STATUS_RESIDUAL, STATUS_ROWS, finish, header_want, join_status, packed_rows, raise_status, read_rows, status_text


class ModelError(Exception):
    """rec/models/resnet_vae.py (ModelError)."""


class deterministic_transforms:
    """Encoder and decoder must evaluate the SAME bits for every prior: a relative-entropy code is only decodable if the
    decoder's coding distribution equals the encoder's exactly.  MIOpen may pick different (or atomically accumulating)
    convolution algorithms from call to call, so compress / decompress pin the deterministic ones for their duration."""

    def __enter__(self):
        self._prev = (torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark)
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
        return self

    def __exit__(self, *exc):
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = self._prev
        return False


class _HandOff:
    """The elementwise hand-offs between the shim's convolutions and the coder as ONE launch each (csrc/irec_shim.hip:
    irec_shim_stats / _cat_elu / _residual_elu) instead of ~10 PyTorch launches of 3-5 us per residual block and pass.
    CUDA float32 contiguous tensors only; anything else takes the plain PyTorch ops (the coder itself has no CPU path)."""

    @staticmethod
    def ok(*tensors):
        return all(t is not None and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() for t in tensors)

    @staticmethod
    def _eng(t):
        from ..engine import get_engine
        return get_engine(t.device)

    @staticmethod
    def _p(t):
        import ctypes
        return ctypes.c_void_p(t.data_ptr() if t is not None else 0)

    @staticmethod
    def stats(y, infer_y, s, n_stats, bias_y=None, bias_infer=None):
        """[n_stats, N, H, W, s]: prior loc, prior scale (, posterior loc, posterior scale) in the coder's NHWC order.
        bias_*: the (not yet added) biases of the convolutions behind y / infer_y."""
        from .. import _lib
        n, cy, h, w = y.shape
        out = torch.empty((n_stats, n, h, w, s), dtype=torch.float32, device=y.device)
        eng = _HandOff._eng(y)
        _lib.check(eng.lib.irec_shim_stats(eng.ctx, _HandOff._p(y), _HandOff._p(infer_y), _HandOff._p(out), n_stats, n, cy,
                                           infer_y.shape[1] if infer_y is not None else 0, s, h * w, _HandOff._p(bias_y),
                                           _HandOff._p(bias_infer), eng._stream()), "irec_shim_stats")
        return out

    @staticmethod
    def cat_elu(y, c_off, d, latent_nhwc, bias_y=None):
        """elu(cat(y[:, c_off:c_off + d] (+ bias), latent NHWC -> NCHW)); latent None: the ELU of the channel slice."""
        from .. import _lib
        n, cy, h, w = y.shape
        s = 0 if latent_nhwc is None else latent_nhwc.shape[-1]
        out = torch.empty((n, d + s, h, w), dtype=torch.float32, device=y.device)
        eng = _HandOff._eng(y)
        _lib.check(eng.lib.irec_shim_cat_elu(eng.ctx, _HandOff._p(y), _HandOff._p(latent_nhwc if s else None), _HandOff._p(out),
                                             n, cy, c_off, d, s, h * w, _HandOff._p(bias_y), eng._stream()), "irec_shim_cat_elu")
        return out

    @staticmethod
    def residual_elu(inp, t, alpha, bias_t=None):
        """(inp + alpha * (t + bias), elu of it)"""
        from .. import _lib
        out, out_elu = torch.empty_like(inp), torch.empty_like(inp)
        n, c, h, w = inp.shape
        eng = _HandOff._eng(inp)
        _lib.check(eng.lib.irec_shim_residual_elu(eng.ctx, _HandOff._p(inp), _HandOff._p(t), float(alpha), _HandOff._p(out),
                                                  _HandOff._p(out_elu), n, c, h * w, _HandOff._p(bias_t), eng._stream()),
                   "irec_shim_residual_elu")
        return out, out_elu


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


class _Normal:
    """Duck-typed distribution: the coder reads only .loc and .scale (coder.py:427-430)."""

    def __init__(self, loc, scale):
        self.loc, self.scale = loc, scale


class BidirectionalResidualBlock(nn.Module):
    """resnet_vae.py:20-497 (compression-relevant subset)."""

    def __init__(self, stochastic_filters, deterministic_filters, sampler, sampler_args={}, coder_args={},
                 distribution="gaussian", kernel_size=(3, 3), use_iaf=False, is_last=False, kl_per_partition=8.,
                 use_sig_convs=False, name="bidirectional_resnet_block", **kwargs):
        super().__init__()
        if distribution != "gaussian":
            raise ValueError("Distribution must be 'gaussian' on the beam-search path, "
                             f"but {distribution} was given!")
        if use_iaf or use_sig_convs:
            raise ModelError("IAF posteriors / SignalConv2D are outside the compression shim")
        self.name = name
        self.stochastic_filters, self.deterministic_filters = stochastic_filters, deterministic_filters
        self.is_last = is_last
        pad = (kernel_size[0] // 2, kernel_size[1] // 2)

        def conv(cin, cout):
            return nn.Conv2d(cin, cout, kernel_size, padding=pad)

        d, s = deterministic_filters, stochastic_filters
        if not is_last:
            self.infer_conv1, self.infer_conv2 = conv(d, d), conv(d, d)
        self.infer_posterior_loc_head, self.infer_posterior_log_scale_head = conv(d, s), conv(d, s)
        self.gen_conv1, self.gen_conv2 = conv(d, d), conv(d + s, d)
        self.prior_loc_head, self.prior_log_scale_head = conv(d, s), conv(d, s)
        self.gen_posterior_loc_head, self.gen_posterior_log_scale_head = conv(d, s), conv(d, s)
        self._infer_y = self._infer_bias = self._infer_heads = None   # inference pass's head convolution (and its pending bias)
        # Hand-off kernels (csrc/irec_shim.hip) or plain torch ops between the convolutions and the coder: decided ONCE per block --
        # None: by where the block lives (a float32 CUDA block takes the kernels) -- and identically in compress and decompress,
        # never per tensor: the kernels' expf / expm1f and torch.exp / F.elu differ in the last ulp, so an encoder and a decoder
        # that chose differently would rebuild different prior scales and the reconstruction would silently diverge.  Inputs
        # the kernels cannot take as they are (non-contiguous, channels_last) are made contiguous, not routed around them.
        self.use_handoff_kernels = None
        self.posterior = self.prior = None
        self.index = 0       # the block's number in its model: the `tag` of its seeded posterior draws (the model sets it)
        self.kl = None       # float64 [N]: KL(posterior || prior) per image of the last seeded sampling pass (irec.ideal.posterior_draw)
        self._pad = pad
        self._fused = None   # (parameter versions, inference-side weight / bias, generative-side weight / bias)
        self._fuse_mods = None
        # ---- stuff for compression (resnet_vae.py:118-141) ----
        if sampler == "beam_search":
            self.coder = BeamSearchCoder(kl_per_partition=kl_per_partition, n_beams=sampler_args['n_beams'],
                                         extra_samples=sampler_args['extra_samples'], name=f"encoder_for_{self.name}",
                                         **coder_args)
        elif sampler == "importance":                      # resnet_vae.py:126-131
            self.coder = GaussianCoder(kl_per_partition=kl_per_partition, sampler=ImportanceSampler(**sampler_args),
                                       name=f"encoder_for_{self.name}", **coder_args)
        elif sampler == "rejection":
            raise ModelError(f"sampler '{sampler}' is outside the beam-search and importance paths of this build")
        else:
            raise ModelError("Sampler must be one of ['rejection', 'importance', 'beam_search'],"
                             f"but got {sampler}!")

    @property
    def infer_posterior_loc(self):
        """Inference-side posterior loc head (resnet_vae.py: infer_posterior_loc; 0. before an inference pass, as there).  On the
        kernel path the head convolution runs without its bias (the hand-off kernel adds it): the view is biased lazily."""
        return self._infer_head(0)

    @property
    def infer_posterior_log_scale(self):
        return self._infer_head(1)

    def _infer_head(self, k):
        if self._infer_y is None:
            return 0.
        s = self.stochastic_filters
        v = self._infer_y[:, k * s:(k + 1) * s]
        return v if self._infer_bias is None else v + self._infer_bias[k * s:(k + 1) * s].reshape(1, -1, 1, 1)

    def _handoff(self, *tensors):
        """Whether this block's passes take the hand-off kernels: the explicit flag, else float32-on-CUDA of the block ITSELF -- decided
        by the block's own parameters, identically in compress and decompress, never by the activations of one call (round 5: a
        decompress whose activations arrived in another dtype or on another device used to take the torch path silently, and
        torch.exp / F.elu differ from the kernels' expf / expm1f in the last ulp: the prior scales, and with them the reconstruction,
        diverged).  Activations that disagree with the block are an error."""
        w = self.gen_conv1.weight
        use = bool(self.use_handoff_kernels) if self.use_handoff_kernels is not None else (w.is_cuda and w.dtype == torch.float32)
        if use and not all(t is None or (t.is_cuda and t.dtype == torch.float32 and t.device == w.device) for t in tensors):
            raise ModelError("this residual block runs its hand-off kernels (float32 parameters on a HIP device): its activations must be "
                             "float32 on that device too, in compress and decompress alike")
        return use

    @property
    def posterior_loc(self):
        """resnet_vae.py: infer_posterior_loc + gen_posterior_loc (the sum is formed in place in `forward`)."""
        return _nchw(self.posterior.loc)

    @property
    def posterior_scale(self):
        return _nchw(self.posterior.scale)

    def _fused_weights(self):
        """The convolutions that read the same activation, as ONE convolution each (output channels concatenated):
        inference side = posterior heads (loc, log-scale) + infer_conv1; generative side = prior heads, posterior heads
        + gen_conv1.  Ten convolutions per residual block become four -- on a 16x16 latent grid each one is a
        launch-bound im2col + GEMM pair, and a single image spends more time in them than in the coder.  The compress and
        the decompress pass both run the SAME generative-side convolution (the decoder drops the posterior channels), so
        the prior the decoder rebuilds is bit-identical to the one the encoder coded against.  Rebuilt when a parameter
        changes in place, is replaced or moves (tensor version counters and storage addresses)."""
        mods = self._fuse_mods
        if mods is None:   # (looked up once: nn.Module attribute access is a microsecond each, and this runs 48 times per image)
            heads_i = [self.infer_posterior_loc_head, self.infer_posterior_log_scale_head] + ([] if self.is_last else [self.infer_conv1])
            heads_g = [self.prior_loc_head, self.prior_log_scale_head, self.gen_posterior_loc_head,
                       self.gen_posterior_log_scale_head, self.gen_conv1]
            mods = self._fuse_mods = (heads_i, heads_g)
        heads_i, heads_g = mods
        ver = [x for m in heads_i + heads_g for p in (m._parameters["weight"], m._parameters["bias"])
               for x in (id(p), p._version, p.data_ptr())]
        if self._fused is None or self._fused[0] != ver:
            with torch.no_grad():
                self._fused = (ver,
                               torch.cat([m.weight for m in heads_i]).contiguous(), torch.cat([m.bias for m in heads_i]).contiguous(),
                               torch.cat([m.weight for m in heads_g]).contiguous(), torch.cat([m.bias for m in heads_g]).contiguous())
        return self._fused[1:]

    def update_coders(self, **fit_args):
        """resnet_vae.py:497-499: fit the coder's auxiliary variance ratios to the posterior / prior of the last pass."""
        if self.posterior is None or self.prior is None:
            raise ModelError(f"{self.name}: update_coders needs the posterior and prior of a pass over some images first")
        self.coder.update_auxiliary_variance_ratios(target_dist=self.posterior, coding_dist=self.prior, **fit_args)

    def forward(self, tensor, inference_pass=True, encoder_args=None, decoder_args=None, sample_args=None):
        """resnet_vae.py:372-497.  sample_args={"generator": g}: the generative pass of the reference's `call` -- the latent is a
        draw from the posterior (standard normals from the CPU generator g), nothing is coded; it leaves the block's posterior and
        prior in place for update_coders.  sample_args={"seed": s, "image_base": b}: the same pass with the draw made where the
        statistics are (irec.ideal.posterior_draw with tag = the block's index: the library's own seeded stream, image i of the batch
        drawing as image b + i), no host round trip; it also leaves self.kl, float64 [N], the block's KL per image."""
        inp = tensor
        pre = getattr(tensor, "_irec_elu", None)          # the previous block's residual kernel already formed elu(tensor)
        tensor = pre if pre is not None else F.elu(tensor)
        indices = None
        s, d = self.stochastic_filters, self.deterministic_filters
        w_i, b_i, w_g, b_g = self._fused_weights()
        # On the fused path the convolutions run WITHOUT their bias: the hand-off kernel that reads a convolution's output adds
        # it first (same operation, same order, one launch fewer per convolution: 96 per image).
        fused = self._handoff(inp, tensor)                 # one decision per block: the same in compress and decompress
        if fused:
            inp, tensor = inp.contiguous(), tensor.contiguous()
        bias2 = None
        if inference_pass:
            y = F.conv2d(tensor, w_i, None if fused else b_i, padding=self._pad)   # [N, 2s (+ d), H, W]
            if fused:
                y = y.contiguous()
            self._infer_y, self._infer_bias = y, (b_i if fused else None)
            self._infer_heads = None if fused else y[:, :2 * s]     # (infer_posterior_loc / _log_scale: lazily biased views)
            if not self.is_last:
                if fused:
                    tensor = F.conv2d(_HandOff.cat_elu(y, 2 * s, d, None, b_i), self.infer_conv2.weight, None, padding=self._pad)
                    bias2 = self.infer_conv2.bias
                else:
                    tensor = self.infer_conv2(F.elu(y[:, 2 * s:]))
        else:
            if encoder_args is None and decoder_args is None and sample_args is None:
                raise ModelError("training / sampling passes are outside the compression shim")
            if (encoder_args is not None or sample_args is not None) and self._infer_y is None:
                raise ModelError(f"{self.name}: a compression pass needs the statistics of an inference pass over the same input first")
            if (encoder_args is not None or sample_args is not None) and fused != (self._infer_bias is not None):
                raise ModelError(f"{self.name}: use_handoff_kernels changed between the inference and the generative pass")
            y = F.conv2d(tensor, w_g, None if fused else b_g, padding=self._pad)  # [N, 4s + d, H, W]
            if fused:
                y = y.contiguous()
            n, _, h, w = y.shape
            if encoder_args is not None or sample_args is not None:               # :462-470
                if fused:
                    st = _HandOff.stats(y, self._infer_y, s, 4, b_g, self._infer_bias)   # all four statistics, NHWC, one launch
                else:
                    y[:, 2 * s:4 * s] += self._infer_heads                                   # posterior loc / log-scale = inference + generative
                    st = y[:, :4 * s].view(n, 4, s, h, w).permute(1, 0, 3, 4, 2).contiguous()   # coder sees NHWC, as in the reference
                    st[1::2].exp_()                                               # the two scales
                self.prior, self.posterior = _Normal(st[0], st[1]), _Normal(st[2], st[3])
                if encoder_args is not None:
                    indices, latent_code = self.coder.encode(self.posterior, self.prior, **encoder_args)
                elif "seed" in sample_args:                                       # :471-473, posterior.sample(), seeded on the device
                    from .. import ideal
                    latent_code, self.kl = ideal.posterior_draw(self.posterior, self.prior, sample_args["seed"], self.index,
                                                                sample_args.get("image_base", 0))
                else:                                                             # :471-473, posterior.sample()
                    noise = torch.randn(self.posterior.loc.shape, generator=sample_args["generator"], dtype=torch.float32)
                    latent_code = self.posterior.loc + self.posterior.scale * noise.to(self.posterior.loc.device)
            else:                                                                 # :475-476
                if fused:
                    st = _HandOff.stats(y, None, s, 2, b_g)                       # the SAME kernel and exp as the encoder's prior
                else:
                    st = y[:, :2 * s].view(n, 2, s, h, w).permute(1, 0, 3, 4, 2).contiguous()
                    st[1].exp_()
                self.prior = _Normal(st[0], st[1])
                latent_code = self.coder.decode(self.prior, **decoder_args)
            if fused:
                latent_code = latent_code.to(dtype=torch.float32).contiguous()
                tensor = F.conv2d(_HandOff.cat_elu(y, 4 * s, d, latent_code, b_g), self.gen_conv2.weight, None, padding=self._pad)
                bias2 = self.gen_conv2.bias
            else:
                tensor = torch.cat([y[:, 4 * s:], latent_code.permute(0, 3, 1, 2)], dim=1)
                tensor = self.gen_conv2(F.elu(tensor, inplace=True))
        if fused:
            tensor, tensor_elu = _HandOff.residual_elu(inp, tensor.contiguous(), 0.1, bias2)
            tensor._irec_elu = tensor_elu                  # (a Python attribute: the next block, or _finish, picks it up)
        else:
            tensor = torch.add(inp, tensor, alpha=0.1)
        if encoder_args is not None:
            return indices, tensor
        return tensor


class BidirectionalResNetVAE(nn.Module):
    """resnet_vae.py:512-860 (compression-relevant subset)."""

    def __init__(self, num_res_blocks, sampler, sampler_args={}, coder_args={}, likelihood_function="discretized_logistic",
                 learn_likelihood_scale=True, first_kernel_size=(5, 5), first_strides=(2, 2), kernel_size=(3, 3),
                 strides=(1, 1), deterministic_filters=160, stochastic_filters=32, use_iaf=False, kl_per_partition=8.,
                 latent_size="variable", ema_decay=0.999, name="resnet_vae", **kwargs):
        super().__init__()
        self.sampler_name = str(sampler)
        self.num_res_blocks = num_res_blocks
        self.deterministic_filters, self.stochastic_filters = deterministic_filters, stochastic_filters
        self.kl_per_partition = kl_per_partition
        pad = (first_kernel_size[0] // 2, first_kernel_size[1] // 2)
        self.first_infer_conv = nn.Conv2d(3, deterministic_filters, first_kernel_size, stride=first_strides, padding=pad)
        self.last_gen_conv = nn.ConvTranspose2d(deterministic_filters, 3, first_kernel_size, stride=first_strides,
                                                padding=pad, output_padding=(first_strides[0] - 1, first_strides[1] - 1))
        self.residual_blocks = nn.ModuleList([
            BidirectionalResidualBlock(stochastic_filters=stochastic_filters, deterministic_filters=deterministic_filters,
                                       sampler=self.sampler_name, sampler_args=sampler_args, coder_args=coder_args,
                                       kernel_size=kernel_size, is_last=res_block_idx == 0, use_iaf=use_iaf,
                                       kl_per_partition=kl_per_partition, name=f"resnet_block_{res_block_idx}")
            for res_block_idx in range(num_res_blocks)])
        for res_block_idx, block in enumerate(self.residual_blocks):
            block.index = res_block_idx
        self.likelihood_function_name = str(likelihood_function)   # (only `forward` reads it: the one family its likelihood term is built for)
        self.log_likelihood = None                                 # float64 [N] of the last `forward`
        self._generative_base = nn.Parameter(torch.zeros(deterministic_filters))
        # resnet_vae.py:581: the log of the discretized-logistic likelihood's one scale (the .res coder's model, compress_lossless).
        # Created after every other parameter and without a random draw: no existing initialisation moves.
        self.likelihood_log_scale = nn.Parameter(torch.zeros(()))
        self._likelihood_scale_cache = None
        # One log-scale per colour channel, or None (the scalar parameter above holds): a buffer that is absent from state_dict()
        # while it is None, so a model without per-channel scales keeps its keys.  set_likelihood_scales / fit_likelihood_scale set it.
        self.register_buffer("likelihood_log_scales", None)
        self._likelihood_scales_cache = None

    def generative_base(self, batch_size, height, width):
        """resnet_vae.py:619-623."""
        return self._generative_base.reshape(1, -1, 1, 1).expand(batch_size, -1, height // 2, width // 2).contiguous()

    def _finish(self, tensor):
        pre = getattr(tensor, "_irec_elu", None)
        reconstruction = self.last_gen_conv(pre if pre is not None else F.elu(tensor))
        return torch.clamp(reconstruction, -0.5 + 1. / 512., 0.5 - 1. / 512.)

    @torch.no_grad()
    def forward(self, images, seed, image_base=0, binsize=1. / 256.):
        """resnet_vae.py:687-727, the reference's `call` as its evaluation script uses it (`model(image)`): the inference pass, the
        generative pass with every latent DRAWN from its posterior, the clipped reconstruction; returns reconstruction + 0.5.
        images: [N, 3, H, W] in [-0.5, 0.5].  The reference's draws are unseeded; these are seeded (irec.ideal.posterior_draw: seed,
        tag = the residual block's index, image i drawing as image number image_base + i), made on the device with no host round trip.
        Leaves self.log_likelihood, float64 [N] in nats PER IMAGE (the reference's scalar attribute is the mean of these over the
        batch), under the scalar likelihood_log_scale or, when they are set, the per-channel likelihood_log_scales; and every block's
        kl for kl_divergence().  Nothing is read back.  Only likelihood_function='discretized_logistic' is built."""
        from .. import ideal
        if self.likelihood_function_name != "discretized_logistic":
            raise ModelError(f"forward: the likelihood term is built for 'discretized_logistic' only, not for '{self.likelihood_function_name}'")
        batch_size, _, height, width = images.shape
        sample_args = {"seed": seed, "image_base": image_base}
        with deterministic_transforms():
            tensor = self.first_infer_conv(images)
            for resnet_block in list(self.residual_blocks)[::-1]:
                tensor = resnet_block(tensor, inference_pass=True)
            tensor = self.generative_base(batch_size=batch_size, width=width, height=height)
            for resnet_block in self.residual_blocks:
                tensor = resnet_block(tensor, inference_pass=False, sample_args=sample_args)
            reconstruction = self._finish(tensor)
        log_scale = self.likelihood_log_scale if self.likelihood_log_scales is None else self.likelihood_log_scales
        self.log_likelihood = ideal.log_likelihood(images, reconstruction, log_scale, binsize)
        return reconstruction + 0.5

    def kl_divergence(self, reduce=True):
        """resnet_vae.py:729-750 for the last `forward`: float64 [N], the sum over the residual blocks of an image's KL in nats;
        reduce=False: the list of the blocks' [N]."""
        kls = [block.kl for block in self.residual_blocks]
        if any(kl is None for kl in kls):
            raise ModelError("kl_divergence needs a forward(images, seed) pass first")
        return torch.stack(kls).sum(dim=0) if reduce else kls

    @torch.no_grad()
    def coded_kl(self):
        """float64 [N]: the KL of the posteriors and priors that the last pass left in the residual blocks (after a compress pass: the
        distributions the indices were coded under), through the kernel of irec.ideal.posterior_draw (its sample is dropped)."""
        from .. import ideal
        if any(block.posterior is None or block.prior is None for block in self.residual_blocks):
            raise ModelError("coded_kl needs the posteriors and priors of a pass over some images first")
        return torch.stack([ideal.posterior_draw(block.posterior, block.prior, 0, block.index)[1] for block in self.residual_blocks]).sum(dim=0)

    @torch.no_grad()
    def update_coders(self, images, seed=42, **fit_args):
        """resnet_vae.py:795-801: a forward pass over `images` ([N, 3, H, W]) sets the posterior and prior of every residual block
        (the latents are posterior draws, seeded by `seed`), then every block's coder fits its auxiliary variance ratios to them
        (GaussianCoder.update_auxiliary_variance_ratios; fit_args: relative_tolerance, max_iters, learning_rate)."""
        batch_size, _, height, width = images.shape
        with deterministic_transforms():
            tensor = self.first_infer_conv(images)
            for resnet_block in list(self.residual_blocks)[::-1]:
                tensor = resnet_block(tensor, inference_pass=True)
            tensor = self.generative_base(batch_size=batch_size, width=width, height=height)
            generator = torch.Generator().manual_seed(int(seed))
            for resnet_block in self.residual_blocks:
                tensor = resnet_block(tensor, inference_pass=False, sample_args={"generator": generator})
        for resnet_block in self.residual_blocks:
            resnet_block.update_coders(seed=seed, **fit_args)

    @torch.no_grad()
    def compress(self, image, seed, update_sampler=False):
        """resnet_vae.py:803-836.  image: [N, 3, H, W] in [-0.5, 0.5].  Returns (block_indices, reconstruction).

        N = 1 (the reference's only case): block_indices[res_block][coder_block] = list of indices, as the reference returns.
        N > 1 (extension): the N images go through every residual block together -- one coder launch per residual block
        for all of them -- and block_indices[image][res_block][coder_block].
        Nothing is copied to the host until the last residual block has been coded: each block's `coder.encode(...,
        defer=True)` leaves its K / index rows on the device and hands the merged sample straight to the next block's
        convolutions; ONE device-to-host copy then fetches all indices of all blocks and images."""
        per_block, reconstruction = self._recode(image, seed, update_sampler, PendingCode.gather)   # [res_block][image][coder_block]; the only host sync
        return self._indices_structure(per_block, image.shape[0]), reconstruction

    @torch.no_grad()
    def compress_packed(self, image, seed, update_sampler=False):
        """`compress` for a batch, with the indices left packed: (K [N, R, bpt], idx [N, R, bpt, max_K] int32 numpy arrays,
        reconstruction) -- what irec.io.encode_files turns into N .rec files without one Python object per index.  Needs every
        residual block to share one block layout (they do: same latent shape and block_size)."""
        (K, idx), reconstruction = self._recode(image, seed, update_sampler, PendingCode.gather_packed)
        return K, idx, reconstruction

    @torch.no_grad()
    def compress_rec(self, image, seed, update_sampler=False, block_size=None, return_pendings=False, tables=None, segment_blocks=None):
        """`compress_packed` with the indices never leaving the device: (blob uint8, offsets int64 [N + 1], reconstruction), CUDA tensors
        -- image i's .rec file is blob[offsets[i]:offsets[i + 1]], byte for byte what irec.io.encode_files makes of compress_packed's
        arrays (irec.io.encode_files_device: the arithmetic coder runs on the device, one lane per stream).  Only the partition counts
        and the files' offsets are read back.  block_size: the header's block-size word (default: the coders' own).
        return_pendings: also the device K / idx views the files were built from, ((blob, offsets, reconstruction), (K, idx)).
        tables: an irec.io.SymbolTables (harness.fit_symbol_tables) -- the streams coded under its count tables, the files flagged as
        the reference's writer flags them; decompress_rec needs the same tables.
        segment_blocks: None for the reference's file; g >= 1 for the segmented container (NAME.recs, INTEGRATION.md §8: every residual
        block's rows in segments of g coder blocks, one lane per stream of a segment -- irec.io.encode_files_device_segmented), which
        decompress_rec_segmented reads.  Default symbol models only: together with tables it is a ValueError."""
        from ..io import encode_files_device, encode_files_device_segmented, header_seed
        from ..io.utils import _block_rows
        seed = header_seed(seed, "compress_rec")           # (before anything is coded: the files could not name another seed)
        if segment_blocks is not None and tables is not None:
            raise ValueError("compress_rec: the segmented container codes under the default symbol models only (tables= with segment_blocks=)")
        _, _, height, width = image.shape
        (K, idx), reconstruction = self._recode(image, seed, update_sampler, PendingCode.gather_packed_device)
        coder = self.residual_blocks[0].coder
        # the header's max_index word: the samples a step chooses among (the sequential coder's are its sampler's)
        n_samples = coder.sampler.n_samples() if coder.sampler is not None else coder.n_samples
        block_size = coder.block_size if block_size is None else block_size
        if segment_blocks is not None:
            blob, offsets = encode_files_device_segmented(seed, (height, width, 3), block_size, *_block_rows(K, idx), n_samples,
                                                          [K.shape[2]] * K.shape[1], segment_blocks)
        else:
            blob, offsets = encode_files_device(seed, (height, width, 3), block_size, K, idx, max_index=n_samples, tables=tables)
        return ((blob, offsets, reconstruction), (K, idx)) if return_pendings else (blob, offsets, reconstruction)

    def _recode(self, image, seed, update_sampler, gather):
        """(gather(pendings), reconstruction) of a device pass that `gather` reads back whole (irec.coding.pending.recode)."""
        return recode(lambda: self._compress_device(image, seed, update_sampler), gather, [b.coder for b in self.residual_blocks])

    def _compress_device(self, image, seed, update_sampler=False):
        """Everything of `compress` that runs on the device, with no host synchronisation: (PendingCode per residual
        block, reconstruction).  Capturable in a HIP graph (GraphedCompress)."""
        batch_size, _, height, width = image.shape
        with deterministic_transforms():
            tensor = self.first_infer_conv(image)
            for resnet_block in list(self.residual_blocks)[::-1]:         # inference pass, reverse order (:811-813)
                tensor = resnet_block(tensor, inference_pass=True)
            tensor = self.generative_base(batch_size=batch_size, width=width, height=height)
            pendings = []
            # every residual block codes with the same seed, S and block dims (:822-824): with ONE table window for all of them
            # the proposal tables of the first block serve the other 23 (IREC_FLAG_REUSE_TABLES)
            # (one max_K too: it bounds the window, and a window that covers max_K leaves no second pass to launch -- built
            #  once per image, a long window costs next to nothing)
            max_K = max(blk.coder._max_K_hint for blk in self.residual_blocks)
            window = max(max(blk.coder.table_window() for blk in self.residual_blocks), min(max_K, 64))
            from ..engine import get_engine
            with get_engine(tensor.device).table_session():              # twin calls back to back: no table launches after the first
                for resnet_block in self.residual_blocks:                 # strictly sequential (:821-826)
                    pending, tensor = resnet_block(tensor, inference_pass=False,
                                                   encoder_args={"seed": seed, "update_sampler": update_sampler, "batched": True,
                                                                 "defer": True, "table_steps": window, "max_K": max_K})
                    pendings.append(pending)
            return pendings, self._finish(tensor)

    def _indices_structure(self, per_block, batch_size):
        flat = [blk.coder.block_size is None for blk in self.residual_blocks]   # no block_size: one index list per tensor
        per_block = [[img[0] if flat[r] else img for img in blk] for r, blk in enumerate(per_block)]
        if batch_size == 1:
            return [blk[0] for blk in per_block]
        return [[blk[i] for blk in per_block] for i in range(batch_size)]

    @torch.no_grad()
    def decompress(self, block_indices, seed, image_shape):
        """The generative pass driven by the stored indices.  (The reference's own decompress, resnet_vae.py:844-860,
        is an unfinished stub; this is the pass its decoder_args plumbing implies.)  image_shape[0] = N > 1 takes the
        batched form of `compress`'s block_indices."""
        batch_size, _, height, width = image_shape
        with deterministic_transforms():
            tensor = self.generative_base(batch_size=batch_size, width=width, height=height)
            for r, resnet_block in enumerate(self.residual_blocks):
                if batch_size == 1:
                    args = {"seed": seed, "indices": block_indices[r]}
                else:
                    args = {"seed": seed, "indices": [block_indices[i][r] for i in range(batch_size)], "batched": True}
                tensor = resnet_block(tensor, inference_pass=False, decoder_args=args)
            return self._finish(tensor)

    # ---- the read side on the device: rows that never leave it, one read-back per batch -----------------------------------------
    def blocks_per_tensor(self, image_shape):
        """Coder blocks per residual block and image (Coder.split, coder.py:69-83) for images of this shape."""
        _, _, h, w = image_shape
        n = (h // 2) * (w // 2) * self.stochastic_filters
        bs = self.residual_blocks[0].coder.block_size
        return 1 if bs is None else -(-n // int(bs))

    def _decompress_device(self, K, idx, seed, image_shape, status):
        """The generative pass driven by rows on the device: K [N, R, bpt], idx [N, R, bpt, max_K] int32 (contiguous, or the views of
        one joined tensor), every residual block's coder reading its rows in place (decoder_args={"packed": ...}) and accumulating
        its verdict on them into `status` (int32 [N], device).  No host synchronisation: capturable in a HIP graph
        (GraphedDecompress)."""
        batch_size, _, height, width = image_shape
        n, R, bpt = K.shape
        if n != batch_size or R != self.num_res_blocks or tuple(idx.shape[:3]) != (n, R, bpt):
            raise ModelError(f"K {tuple(K.shape)} / idx {tuple(idx.shape)} are not [N = {batch_size}, R = {self.num_res_blocks}, bpt] and [N, R, bpt, max_K]")
        if bpt != self.blocks_per_tensor(image_shape):
            raise ModelError(f"{bpt} blocks per residual block, but images of shape {tuple(image_shape)} are coded in {self.blocks_per_tensor(image_shape)}")
        rows = packed_rows(n, [bpt] * R, K.device)
        with deterministic_transforms():
            tensor = self.generative_base(batch_size=batch_size, width=width, height=height)
            for r, resnet_block in enumerate(self.residual_blocks):
                tensor = resnet_block(tensor, inference_pass=False,
                                      decoder_args={"seed": seed, "indices": None, "batched": True, "packed": (K, idx, rows[r]),
                                                    "status": status})
            return self._finish(tensor)

    def status_text(self, status, K_image=None):
        """status_text for one image of this model; K_image (its counts [R, bpt], device or numpy): the reference's ratio-table message
        names the count of the block that set the status -- the first, in coding order, beyond the table."""
        if int(status) != STATUS_ROWS + _lib.IREC_ROWS_E_RATIO_TABLE or K_image is None:
            return status_text(status)
        counts = (K_image.cpu().numpy() if hasattr(K_image, "cpu") else np.asarray(K_image)).reshape(self.num_res_blocks, -1)
        for r, block in enumerate(self.residual_blocks):
            if block.coder.extrapolate_auxiliary_ratios:
                continue
            length = int(block.coder.aux_variable_variance_ratios.shape[0])
            beyond = counts[r][counts[r] > length]
            if beyond.size:
                return status_text(status, length, int(beyond[0]))
        return status_text(status)

    def _raise_status(self, status, K=None):
        """CodingError for the first image with a nonzero joined status (decompress_rec has the encoding), "(image i)" appended."""
        raise_status(status, lambda i, st: self.status_text(st, None if K is None else K[i]))

    def _finish_status(self, result, host, K, strict):
        return finish(result, host, strict, lambda status: self._raise_status(status, K))

    @torch.no_grad()
    def decompress_packed(self, K, idx, seed, image_shape, strict=True):
        """`decompress` for packed rows on the device (K [N, R, bpt], idx [N, R, bpt, max_K] int32 CUDA: the arrays of
        irec.io.decode_files_device, or the views of PendingCode.gather_packed_device): ONE read-back, the per-image status.
        strict: CodingError naming the first image whose rows cannot be decoded; strict=False: (reconstruction, status int32 numpy
        [N]) -- 0, or STATUS_ROWS + irec_rows_status; the images with status 0 are what they would be without the others."""
        status = torch.zeros(int(image_shape[0]), dtype=torch.int32, device=K.device)
        reconstruction = self._decompress_device(K, idx, seed, image_shape, status)
        host = status.cpu().numpy()
        return self._finish_status(reconstruction, np.where(host != 0, host + STATUS_ROWS, 0).astype(np.int32), K, strict)

    def _decompress_rec_device(self, blob, offsets, seed, image_shape, max_K, tables=None, segment_blocks=None):
        """Everything of decompress_rec that runs on the device: the three launches of the .rec reader, the header check, the pass,
        the joined status.  Returns (reconstruction, status int32 [N] on the device, K).  No host synchronisation when max_K is given."""
        from ..io.utils import _Layout
        n, R, bpt = int(image_shape[0]), self.num_res_blocks, self.blocks_per_tensor(image_shape)
        layout = _Layout(R, bpt) if tables is None and segment_blocks is None else [bpt] * R     # (one count: the reader of any R)
        words, K, idx, rec_status = read_rows(blob, offsets, layout, max_K, rec_on_device=True, tables=tables, segment_blocks=segment_blocks)
        K, idx = K.view(K.shape[0], R, bpt), idx.view(K.shape[0], R, bpt, idx.shape[2])
        rows_status = torch.zeros(n, dtype=torch.int32, device=K.device)
        reconstruction = self._decompress_device(K, idx, seed, image_shape, rows_status)
        return reconstruction, join_status(rec_status, words, header_want(seed, image_shape, R, K.device), rows_status), K

    def files_max_K(self, blob, offsets, tables=None):
        """Index slots per block that decode the files of a blob on the device: the largest max_partitions word of their headers
        (irec.io.rec_files_max_K; with count tables, those tables' largest K).  Only the 28 + 16 R header bytes of every file are
        gathered and copied to the host."""
        from ..io.utils import rec_files_max_K_device
        return rec_files_max_K_device(blob, offsets, self.num_res_blocks, tables)

    @torch.no_grad()
    def _decompress_rec_status(self, blob, offsets, seed, image_shape, max_K=None, tables=None, segment_blocks=None):
        """decompress_rec up to its read-back: (reconstruction, status int32 numpy [N], K on the device)."""
        reconstruction, joined, K = self._decompress_rec_device(blob, offsets, seed, image_shape, max_K, tables, segment_blocks)
        return reconstruction, joined.cpu().numpy(), K

    @torch.no_grad()
    def decompress_rec(self, blob, offsets, seed, image_shape, max_K=None, strict=True):
        """The inverse of compress_rec: N .rec files (blob uint8 CUDA, file i = blob[offsets[i]:offsets[i + 1]]; offsets [N + 1] on the
        device or the host) to reconstructions [N, 3, H, W], with the indices never on the host: one launch of the device reader
        (irec.io.decode_files_device's launch form), the headers checked on the device against seed / image_shape / R, the pass
        (every coder checks its rows on the device), and ONE read-back -- the per-image status:
          0 ok;  1 .. 19 irec_rec_status (include/irec.h);  STATUS_HEADER: seed, height, width, channels or R differ from the
          arguments;  STATUS_ROWS + irec_rows_status: a count or an index the coder cannot decode.  First cause in that order.
        strict: CodingError with the coder's text for the first such image, "(image i)" appended; strict=False: (reconstruction,
        status int32 numpy [N]), the images with status 0 being what they would be without the others (a refused image's rows read as
        zero partitions).  max_K: index slots per block (a file with a longer row: IREC_REC_E_MAX_K); None: the largest
        max_partitions word of the files' headers (files_max_K) -- a second, small read-back of the header bytes, which a driver that
        has the bytes on the host already (harness.decompress_images) spares by passing max_K.
        A file written under count tables (compress_rec(tables=)) has status 5 here: decompress_rec_tables reads it."""
        reconstruction, host, K = self._decompress_rec_status(blob, offsets, seed, image_shape, max_K)
        return self._finish_status(reconstruction, host, K, strict)

    @torch.no_grad()
    def decompress_rec_tables(self, blob, offsets, seed, image_shape, tables, max_K=None, strict=True):
        """decompress_rec for files written under an irec.io.SymbolTables (compress_rec(tables=)); a method of its own because
        decompress_rec's signature is pinned.  The file's header flags decide per kind of stream: a flagged kind is read under the
        call's table, or has status 5 (IREC_REC_E_COUNT_FILES) if the call brought none; a file without flags decodes under the
        default models, so one call reads both sorts.  max_K None: the largest of the headers' words and the count tables' K."""
        reconstruction, host, K = self._decompress_rec_status(blob, offsets, seed, image_shape, max_K, tables)
        return self._finish_status(reconstruction, host, K, strict)

    @torch.no_grad()
    def decompress_rec_segmented(self, blob, offsets, seed, image_shape, segment_blocks=None, max_K=None, strict=True):
        """decompress_rec for segmented files (compress_rec(segment_blocks=g), NAME.recs); a method of its own because decompress_rec's
        signature is pinned.  segment_blocks None: the word of the first file's header (a 40-byte read-back).  The segmented reader's
        own causes (irec_rec_status 20 .. 22: magic or version, directory, segment size) are STATUS_SEGMENTED + 0 .. 2 in the joined
        status.  max_K None: the largest max_part word of the files' directories."""
        if segment_blocks is None:
            from ..io.segmented import FIXED_BYTES, segment_blocks_of
            first = int(offsets[0])
            segment_blocks = segment_blocks_of(blob[first:first + FIXED_BYTES].cpu().numpy().tobytes())
            if not segment_blocks:
                raise CodingError("decompress_rec_segmented: the first file is not a segmented file (no magic, or segment_blocks 0)")
        reconstruction, host, K = self._decompress_rec_status(blob, offsets, seed, image_shape, max_K, None, segment_blocks)
        return self._finish_status(reconstruction, host, K, strict)

    # ---- the lossless pair: .rec (the latents' indices) + .res (the pixels under the likelihood given the reconstruction) ----------
    def likelihood_scale(self):
        """exp(likelihood_log_scale) as the float32 the .res coder takes by value.  The parameter is read back when it has changed
        since the last call (its version counter), not per call."""
        p = self.likelihood_log_scale
        key = (p._version, p.data_ptr())
        if self._likelihood_scale_cache is None or self._likelihood_scale_cache[0] != key:
            from ..io.residual import scale_from_log
            self._likelihood_scale_cache = (key, scale_from_log(p.detach().cpu().item()))
        return self._likelihood_scale_cache[1]

    def set_likelihood_scales(self, log_scales):
        """One likelihood log-scale per colour channel ([3] values: .res version 2 from here on), or None: back to the scalar
        likelihood_log_scale and version 1.  A model with per-channel scales has the extra state_dict() key likelihood_log_scales."""
        if log_scales is None:
            self.likelihood_log_scales = None
        else:
            t = torch.as_tensor(log_scales, dtype=torch.float32).detach().reshape(-1)
            if t.numel() != 3 or not bool(torch.isfinite(t).all()):
                raise ModelError("set_likelihood_scales takes three finite log-scales, or None")
            self.likelihood_log_scales = t.clone().to(self.likelihood_log_scale.device)
        self._likelihood_scales_cache = None

    def likelihood_scales(self):
        """None, or exp(likelihood_log_scales) as the float32 [3] tensor (on the model's device) that the version-2 .res coder reads:
        exp in float64, rounded once to float32, as likelihood_scale() does.  Read back when the buffer has changed, not per call."""
        p = self.likelihood_log_scales
        if p is None:
            return None
        key = (p._version, p.data_ptr())
        if self._likelihood_scales_cache is None or self._likelihood_scales_cache[0] != key:
            from ..io.residual import scale_from_log
            scales = torch.tensor([scale_from_log(v) for v in p.detach().cpu().tolist()], dtype=torch.float32, device=p.device)
            self._likelihood_scales_cache = (key, scales)
        return self._likelihood_scales_cache[1]

    def residual_scale(self):
        """What the .res calls take as `scale`: the per-channel tensor when it is set (version 2), else the one float (version 1)."""
        scales = self.likelihood_scales()
        return self.likelihood_scale() if scales is None else scales

    @torch.no_grad()
    def _lossless_rec(self, images_u8, seed, update_sampler=False, block_size=None):
        """compress_lossless's two passes: ((rec blob, offsets), (K, idx), the DECODER's reconstruction of those files)."""
        if not (images_u8.is_cuda and images_u8.dtype == torch.uint8 and images_u8.dim() == 4 and images_u8.shape[1] == 3):
            raise ModelError("compress_lossless takes a CUDA uint8 tensor [N, 3, H, W]")
        x = images_u8.to(torch.float32).mul_(1.0 / 256.0).sub_(0.5)                 # exact: the values are k / 256 - 1 / 2
        (blob, offsets, _), pendings = self.compress_rec(x, seed, update_sampler=update_sampler, block_size=block_size, return_pendings=True)
        # loc must be the DECODER's reconstruction to the bit.  compress_rec's own differs from it in the last bits (its generative
        # pass runs beside the inference heads: other convolution shapes; tests/test_decompress_device_gpu.py bounds the gap by 1e-5),
        # so the pass that decompress_rec will run is run here, on the rows the files were built from: same function, same rows,
        # same batch, the same bits.
        K, idx = pendings
        reconstruction = self._decompress_device(K, idx, seed, tuple(images_u8.shape), torch.zeros(K.shape[0], dtype=torch.int32, device=K.device))
        return (blob, offsets), pendings, reconstruction

    @torch.no_grad()
    def fit_likelihood_scale(self, images_u8, seed, per_channel=False, batch=None, block_size=None):
        """Fit the likelihood scale to `images_u8` [n, 3, H, W] (uint8, on the model's device) where the data is: every batch goes
        through compress_lossless's own two passes to the decoder's reconstruction, irec.io.residual.fit_scales searches the exact
        coded cost of the pixels over the log-scale (the current scalar among the candidates), and the result is set: the scalar
        likelihood_log_scale (per-channel scales cleared), or with per_channel=True the three likelihood_log_scales.  One small
        read-back per round of the search.  Returns fit_scales' (log_scales, bits, evaluated)."""
        from ..io.residual import fit_scales
        n = images_u8.shape[0]
        step = n if not batch else int(batch)
        pairs = []
        for lo in range(0, n, step):
            chunk = images_u8[lo:lo + step]
            pairs.append((chunk, self._lossless_rec(chunk, seed, block_size=block_size)[2]))
        start = float(self.likelihood_log_scale.detach().cpu().item())
        log_scales, bits, evaluated = fit_scales(pairs, per_channel=per_channel, start=start)
        if per_channel:
            self.set_likelihood_scales(log_scales)
        else:
            self.set_likelihood_scales(None)
            self.likelihood_log_scale.fill_(float(log_scales))
        return log_scales, bits, evaluated

    @torch.no_grad()
    def compress_lossless(self, images_u8, seed, stream_len=None, update_sampler=False, block_size=None, return_pendings=False):
        """images_u8 [N, 3, H, W] uint8 CUDA -> (rec_blob, rec_offsets, res_blob, res_offsets, reconstruction), CUDA tensors.  The model
        sees x / 256 - 0.5; the .rec files are exactly compress_rec's on that input; image i's .res file is
        res_blob[res_offsets[i]:res_offsets[i + 1]]: its pixels arithmetic-coded on the device under the discretized logistic of
        loc = the reconstruction that decompress_rec makes of those files (returned as `reconstruction`) and
        scale = exp(likelihood_log_scale) (irec.io.encode_residuals_device; stream_len: symbols per stream, default
        irec.io.residual.DEFAULT_STREAM_LEN), or, exactly when likelihood_log_scales is set, one scale per channel and version-2
        files.  decompress_lossless gives the images back exactly.
        return_pendings: also compress_rec's device K / idx views, (the five, (K, idx))."""
        from ..io.residual import encode_residuals_device
        (blob, offsets), pendings, reconstruction = self._lossless_rec(images_u8, seed, update_sampler, block_size)
        try:
            res_blob, res_offsets = encode_residuals_device(images_u8, reconstruction, self.residual_scale(), stream_len=stream_len)
        except ValueError as e:
            raise CodingError(str(e))
        out = (blob, offsets, res_blob, res_offsets, reconstruction)
        return (out, pendings) if return_pendings else out

    def _decompress_lossless_device(self, rec_blob, rec_offsets, res_blob, res_offsets, seed, image_shape, max_K, stream_len):
        """Everything of decompress_lossless that runs on the device, on one stream: _decompress_rec_device, the three launches of the
        .res reader on its reconstruction, the joined status, refused images zeroed.  Returns (pixels uint8, status int32 [N], K) on
        the device.  No host synchronisation when max_K is given."""
        from ..io.residual import _decode_residuals_device_launch
        reconstruction, joined, K = self._decompress_rec_device(rec_blob, rec_offsets, seed, image_shape, max_K)
        pixels, res_status = _decode_residuals_device_launch(res_blob, res_offsets, reconstruction, self.residual_scale(), stream_len,
                                                             on_device=True)
        joined = torch.where(joined != 0, joined, torch.where(res_status != 0, res_status + STATUS_RESIDUAL, res_status))
        # an image that an earlier stage refused was residual-decoded on a reconstruction that means nothing: zero, not garbage
        pixels = pixels * (joined == 0).to(torch.uint8).reshape(-1, 1, 1, 1)
        return pixels, joined, K

    @torch.no_grad()
    def _decompress_lossless_status(self, rec_blob, rec_offsets, res_blob, res_offsets, seed, image_shape, max_K=None, stream_len=None):
        """decompress_lossless up to its read-back: (pixels, status int32 numpy [N], K on the device)."""
        from ..io.residual import MAX_STREAM_LEN, _stream_len_device
        if stream_len is None:
            off = res_offsets.cpu().numpy() if hasattr(res_offsets, "cpu") else np.asarray(res_offsets)
            stream_len = _stream_len_device(res_blob, off[:2])
            stream_len = stream_len if stream_len and 1 <= stream_len <= MAX_STREAM_LEN else None   # (a damaged word: the default, and a status)
        pixels, joined, K = self._decompress_lossless_device(rec_blob, rec_offsets, res_blob, res_offsets, seed, image_shape, max_K, stream_len)
        return pixels, joined.cpu().numpy(), K

    @torch.no_grad()
    def decompress_lossless(self, rec_blob, rec_offsets, res_blob, res_offsets, seed, image_shape, max_K=None, strict=True, stream_len=None):
        """The inverse of compress_lossless: N .rec files and their N .res files (blobs uint8 CUDA; offsets [N + 1] on the device or the
        host) to the images, uint8 [N, 3, H, W] on the device, exactly.  decompress_rec's device pass, then the .res reader on its
        reconstruction on the same stream, and ONE read-back -- the per-image status: decompress_rec's, then
        STATUS_RESIDUAL + irec_res_status (include/irec.h) for an image whose .rec decoded but whose .res did not; first cause in that
        order.  An image with a nonzero status is zero.  A reconstruction that differs from the encoder's in any pixel's
        rint(loc * 4096) is the checksum status, not wrong pixels.
        strict: CodingError with the first such image's text, "(image i)" appended; strict=False: (images, status int32 numpy [N]).
        max_K None costs decompress_rec's small read-back of the .rec headers, stream_len None one of 12 bytes of the first .res
        header; a caller that knows them passes them."""
        pixels, host, K = self._decompress_lossless_status(rec_blob, rec_offsets, res_blob, res_offsets, seed, image_shape, max_K, stream_len)
        return self._finish_status(pixels, host, K, strict)


class GraphedDecompress:
    """`model.decompress_rec` for a fixed batch shape as ONE HIP graph on one stream: the three launches of the .rec reader, the
    header check and the whole generative pass (every convolution, hand-off and decode launch of the sequential residual blocks,
    each coder's row check included) are captured once and replayed per batch of files.  Static buffers: the files' bytes
    (blob_bytes), their offsets and the joined status, which is the only read-back.  No parallel branches.  Same outputs as
    decompress_rec.  A file that needs more index slots than the captured max_K (IREC_REC_E_MAX_K), or a blob larger than the static
    buffer, is answered by the eager path with the size it needs, and the next call captures again at that size."""

    def __init__(self, model, image_shape, seed, R, bpt, max_K, blob_bytes):
        self.model, self.image_shape, self.seed = model, tuple(int(v) for v in image_shape), seed
        self.device = next(model.parameters()).device
        if int(R) != model.num_res_blocks or int(bpt) != model.blocks_per_tensor(self.image_shape):
            raise ModelError(f"R = {R}, bpt = {bpt}: the model codes images of shape {self.image_shape} in {model.num_res_blocks} residual "
                             f"blocks of {model.blocks_per_tensor(self.image_shape)} blocks")
        self.R, self.bpt, self.max_K, self.blob_bytes = int(R), int(bpt), max(1, int(max_K)), max(1, int(blob_bytes))
        self.stream = torch.cuda.Stream(device=self.device)
        self.graph = None
        self.captures = 0

    @torch.no_grad()
    def _capture(self):
        n = self.image_shape[0]
        self.static_blob = torch.zeros(self.blob_bytes, dtype=torch.uint8, device=self.device)
        self.static_offsets = torch.zeros(n + 1, dtype=torch.int64, device=self.device)     # N empty files: every image refused, no fault
        cur = torch.cuda.current_stream(self.device)
        self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream):               # warm-up on the graph's stream: caches, ITS scratch, MIOpen
            for _ in range(2):
                self.model._decompress_rec_device(self.static_blob, self.static_offsets, self.seed, self.image_shape, self.max_K)
        cur.wait_stream(self.stream)
        torch.cuda.synchronize(self.device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=self.stream):
            self.reconstruction, self.status, self.K = self.model._decompress_rec_device(self.static_blob, self.static_offsets, self.seed,
                                                                                         self.image_shape, self.max_K)
        self.graph = g
        self.captures += 1

    def _eager(self, blob, offsets, strict):
        """The eager path at the size this batch needs.  Where that is more than the graph holds (a longer row by the headers' own
        words, a larger blob) the next call captures at that size; a damaged file that merely reports IREC_REC_E_MAX_K keeps the graph."""
        need = self.model.files_max_K(blob, offsets)
        if need > self.max_K or blob.numel() > self.blob_bytes:
            self.max_K, self.blob_bytes, self.graph = max(self.max_K, need), max(self.blob_bytes, int(blob.numel())), None
        return self.model.decompress_rec(blob, offsets, self.seed, self.image_shape, max_K=max(self.max_K, need), strict=strict)

    @torch.no_grad()
    def __call__(self, blob, offsets, strict=True):
        """blob: uint8 CUDA tensor; offsets: [N + 1] on the host (numpy / list), checked against the blob before any kernel sees them."""
        n = self.image_shape[0]
        offsets = np.ascontiguousarray(offsets.cpu().numpy() if hasattr(offsets, "cpu") else offsets, dtype=np.int64)
        if offsets.size != n + 1 or offsets[0] < 0 or (np.diff(offsets) < 0).any() or offsets[-1] > blob.numel():
            raise ValueError(f"GraphedDecompress: offsets must be {n + 1} non-decreasing positions that end inside the blob")
        if blob.numel() > self.blob_bytes:
            return self._eager(blob, offsets, strict)
        if self.graph is None:
            self._capture()
        self.static_blob[:blob.numel()].copy_(blob.reshape(-1))
        self.static_offsets.copy_(torch.from_numpy(offsets))
        cur = torch.cuda.current_stream(self.device)
        self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream):
            self.graph.replay()
        cur.wait_stream(self.stream)
        host = self.status.cpu().numpy()
        if (host == _lib.IREC_REC_E_MAX_K).any():
            return self._eager(blob, offsets, strict)
        return self.model._finish_status(self.reconstruction.clone(), host, self.K, strict)


class GraphedCompress:
    """`model.compress` for a fixed image shape and seed as ONE HIP graph: the first call captures the whole device side
    of the pass -- every convolution, elementwise op and coder launch of the 24 strictly sequential residual blocks --
    and later calls replay it (one graph launch instead of several hundred kernel launches; the coder's entry points are
    asynchronous and allocation-free, so they capture like any other kernel).  Inputs are copied into the graph's static
    image buffer; indices are read back with the usual single device-to-host copy.  Same outputs as `model.compress`.
    A block that needs more partitions than the captured index buffers hold falls back to the eager path and re-captures.

    lanes > 1 (round 3; off by default, see below): the batch is cut into `lanes` independent sub-batches, each captured
    as its own graph on its own stream and replayed side by side.  Images are independent (compression_performance.py:305 is
    a plain loop), only the 24 residual blocks of ONE image are sequential (resnet_vae.py:821-826): while one lane waits for
    the single-wave tail of its coder call -- a mid-size call is one or two blocks per CU and lasts as long as its slowest
    block's K sequential steps -- the other lane's convolutions and coder fill the device.  Each lane has its own scratch
    (the engine keys it by stream), its own static buffers and index rows; the indices are the same, image for image."""

    def __init__(self, model, image_shape, seed, update_sampler=False, lanes=None):
        self.model, self.seed, self.update_sampler = model, seed, update_sampler
        self.device = next(model.parameters()).device
        n = int(image_shape[0])
        if lanes is None:
            lanes = 1   # (measured r03d: two lanes do not overlap -- the convolutions' 64 KB and the coder's 160 KB of LDS per workgroup cannot share a CU)
        self.lanes = max(1, min(int(lanes), n))
        cuts = [n * k // self.lanes for k in range(self.lanes + 1)]
        self.slices = [slice(cuts[k], cuts[k + 1]) for k in range(self.lanes)]
        self.static_images = [torch.zeros((sl.stop - sl.start,) + tuple(image_shape[1:]), device=self.device) for sl in self.slices]
        self.streams = [torch.cuda.Stream(device=self.device) for _ in range(self.lanes)]
        self.graphs = None

    @property
    def graph(self):                        # (kept for callers that test "has it been captured")
        return self.graphs

    @graph.setter
    def graph(self, value):
        self.graphs = value

    @torch.no_grad()
    def _capture(self):
        cur = torch.cuda.current_stream(self.device)
        self.graphs, self.pendings, self.reconstructions = [], [], []
        for lane, st in enumerate(self.streams):
            st.wait_stream(cur)
            with torch.cuda.stream(st):                                # warm-up on the lane's stream: caches, ITS scratch, MIOpen
                for _ in range(2):
                    self.model._compress_device(self.static_images[lane], self.seed, self.update_sampler)
            cur.wait_stream(st)
        torch.cuda.synchronize(self.device)
        for lane, st in enumerate(self.streams):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=st):
                pend, rec = self.model._compress_device(self.static_images[lane], self.seed, self.update_sampler)
            self.graphs.append(g); self.pendings.append(pend); self.reconstructions.append(rec)

    @torch.no_grad()
    def __call__(self, image):
        for lane, sl in enumerate(self.slices):
            self.static_images[lane].copy_(image[sl])
        if self.graphs is None:
            if any(getattr(b.coder, "_split_pause", 0) for b in self.model.residual_blocks):
                # a coder is stepping back from a give-up of its cooperative encoder: eager until its pause is over -- a graph
                # captured now would keep the pause's IREC_FLAG_NO_SPLIT for good
                return self.model.compress(image, seed=self.seed, update_sampler=self.update_sampler)
            self._capture()
        cur = torch.cuda.current_stream(self.device)
        for lane, st in enumerate(self.streams):                       # the lanes' graphs side by side, each on its own stream
            st.wait_stream(cur)
            with torch.cuda.stream(st):
                self.graphs[lane].replay()
        for st in self.streams:
            cur.wait_stream(st)
        try:
            flat = PendingCode.gather([p for lane in self.pendings for p in lane])   # ONE device-to-host copy for all lanes
        except (MorePartitionsNeeded, SplitNotResident):
            self.graphs = None                                         # hints were raised / the coders step back from sharing: eager now, re-capture later
            return self.model.compress(image, seed=self.seed, update_sampler=self.update_sampler)
        n_res = len(self.pendings[0])
        per_block = [[img for lane in range(self.lanes) for img in flat[lane * n_res + r]] for r in range(n_res)]
        rec = self.reconstructions[0].clone() if self.lanes == 1 else torch.cat(self.reconstructions, dim=0)
        return self.model._indices_structure(per_block, image.shape[0]), rec
