"""The ideal half of a results row: what the reference's evaluation drivers take from a sampling forward pass `model(image)`
(examples/lossless/compression_performance.py:321-342, examples/lossy/compress_with_lossy_model.py:193-215) -- seeded draws from a
batch's posteriors with the closed-form KL, and the discretized-logistic log-likelihood of a batch.

CUDA tensors go through irec_posterior_draw_device / irec_loglik_device (csrc/irec_ideal.hip: two launches each, nothing else) on
the current stream, CPU tensors through the host twins, the same core over host memory, which give the device's bits.  Nothing
synchronises: both functions can be captured by torch.cuda.graph on one stream, and their float64 results stay on the device until
the caller reads them.

The noise is this library's own seeded stream (include/irec.h has the definition), not TensorFlow's: the reference's pass is
unseeded.  A draw is a property of (seed, tag, image number, element) only, so image i of a batch with base b has the bits of a
one-image call with base b + i."""
import torch

from . import _lib

TILE = 4096


def _f32(t, what):
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"irec.ideal: {what} must be a tensor")
    return t.to(torch.float32).contiguous()


def _workspace(lib, n, dims, device):
    nbytes = lib.irec_ideal_workspace_bytes(n, dims)
    return torch.empty(max(nbytes, 8) // 8, dtype=torch.float64, device=device)


def _check(lib, st):
    if st != 0:
        raise ValueError(lib.irec_last_error().decode("utf-8", "replace"))


def posterior_draw(posterior, prior, seed, tag, image_base=0, n_threads=0):
    """(sample, kl): sample = posterior.loc + posterior.scale * eps(seed, tag, image_base + i, e) in float32, in the shape of
    posterior.loc ([N, ...]: the first axis is the image); kl float64 [N], the sum over an image's elements of
    KL(posterior || prior) in nats.  posterior / prior: anything with .loc and .scale, four tensors of one shape on one device.
    seed: any int64; tag: a uint32 naming the tensor (a residual block's index, a level); image_base + i in [0, 2^32)."""
    lib = _lib.load()
    mq, sq, mp, sp = (_f32(t, "loc / scale") for t in (posterior.loc, posterior.scale, prior.loc, prior.scale))
    if not (mq.shape == sq.shape == mp.shape == sp.shape) or mq.dim() < 1 or mq.numel() == 0:
        raise ValueError(f"irec.ideal.posterior_draw: the four statistics are not one non-empty [N, ...] shape ({tuple(mq.shape)}, "
                         f"{tuple(sq.shape)}, {tuple(mp.shape)}, {tuple(sp.shape)})")
    if not (mq.device == sq.device == mp.device == sp.device):
        raise ValueError("irec.ideal.posterior_draw: the four statistics are not on one device")
    n = int(mq.shape[0])
    dims = mq.numel() // n
    tag = int(tag)
    if not 0 <= tag < 2 ** 32:
        raise ValueError(f"irec.ideal.posterior_draw: tag {tag} is not a uint32")
    sample = torch.empty_like(mq)
    kl = torch.empty((n,), dtype=torch.float64, device=mq.device)
    args = (mq.data_ptr(), sq.data_ptr(), mp.data_ptr(), sp.data_ptr(), n, dims, _lib.seed64(seed), tag, int(image_base), sample.data_ptr(),
            kl.data_ptr())
    if mq.is_cuda:
        workspace = _workspace(lib, n, dims, mq.device)
        with torch.cuda.device(mq.device):
            st = lib.irec_posterior_draw_device(*args, workspace.data_ptr(), workspace.numel() * 8,
                                                torch.cuda.current_stream(mq.device).cuda_stream)
    else:
        st = lib.irec_posterior_draw_host(*args, int(n_threads))
    _check(lib, st)
    return sample, kl


def log_likelihood(images, reconstruction, log_scale, binsize=1. / 256., n_threads=0):
    """float64 [N]: the reference's discretized_logistic (rec/models/resnet_vae.py:640-650) per image, in nats, of images
    [N, C, H, W] under loc = reconstruction (the clipped one) and scale = exp(log_scale).  log_scale: a number or a one-element
    tensor (one scale), or C values (one per channel).  The exponential is taken by the library, on the tensors' device."""
    lib = _lib.load()
    if not isinstance(images, torch.Tensor) or not isinstance(reconstruction, torch.Tensor) or images.shape != reconstruction.shape \
            or images.dim() != 4 or images.numel() == 0:
        raise ValueError("irec.ideal.log_likelihood: images and reconstruction are not one non-empty [N, C, H, W] shape")
    if images.device != reconstruction.device:
        raise ValueError(f"irec.ideal.log_likelihood: images on {images.device}, reconstruction on {reconstruction.device}")
    x, loc = _f32(images, "images"), _f32(reconstruction, "reconstruction")
    n, c, h, w = (int(v) for v in x.shape)
    if isinstance(log_scale, torch.Tensor):
        scales = log_scale.detach().to(device=x.device, dtype=torch.float32).reshape(-1).contiguous()
    else:
        scales = torch.full((1,), float(log_scale), dtype=torch.float32, device=x.device)
    if scales.numel() not in (1, c):
        raise ValueError(f"irec.ideal.log_likelihood: {scales.numel()} log-scales for {c} channels (one, or one per channel)")
    ll = torch.empty((n,), dtype=torch.float64, device=x.device)
    args = (x.data_ptr(), loc.data_ptr(), scales.data_ptr(), int(scales.numel()), n, c, h * w, float(binsize), ll.data_ptr())
    if x.is_cuda:
        workspace = _workspace(lib, n, c * h * w, x.device)
        with torch.cuda.device(x.device):
            st = lib.irec_loglik_device(*args, workspace.data_ptr(), workspace.numel() * 8, torch.cuda.current_stream(x.device).cuda_stream)
    else:
        st = lib.irec_loglik_host(*args, int(n_threads))
    _check(lib, st)
    return ll
