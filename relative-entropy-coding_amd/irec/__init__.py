"""irec -- MI355X-native iREC coders (host package).

Mirrors the `rec.coding` operator surface of gergely-flamich/relative-entropy-coding for the sampler='beam_search' path and
for sampler='importance' (the sequential GaussianCoder over an ImportanceSampler); all arithmetic of the hot paths runs in
hand-written gfx950 kernels behind the C ABI of libirec_hip.so (include/irec.h).  The beam-search coder has no CPU
fallback: without the built library or without a GPU its entry points raise.  The sequential coder runs the reference's
loop on the host for CPU tensors and for samplers the kernels do not cover, as the reference itself does.
"""
from . import _lib  # noqa: F401
from . import ideal  # noqa: F401
from . import image  # noqa: F401
from . import metrics  # noqa: F401
from .coding import BeamSearchCoder, Coder, CodingError, GaussianCoder  # noqa: F401
from .coding.samplers import ImportanceSampler, Sampler  # noqa: F401
from .engine import Engine, get_engine  # noqa: F401

__all__ = ["BeamSearchCoder", "Coder", "GaussianCoder", "ImportanceSampler", "Sampler", "CodingError", "Engine", "get_engine", "metrics", "ideal", "image"]
