"""rec/coding/utils.py: CodingError (:6) and stateless_gumbel_sample (:9-12)."""
import ctypes

import numpy as np

from ..errors import CodingError  # noqa: F401


def stateless_gumbel_sample(shape, seed):
    """-log(-log(tf.random.stateless_normal(shape, [seed, seed + 1]))) -- rec/coding/utils.py:9-12, as written (a NORMAL
    draw inside the double log: NaN wherever it falls outside (0, 1]).  Host numpy float32 of the given shape, evaluated by
    the library's one definition of g (libm's logf twice: irec_tf_stateless_gumbel) -- the bits that the importance sampler's
    Gumbel-max branch (irec_importance_encode, alpha < inf) adds to the weights and that irec_gumbel_table_build hands to the
    kernels.  (numpy's vectorised float32 log is a different function: up to 2 ulp away from logf on this stream.)"""
    from .. import _lib
    n = int(np.prod(shape))
    g = np.empty(n, dtype=np.float32)
    _lib.check(_lib.load().irec_tf_stateless_gumbel(_lib.seed64(seed), n, g.ctypes.data_as(ctypes.c_void_p)), "irec_tf_stateless_gumbel")
    return g.reshape(shape)
