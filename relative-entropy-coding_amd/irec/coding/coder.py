"""Host mirror of rec/coding/coder.py (reference file:line in each docstring).

The block split/merge bookkeeping, the auxiliary-variance ratios -- extrapolated (the power law), FITTED ones handed over
as data, or fitted here by update_auxiliary_variance_ratios (coder.py:233-410: the kernels of csrc/irec_fit.hip for GPU tensors,
their host twin for CPU tensors) -- and the sampler-driven GaussianCoder.encode / decode / encode_block / decode_block
(coder.py:412-587): the reference's loop on the host for any Sampler object, the gfx950 kernels of csrc/irec_gc.hip for the
ImportanceSampler (alpha = inf, or the Gumbel-max of a finite alpha >= 1) on GPU tensors -- blocks of any dim, block_size=None included; the size of the normal proposal
tables (IREC_TABLE_BYTES_HARD, IREC_TABLE_STEPS_MAX) is the remaining limit.  The update_sampler branch is out of scope.
"""
import abc

import numpy as np
import torch

from .pending import MorePartitionsNeeded, PendingCode
from .utils import CodingError
from .. import _lib
from ..engine import Engine, FitError, NormalTableTooLarge, fit_aux_ratios_host, get_engine, tf_shuffle_perm

AUX_RATIO_POWER_LAW = -0.7864636765648174  # coder.py:16
# coder.py:226-230: a partition count beyond the fitted ratio table (table length, count asked for)
RATIO_TABLE_TEXT = ("KL divergence higher than auxiliary variables can account for. "
                    "Update auxiliary variable ratios with high-enough KL divergence."
                    "Maximum possible number of partitions is {}."
                    "Requested {}")


def _det_log(x):
    """The deterministic float64 log of csrc/irec_device.h (det_log), operation by operation."""
    x = np.array(x, dtype=np.float64, copy=True).reshape(-1)
    bits = x.view(np.uint64)
    e = ((bits >> np.uint64(52)) & np.uint64(0x7FF)).astype(np.int64)
    sub = e == 0
    if sub.any():
        x = np.where(sub, x * 18014398509481984.0, x)
        bits = x.view(np.uint64)
        e = np.where(sub, ((bits >> np.uint64(52)) & np.uint64(0x7FF)).astype(np.int64) - 54, e)
    e = e - 1023
    m = ((bits & np.uint64(0x000FFFFFFFFFFFFF)) | np.uint64(0x3FF0000000000000)).view(np.float64)
    big = m > 1.4142135623730951
    m = np.where(big, m * 0.5, m)
    e = e + big
    s = (m - 1.0) / (m + 1.0)
    s2 = s * s
    q = np.full_like(s, 1.0 / 25.0)
    for k in (23, 21, 19, 17, 15, 13, 11, 9, 7, 5, 3):
        q = q * s2 + 1.0 / k
    return e.astype(np.float64) * 0.6931471805599453 + (2.0 * s + (2.0 * s) * (s2 * q))


def _det_exp(x):
    """The deterministic float64 exp of csrc/irec_device.h (det_exp), operation by operation."""
    x = np.array(x, dtype=np.float64, copy=True).reshape(-1)
    with np.errstate(all="ignore"):
        xs = np.clip(np.nan_to_num(x, nan=0.0), -708.0, 709.0)
        kf = np.floor(xs * 1.4426950408889634 + 0.5)
        r = (xs - kf * 0.693147180369123816490) - kf * 1.90821492927058770002e-10
        p = np.full_like(r, 1.0 / 6227020800.0)
        for c in (479001600.0, 39916800.0, 3628800.0, 362880.0, 40320.0, 5040.0, 720.0, 120.0, 24.0, 6.0):
            p = p * r + 1.0 / c
        p = p * r + 0.5
        p = p * r + 1.0
        p = p * r + 1.0
        scale = ((kf.astype(np.int64) + 1023).astype(np.uint64) << np.uint64(52)).view(np.float64)
        out = p * scale
    out = np.where(x < -708.0, 0.0, np.where(x > 709.0, np.inf, out))
    return np.where(np.isnan(x), x, out)


def canonical_partitions(mq, sq, mp, sp, omega):
    """K = ceil(KL / Omega) of one block as block_kl_kernel computes it (csrc/irec_kernels.hip): the float64 KL of
    every dim, dims in groups of 256, lane l chains dims 4l .. 4l+3, the 64 lane sums paired at distance 32, 16, .., 1, group sums
    added in order, rounded to float32 once; then ceil in float32.  A KL that is not positive gives 0, an infinite one 10^9."""
    with np.errstate(all="ignore"):
        mq, sq, mp, sp = (np.asarray(v, np.float32).reshape(-1).astype(np.float64) for v in (mq, sq, mp, sp))
        t = sq / sp
        dm = (mq - mp) / sp
        kl = 0.5 * (dm * dm) + (0.5 * (t * t - 1.0) - _det_log(t))
        groups = -(-kl.size // 256)
        if not groups:
            return 0
        v = np.zeros(groups * 256)
        v[:kl.size] = kl
        v = v.reshape(groups, 64, 4)
        lanes = np.zeros((groups, 64))
        for i in range(4):
            lanes = lanes + v[:, :, i]
        at = np.arange(64)
        for off in (32, 16, 8, 4, 2, 1):
            lanes = lanes + lanes[:, at ^ off]
        total = lanes[0, 0]
        for g in range(1, groups):
            total = total + lanes[g, 0]
        total = np.float32(total)
        if not total > 0:
            return 0
        k = np.ceil(total / np.float32(omega))
        return int(k) if k < np.float32(1.0e9) else 1000000000


class DeviceWindowExceeded(NormalTableTooLarge):
    """A block of a device call needs more partitions than its normal tables can cover: the call takes the host loop."""


class _Dist:
    """Duck-typed distribution: samplers and coders read only .loc and .scale (coder.py:427-430)."""

    def __init__(self, loc, scale):
        self.loc, self.scale = loc, scale


class Coder(abc.ABC):
    """coder.py:27-138.  `split`/`merge` are kept for API parity and for host-side checks; the kernels perform the
    same gather / scatter through the permutation on the fly."""

    def __init__(self, block_size=None, name="encoder", **kwargs):
        self.name = name
        self.block_size = block_size

    def split(self, *args, seed=42):
        """coder.py:38-85: flatten, shuffle all tensors with the same seeded permutation, cut into blocks."""
        tensor_shape = args[0].shape
        flattened = []
        for tensor in args:
            if tensor.shape != tensor_shape:
                raise CodingError("All tensor arguments supplied to split must have the same batch dimensions!")
            flattened.append(tensor.reshape(-1))
        num_dims = flattened[0].shape[0]
        perm = torch.from_numpy(tf_shuffle_perm(seed, num_dims)).to(flattened[0].device)
        flattened = [flat[perm] for flat in flattened]
        all_blocks = []
        for tensor in flattened:
            all_blocks.append([tensor[i:min(i + self.block_size, num_dims)]
                               for i in range(0, num_dims, self.block_size)])
        return all_blocks

    def merge(self, *args, shape=None, seed=42):
        """coder.py:87-122: inverse of split."""
        if shape is None:
            raise CodingError("Shape cannot be None!")
        tensors = [torch.cat(list(blocks), dim=0) for blocks in args]
        num_dims = tensors[0].shape[0]
        for tensor in tensors:
            if tensor.dim() != 1:
                raise CodingError("All supplied tensors to merge must be rank 1!")
            if tensor.shape[0] != num_dims:
                raise CodingError("All tensors must have the same number of dimensions!")
        perm = torch.from_numpy(tf_shuffle_perm(seed, num_dims)).to(tensors[0].device)
        inv = torch.empty_like(perm)
        inv[perm] = torch.arange(num_dims, device=perm.device)
        return [tensor[inv].reshape(shape) for tensor in tensors]

    @abc.abstractmethod
    def encode(self, target_dist, coding_dist, seed, **kwargs):
        pass

    @abc.abstractmethod
    def decode(self, coding_dist, indices, seed, **kwargs):
        pass

    @abc.abstractmethod
    def encode_block(self, target_dist, coding_dist, seed, **kwargs):
        pass

    @abc.abstractmethod
    def decode_block(self, coding_dist, indices, seed, **kwargs):
        pass


class GaussianCoder(Coder):
    """coder.py:174-231 (constructor + get_auxiliary_ratio)."""

    def __init__(self, kl_per_partition, sampler=None, extrapolate_auxiliary_ratios=True, block_size=None,
                 name="gaussian_encoder", **kwargs):
        super().__init__(name=name, block_size=block_size, **kwargs)
        self.sampler = sampler
        self.kl_per_partition = np.float32(kl_per_partition)  # tf.cast(kl_per_partition, tf.float32), coder.py:192
        self.extrapolate_auxiliary_ratios = extrapolate_auxiliary_ratios
        if not self.extrapolate_auxiliary_ratios:          # coder.py:203-216: the variables a checkpoint restores
            self.aux_variable_variance_ratios = np.array([1.], dtype=np.float32)
            self.average_counts = np.array([1.], dtype=np.float32)   # batch elements every ratio was averaged over
            self._initialized = False
        self.last_fit_iters = None   # SGD iterations of every step of the last ratio fit (ratio = M .. 2)
        self.table_steps = 0         # steps the normal proposal tables of a device call cover; 0 = the default window
        self.engine = None           # an `irec.Engine` of the caller's own instead of the device's default (BeamSearchCoder's `engine=`)
        # what PendingCode's checks keep for every coder that issues device calls
        self._max_K_hint = _lib.IREC_TABLE_STEPS_DEFAULT   # index slots per block of a device call (raised when a block needs more)
        self._K_seen = 28            # what covers the bulk of the K read back so far (starts at the default window; shrinks with evidence)
        self._K_reads = 0
        self._split_strikes = 0      # consecutive give-ups of the cooperative encoders (SplitNotResident), BeamSearchCoder._split_gave_up
        self.last_path = None        # "device" / "host": which path the sequential coder's last encode / decode call took

    def set_auxiliary_variance_ratios(self, ratios, average_counts=None):
        """The FITTED ratios of an extrapolate_auxiliary_ratios=False coder, as data: what the reference restores into
        `aux_variable_variance_ratios` / `average_counts` / `_initialized` from a checkpoint (coder.py:203-216).
        average_counts (None: ones): over how many batch elements every ratio was averaged -- a later
        update_auxiliary_variance_ratios keeps averaging from there (coder.py:385-389)."""
        if self.extrapolate_auxiliary_ratios:
            raise CodingError("this coder extrapolates its auxiliary ratios (extrapolate_auxiliary_ratios=True)")
        r = np.ascontiguousarray(np.asarray(ratios, dtype=np.float32).reshape(-1))
        if r.size < 1 or not np.all((r > 0) & (r <= 1)):
            raise CodingError("auxiliary variance ratios must be a non-empty sequence of numbers in (0, 1]")
        c = np.ones_like(r) if average_counts is None else np.ascontiguousarray(np.asarray(average_counts, dtype=np.float32).reshape(-1))
        if c.shape != r.shape or not np.all(c >= 0):
            raise CodingError("average_counts must hold one non-negative number per ratio")
        self.aux_variable_variance_ratios = r
        self.average_counts = c
        self._initialized = True
        self._ratio_engine = None

    def get_auxiliary_ratio(self, index):
        """coder.py:218-231."""
        if self.extrapolate_auxiliary_ratios:
            return np.power(index + 1., AUX_RATIO_POWER_LAW)
        if not self._initialized:
            raise CodingError("Coder has not been initialized yet, please call"
                              "update_auxiliary_variance_ratios() first"
                              " or use extrapolation")
        if index >= self.aux_variable_variance_ratios.shape[0]:
            raise CodingError(RATIO_TABLE_TEXT.format(self.aux_variable_variance_ratios.shape[0], index + 1))
        return self.aux_variable_variance_ratios[index]

    def update_auxiliary_variance_ratios(self, target_dist, coding_dist, seed=42, relative_tolerance=1e-4, max_iters=10000,
                                         learning_rate=0.001):
        """coder.py:233-264.  A no-op with extrapolated ratios (the coder is stateless).  Otherwise the rows of the
        fit: with block_size=None the leading dim indexes them and the rest is flattened; with a block size every block BUT THE
        LAST of every tensor of the leading batch after split(seed=seed) (the last is dropped even when it is full, coder.py:253-258).
        `seed` also seeds the fit's auxiliary draws (DESIGN.md §3 "ratio fit": the reference's are unseeded)."""
        if self.extrapolate_auxiliary_ratios:
            return
        stats = [torch.as_tensor(t).detach() for t in (target_dist.loc, target_dist.scale, coding_dist.loc, coding_dist.scale)]
        if len({tuple(t.shape) for t in stats}) != 1:
            raise CodingError("All tensor arguments supplied to split must have the same batch dimensions!")
        if stats[0].ndim < 1 or stats[0].numel() < 1:
            raise CodingError("update_auxiliary_variance_ratios needs at least one row")
        if self.block_size is None:
            rows = [t.reshape(t.shape[0], -1) for t in stats]
        else:
            per = [[] for _ in stats]
            for i in range(stats[0].shape[0]):
                blocks = self.split(*(t[i:i + 1] for t in stats), seed=seed)
                for k, b in enumerate(blocks):
                    per[k].extend(b[:-1])
            if not per[0]:
                raise CodingError("update_auxiliary_variance_ratios: no full block to fit to (every tensor has a single block, "
                                  "and the last block of a tensor is left off, coder.py:253-258)")
            rows = [torch.stack(b, dim=0) for b in per]
        self.update_block_auxiliary_variance_ratios(_Dist(rows[0], rows[1]), _Dist(rows[2], rows[3]), seed=seed,
                                                    relative_tolerance=relative_tolerance, max_iters=max_iters, learning_rate=learning_rate)

    def update_block_auxiliary_variance_ratios(self, target_dist, coding_dist, seed=42, relative_tolerance=1e-4, max_iters=10000,
                                               learning_rate=0.001):
        """coder.py:266-410 over [rows, ...] statistics: the kernels of csrc/irec_fit.hip for GPU tensors, their host twin for CPU
        tensors -- same bits (DESIGN.md §3 "ratio fit").  `last_path` says which one ran."""
        if self.extrapolate_auxiliary_ratios:
            return
        stats = [torch.as_tensor(t).detach() for t in (target_dist.loc, target_dist.scale, coding_dist.loc, coding_dist.scale)]
        if len({tuple(t.shape) for t in stats}) != 1:
            raise CodingError("All tensor arguments supplied to split must have the same batch dimensions!")
        if stats[0].ndim < 1 or stats[0].numel() < 1:
            raise CodingError("update_auxiliary_variance_ratios needs at least one row")
        if int(max_iters) < 1:
            raise CodingError("max_iters must be at least 1")
        n = stats[0].shape[0]
        args = (seed, self.kl_per_partition, self.aux_variable_variance_ratios, self.average_counts, relative_tolerance, max_iters,
                learning_rate)
        try:
            if stats[0].device.type == "cuda":
                eng = get_engine(stats[0].device)
                r, c, iters = eng.fit_aux_ratios(*(self._dev(t.reshape(n, -1), eng.device) for t in stats), *args)
                self.last_path = "device"
            else:
                r, c, iters = fit_aux_ratios_host(*(self._host(t.reshape(n, -1)) for t in stats), *args)
                self.last_path = "host"
        except FitError as e:
            raise CodingError(str(e))
        self.aux_variable_variance_ratios, self.average_counts, self.last_fit_iters = r, c, [int(v) for v in iters]
        self._initialized = True
        self._ratio_engine = None    # the next encode builds a context over the new table

    # ---- the sequential coder (coder.py:412-587): any Sampler on the host, the ImportanceSampler of the reference's models
    #      (any alpha >= 1) in the gfx950 kernels behind irec_gc_importance_encode / _decode ---------------------------------
    def get_codelength(self, indicies):
        """coder.py:586-587."""
        return sum([self.sampler.get_codelength(i) for i in indicies])

    def table_window(self):
        """Steps the normal proposal tables of a call cover (`table_steps`, or the beam coder's default window)."""
        return int(self.table_steps) if self.table_steps else _lib.IREC_TABLE_STEPS_DEFAULT

    def _on_device(self, loc, block_size):
        """The kernels take the call: the reference's own ImportanceSampler (any alpha: the encoders check theirs first,
        `_check_alpha`; a decoder never looks at it, importance_sampling.py:82-103), tensors on the GPU, blocks of any dim (the size of
        the proposal tables is the remaining limit: NormalTableTooLarge sends a call to the host loop).  Everything else runs the
        reference's loop on the host."""
        from .samplers import ImportanceSampler
        if type(self.sampler) is not ImportanceSampler:
            return False
        t = torch.as_tensor(loc)
        return t.device.type == "cuda" and t.ndim >= 2 and t.shape[0] >= 1 and t[0].numel() >= 1

    def _check_alpha(self):
        """alpha < 1 or NaN: the reference's text (importance_sampling.py:33-34), before any device work."""
        from .samplers import ImportanceSampler
        if type(self.sampler) is ImportanceSampler:
            self.sampler._check_alpha()

    # ---- device plumbing, shared with BeamSearchCoder ---------------------------------------------------------------------------
    def _engine_for(self, tensor):
        if self.engine is not None and self.extrapolate_auxiliary_ratios:
            return self.engine
        t = torch.as_tensor(tensor)
        if self.extrapolate_auxiliary_ratios:
            return get_engine(t.device if t.device.type == "cuda" else None)
        # fitted ratios (extrapolate_auxiliary_ratios=False, coder.py:203-231): a context of this coder's own carries them
        # The context is keyed on what it was built from -- the device and the ratio table's bytes: assigning
        # aux_variable_variance_ratios directly (the analogue of the reference restoring its tf.Variables from a checkpoint) or
        # coding a tensor that lives on another GPU builds a new one instead of coding on a stale table.
        self.get_auxiliary_ratio(0)
        dev = t.device if t.device.type == "cuda" else (self.engine.device if self.engine is not None else
                                                        torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None)
        if dev is None:
            raise _lib.IrecLibraryError("irec needs a HIP device (MI355X / gfx950); there is no CPU fallback")
        ratios = np.ascontiguousarray(np.asarray(self.aux_variable_variance_ratios, dtype=np.float32))
        key = (str(torch.device(dev)), ratios.tobytes())
        if getattr(self, "_ratio_engine", None) is None or getattr(self, "_ratio_engine_key", None) != key:
            self._ratio_engine = Engine(dev, lut=getattr(self.engine, "lut", None), aux_ratios=ratios)
            self._ratio_engine_key = key
        return self._ratio_engine

    @staticmethod
    def _dev(t, device):
        return torch.as_tensor(t).detach().to(device=device, dtype=torch.float32).contiguous()

    def _rows_of_lists(self, lay, indices, min_indices, n_samples, device):
        """indices[tensor][block] (host lists) as the rows of a decode call on `device`: K [n_blocks], idx [n_blocks, max_K] int32 in
        layout order.  min_indices: the least a row may hold (the coder's MIN_INDICES)."""
        bpt = lay.blocks_per_tensor
        if len(indices) != lay.n_tensors or any(len(b) != bpt for b in indices):
            raise CodingError("indices do not match the block structure of coding_dist")
        if any(len(ix) < min_indices for b in indices for ix in b):
            raise CodingError("every block of the sequential coder holds at least one index" if min_indices == 1 else
                              f"every block holds at least {min_indices} indices")
        max_K = max(1, max((len(ix) for b in indices for ix in b), default=1))
        if not self.extrapolate_auxiliary_ratios:
            # decode_block asks get_auxiliary_ratio(i) for i = len(indices) - 1 .. 0 (beam_search_coder.py:129-131): an index list longer
            # than the fitted table raises the reference's error here -- the kernels would only mark such a row "not decodable" (p.loc)
            self.get_auxiliary_ratio(max_K - 1)
        K = np.zeros(lay.n_blocks, dtype=np.int32)
        idx = np.zeros((lay.n_blocks, max_K), dtype=np.int32)
        for i in range(lay.n_tensors):
            for j in range(bpt):
                row, ix = lay.natural[i * bpt + j], indices[i][j]
                K[row] = len(ix)
                idx[row, :len(ix)] = np.asarray(ix, dtype=np.int32)
        if idx.size and (idx.min() < 0 or idx.max() >= n_samples):
            raise CodingError("index out of range [0, n_samples)")
        return torch.from_numpy(K).to(device), torch.from_numpy(idx).to(device)

    def _device_rows(self, p_loc, p_scale, K, idx, seed, block_size, rows, status, n_samples):
        """The prelude of decode_tensors_device: the engine, the layout, the coding distribution and the rows as the kernels take them
        (eng, lay, pl, ps, Kf, ks, If, ist), with the row check launched into `status` (kept in `last_rows_status`)."""
        src = torch.as_tensor(p_loc)
        eng = self._engine_for(src)
        pl, ps = (self._dev(t, eng.device) for t in (p_loc, p_scale))
        lay = eng.layout(src.shape[0], src[0].numel(), block_size, seed)
        Kf, ks, If, ist = self._flat_rows(K, idx)
        self.last_rows_status = self._rows_check(eng, lay, Kf, ks, If, ist, rows, status, n_samples)
        return eng, lay, pl, ps, Kf, ks, If, ist

    def encode_tensors_device(self, q_loc, q_scale, p_loc, p_scale, seed, block_size, max_K=None, table_steps=None):
        """Asynchronous core of the device path: one block-KL and one encode launch for all blocks of all tensors (leading dim
        = independent latent tensors); returns a `PendingCode`, nothing is copied to the host."""
        self._check_alpha()
        src = torch.as_tensor(q_loc)
        shapes = {tuple(torch.as_tensor(t).shape) for t in (q_loc, q_scale, p_loc, p_scale)}
        if len(shapes) != 1:
            raise CodingError("All tensor arguments supplied to split must have the same batch dimensions!")
        eng = self._engine_for(src)
        ql, qs, pl, ps = (self._dev(t, eng.device) for t in (q_loc, q_scale, p_loc, p_scale))
        lay = eng.layout(src.shape[0], src[0].numel(), block_size, seed)
        self._max_K_hint = min(self._max_K_hint, self.DEVICE_MAX_K)
        max_K = max(1, min(self._max_K_hint if max_K is None else int(max_K), self.DEVICE_MAX_K))
        self.last_path = "device"
        steps = max(int(table_steps) if table_steps else self.table_window(), max_K)
        K, idx, sample = eng.gc_encode_blocks(lay, ql, qs, pl, ps, seed, self.kl_per_partition, self.sampler.n_samples(), max_K, steps,
                                              alpha=float(self.sampler.alpha))
        pending = PendingCode(self, lay, K, idx, sample.reshape(src.shape).to(src.device), max_K)
        pending.min_indices = 1
        return pending

    DEVICE_MAX_K = _lib.IREC_TABLE_STEPS_MAX   # partitions of a block the tables of a device call can cover
    DEVICE_ATTEMPTS = 4

    def encode_tensors(self, q_loc, q_scale, p_loc, p_scale, seed, block_size):
        """Synchronous device path.  A block with more partitions than the window is coded again with a longer one -- a bounded
        number of times; one that needs more than the tables can cover (DEVICE_MAX_K) sends the call to the host loop
        (DeviceWindowExceeded, a NormalTableTooLarge: the callers fall back as for tables that do not fit)."""
        max_K, need = None, 0
        for _ in range(self.DEVICE_ATTEMPTS):
            pending = self.encode_tensors_device(q_loc, q_scale, p_loc, p_scale, seed, block_size, max_K)
            try:
                return pending.to_lists(), pending.sample
            except MorePartitionsNeeded as e:
                need = e.need
                self._max_K_hint = min(self._max_K_hint, self.DEVICE_MAX_K)   # (never a hint the tables cannot cover)
                if need > self.DEVICE_MAX_K:
                    break
                max_K = need
        raise DeviceWindowExceeded(f"a block needs {need} partitions; the device path covers {self.DEVICE_MAX_K} "
                                   f"and codes a call at most {self.DEVICE_ATTEMPTS} times")

    def decode_tensors(self, p_loc, p_scale, indices, seed, block_size):
        src = torch.as_tensor(p_loc)
        eng = self._engine_for(src)
        pl, ps = (self._dev(t, eng.device) for t in (p_loc, p_scale))
        lay = eng.layout(src.shape[0], src[0].numel(), block_size, seed)
        S = self.sampler.n_samples()
        K, idx = self._rows_of_lists(lay, indices, self.MIN_INDICES, S, eng.device)
        self.last_path = "device"
        sample = eng.gc_decode_blocks(lay, pl, ps, seed, S, K, idx, max(self.table_window(), idx.shape[1]))
        return sample.reshape(src.shape).to(src.device)

    # ---- rows that never leave the device (the output of irec.io.decode_files_device, PendingCode.gather_packed_device) ----------
    MIN_INDICES = 1     # indices a decodable row holds at least (the sequential coder's zero-KL block emits one, coder.py:548-557)

    @staticmethod
    def _flat_rows(K, idx):
        """(K [rows], k_stride, idx [rows, max_K], idx_stride): K of any shape and idx of that shape + (max_K,) as flat rows, WITHOUT a
        copy where the strides allow it -- the packed arrays (1, max_K) and the views of one joined [rows][1 + width] tensor
        (1 + width twice) do; anything else is made contiguous."""
        if not (K.is_cuda and idx.is_cuda and K.dtype == torch.int32 and idx.dtype == torch.int32):
            raise CodingError("decode_tensors_device takes CUDA int32 tensors K and idx")
        if tuple(idx.shape[:-1]) != tuple(K.shape) or idx.dim() != K.dim() + 1:
            raise CodingError(f"K {tuple(K.shape)} and idx {tuple(idx.shape)} are not [...] and [..., max_K]")
        max_K = idx.shape[-1]
        if max_K < 1:
            raise CodingError("idx holds no index slot (max_K = 0): rows on the device need at least one slot each")
        Kf, If = K.reshape(-1), idx.reshape(-1, max_K)      # (views where the strides merge, contiguous copies otherwise)
        ks = Kf.stride(0) if Kf.numel() > 1 else 1
        ist = If.stride(0) if If.shape[0] > 1 else max(max_K, 1)
        if ks < 1:
            Kf, ks = Kf.contiguous(), 1
        if If.stride(1) != 1 or ist < max_K:
            If, ist = If.contiguous(), max_K
        return Kf, int(ks), If, int(ist)

    def _rows_check(self, eng, lay, Kf, ks, If, ist, rows, status, n_samples):
        """Launch the row check of one call (a group = a tensor's blocks) into `status`; returns status."""
        if status is None:
            status = torch.zeros(lay.n_tensors, dtype=torch.int32, device=eng.device)
        k_limit = _lib.INT32_MAX if self.extrapolate_auxiliary_ratios else int(self.aux_variable_variance_ratios.shape[0])
        return eng.rows_status(Kf, ks, If, ist, If.shape[1], lay.n_tensors, lay.blocks_per_tensor, rows, self.MIN_INDICES, k_limit,
                               n_samples, status)

    @staticmethod
    def _rows_in_layout_order(lay, Kf, If, rows):
        """The rows of a call gathered into `lay` order: one index_select each for the counts and the index rows (both take strided
        views), contiguous results.  rows: int32 [n_tensors * bpt] -> row of Kf / If, or None for i * bpt + j."""
        sel = lay.natural_inverse_dev()
        if rows is not None:
            sel = rows.to(torch.int64).index_select(0, sel)
        return Kf.index_select(0, sel), If.index_select(0, sel)

    def decode_tensors_device(self, p_loc, p_scale, K, idx, seed, block_size, rows=None, status=None):
        """decode_tensors for rows that are on the device already: K [...] and idx [..., max_K] CUDA int32 (contiguous, or the views of
        one joined [rows][1 + width] tensor), `rows` (int32 CUDA [n_tensors * bpt], None: i * bpt + j) the row of block j of tensor i.
        Launches the row check (irec_decode_rows_status) into `status` (int32 CUDA [n_tensors]; a nonzero entry is kept, so the calls of
        a pass accumulate the first cause per image) and then the decode -- no host copy, no synchronisation, no Python loop over
        blocks.  A row the check refuses decodes to p_loc, as the kernels promise; the verdict is the caller's to read.  status=None:
        a fresh one, left in `last_rows_status` (device).  Needs the device path (`_on_device`)."""
        self._check_sampler()
        if not self._on_device(p_loc, block_size):
            raise CodingError("decode_tensors_device needs the device path: an ImportanceSampler (any alpha), tensors on the GPU, "
                              "and proposal tables that fit (IREC_TABLE_BYTES_HARD, IREC_TABLE_STEPS_MAX)")
        src, S = torch.as_tensor(p_loc), self.sampler.n_samples()
        eng, lay, pl, ps, Kf, _, If, _ = self._device_rows(p_loc, p_scale, K, idx, seed, block_size, rows, status, S)
        K_lay, idx_lay = self._rows_in_layout_order(lay, Kf, If, rows)
        self.last_path = "device"
        sample = eng.gc_decode_blocks(lay, pl, ps, seed, S, K_lay, idx_lay, max(self.table_window(), If.shape[1]))
        return sample.reshape(src.shape).to(src.device)

    # the reference's loop on the host, any Sampler object.  float32 numpy, one correctly rounded operation per operator of the
    # reference (torch's vectorised CPU sqrt is not correctly rounded, and one ulp in a conditional scale moves the sample)
    @staticmethod
    def _host(t):
        return torch.as_tensor(t).detach().to("cpu", torch.float32).numpy()

    @staticmethod
    def _dist(loc, scale):
        return _Dist(torch.from_numpy(np.ascontiguousarray(loc)), torch.from_numpy(np.ascontiguousarray(scale)))

    def _kl_partitions(self, mq, sq, mp, sp):
        """K = int32(ceil(sum KL(q || p) / Omega)) (coder.py:499-501) -- the canonical K, bit for bit what the device path gets from
        block_kl_kernel, so that one coder emits the same number of indices for CPU and GPU tensors; a degenerate block raises as
        the device path does."""
        K = canonical_partitions(mq, sq, mp, sp, self.kl_per_partition)
        if K > _lib.MAX_PARTITIONS:
            raise CodingError(f"KL divergence needs {K} partitions; this build supports {_lib.MAX_PARTITIONS}")
        return K

    def _encode_block_host(self, target_dist, coding_dist, seed):
        """coder.py:497-559 in the notation of DESIGN.md §3 (cv, tv, a): K - 1 auxiliary variables, then the block's sample, every
        draw through `self.sampler.coded_sample`."""
        seed = _lib.seed64(seed, coding=True)              # (the step seeds seed + t are formed here, not in the library)
        mq, sq, mp, sp = (self._host(t) for t in (target_dist.loc, target_dist.scale, coding_dist.loc, coding_dist.scale))
        device = torch.as_tensor(target_dist.loc).device
        picked, self.last_path = [], "host"
        with np.errstate(all="ignore"):
            for i in range(self._kl_partitions(mq, sq, mp, sp) - 1, 0, -1):
                cv, tv = sp * sp, sq * sq
                a = np.float32(self.get_auxiliary_ratio(i)) * cv
                ta = self._dist((mq - mp) * a / cv, np.sqrt(tv * (a * a) / (cv * cv) + a * (cv - a) / cv))   # coder.py:147-154
                pa = self._dist(np.zeros_like(mp), np.sqrt(a))                                             # coder.py:141-144
                j, drawn = self.sampler.coded_sample(target=ta, coder=pa, seed=seed)
                picked.append(j)
                seed += 1
                A = self._host(drawn)
                mq, sq = mp + (A * tv * cv + (mq - mp) * (cv - a) * cv) / (tv * a + cv * (cv - a)), \
                    np.sqrt(tv * cv * (cv - a) / (a * tv + cv * (cv - a)))                                 # coder.py:163-171
                mp, sp = mp + A, np.sqrt(cv - a)                                                           # coder.py:157-160
        j, z = self.sampler.coded_sample(target=self._dist(mq, sq), coder=self._dist(mp, sp), seed=seed)
        picked.append(j)
        return picked, torch.as_tensor(z).to(device)

    def _decode_block_host(self, coding_dist, indices, seed):
        """coder.py:561-584: the p recursion alone, indices read in encoder order (the caller's list is not touched)."""
        seed = _lib.seed64(seed, coding=True)
        mp, sp = self._host(coding_dist.loc), self._host(coding_dist.scale)
        device = torch.as_tensor(coding_dist.loc).device
        n, self.last_path = len(indices), "host"
        with np.errstate(all="ignore"):
            for t in range(n - 1):
                cv = sp * sp
                a = np.float32(self.get_auxiliary_ratio(n - 1 - t)) * cv
                A = self._host(self.sampler.decode_sample(coder=self._dist(np.zeros_like(mp), np.sqrt(a)), sample_index=indices[t],
                                                          seed=seed + t))
                mp, sp = mp + A, np.sqrt(cv - a)
        return torch.as_tensor(self.sampler.decode_sample(coder=self._dist(mp, sp), sample_index=indices[n - 1], seed=seed + n - 1)).to(device)

    def _check_sampler(self, update_sampler=False):
        if self.sampler is None:
            raise CodingError("GaussianCoder needs a sampler (e.g. irec.ImportanceSampler(coding_bits))")
        if update_sampler:
            raise CodingError("update_sampler=True (the training-time branch that draws target.sample() instead of coding, "
                              "coder.py:516-519,543-546) is not part of this build")

    def encode_block(self, target_dist, coding_dist, seed, update_sampler=False, verbose=False, numpy=True):
        """coder.py:493-559.  Returns (list of max(K, 1) indices, sample with the shape of loc)."""
        if target_dist.loc.shape[0] != 1:
            raise CodingError("For encoding, batch size must be 1.")
        self._check_sampler(update_sampler)
        self._check_alpha()
        if self._on_device(target_dist.loc, None):
            try:
                idx, sample = self.encode_tensors(target_dist.loc, target_dist.scale, coding_dist.loc, coding_dist.scale, seed, None)
                return list(idx[0][0]), sample
            except NormalTableTooLarge:
                pass
        return self._encode_block_host(target_dist, coding_dist, seed)

    def decode_block(self, coding_dist, indices, seed, **kwargs):
        """coder.py:561-584.  The caller's list is left as it is."""
        self._check_sampler()
        indices = [int(v) for v in indices]
        loc = torch.as_tensor(coding_dist.loc)
        if loc.ndim >= 2 and loc.shape[0] == 1 and self._on_device(loc, None):
            try:
                return self.decode_tensors(loc, torch.as_tensor(coding_dist.scale), [[indices]], seed, None)
            except NormalTableTooLarge:
                pass
        return self._decode_block_host(coding_dist, indices, seed)

    def encode(self, target_dist, coding_dist, seed, **kwargs):
        """coder.py:412-457.  Extensions, as BeamSearchCoder.encode has them (device path only): `batched=True` codes a leading
        batch of independent latent tensors in one launch, `defer=True` returns (PendingCode, sample) without a host sync."""
        batched, defer = kwargs.pop("batched", False), kwargs.pop("defer", False)
        max_K, table_steps = kwargs.pop("max_K", None), kwargs.pop("table_steps", None)
        self._check_sampler(kwargs.get("update_sampler", False))
        if target_dist.loc.shape[0] != 1 and not batched:
            raise CodingError("For encoding, batch size must be 1.")
        self._check_alpha()
        if self._on_device(target_dist.loc, self.block_size):
            args = (target_dist.loc, target_dist.scale, coding_dist.loc, coding_dist.scale, seed, self.block_size)
            try:
                if defer:
                    pending = self.encode_tensors_device(*args, max_K, table_steps)
                    return pending, pending.sample
                idx, sample = self.encode_tensors(*args)
                if self.block_size is None:
                    idx = [blocks[0] for blocks in idx]
                return (idx if batched else idx[0]), sample
            except NormalTableTooLarge:
                pass
        if defer:
            raise CodingError("defer=True needs the device path: an ImportanceSampler with alpha >= 1, tensors on the GPU, "
                              "and proposal tables that fit (IREC_TABLE_BYTES_HARD, IREC_TABLE_STEPS_MAX)")
        if batched:
            loc, scale = torch.as_tensor(target_dist.loc), torch.as_tensor(target_dist.scale)
            c_loc, c_scale = torch.as_tensor(coding_dist.loc), torch.as_tensor(coding_dist.scale)
            out = [self.encode(_Dist(loc[i:i + 1], scale[i:i + 1]), _Dist(c_loc[i:i + 1], c_scale[i:i + 1]), seed, **kwargs)
                   for i in range(loc.shape[0])]
            return [o[0] for o in out], torch.cat([o[1] for o in out], dim=0)
        if self.block_size is None:
            return self._encode_block_host(target_dist, coding_dist, seed)
        stats = self.split(target_dist.loc, target_dist.scale, coding_dist.loc, coding_dist.scale, seed=seed)   # coder.py:427-457
        coded = [self._encode_block_host(_Dist(b[0][None, :], b[1][None, :]), _Dist(b[2][None, :], b[3][None, :]), seed) for b in zip(*stats)]
        sample, = self.merge([z[0, :] for _, z in coded], shape=target_dist.loc.shape, seed=seed)
        return [ix for ix, _ in coded], sample

    def decode(self, coding_dist, indices, seed, **kwargs):
        """coder.py:459-491, for both coders.  Extensions: `batched=True`, as `encode`; `packed=(K, idx, rows)` (and `status=`) -- rows
        on the device, decode_tensors_device; `indices` is then ignored."""
        batched = kwargs.pop("batched", False)
        packed, status = kwargs.pop("packed", None), kwargs.pop("status", None)
        if packed is not None:       # (K, idx, rows) on the device: decode_tensors_device, nothing crosses to the host
            return self.decode_tensors_device(coding_dist.loc, coding_dist.scale, packed[0], packed[1], seed, self.block_size,
                                              rows=packed[2], status=status)
        return self._decode_lists(coding_dist, indices, seed, batched)

    def _decode_lists(self, coding_dist, indices, seed, batched):
        """`decode` of host lists: the kernels where `_on_device` says so, the reference's loop on the host otherwise."""
        self._check_sampler()
        loc, scale = torch.as_tensor(coding_dist.loc), torch.as_tensor(coding_dist.scale)
        if self._on_device(loc, self.block_size):
            per_tensor = indices if batched else [indices]
            if self.block_size is None:
                per_tensor = [[ix] for ix in per_tensor]
            try:
                return self.decode_tensors(loc, scale, [[[int(v) for v in ix] for ix in b] for b in per_tensor], seed, self.block_size)
            except NormalTableTooLarge:
                pass
        if batched:
            return torch.cat([self.decode(_Dist(loc[i:i + 1], scale[i:i + 1]), indices[i], seed) for i in range(loc.shape[0])], dim=0)
        if self.block_size is None:
            return self._decode_block_host(coding_dist, indices, seed)
        locs, scales = self.split(loc, scale, seed=seed)                                                        # coder.py:471-491
        parts = [self._decode_block_host(_Dist(m[None, :], sd[None, :]), ix, seed)[0, :] for ix, m, sd in zip(indices, locs, scales)]
        sample, = self.merge(parts, shape=loc.shape, seed=seed)
        return sample
