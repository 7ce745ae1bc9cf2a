"""Host mirror of rec/coding/beam_search_coder.py: same constructor, methods, argument order and error behaviour;
the arithmetic runs in the gfx950 kernels behind include/irec.h (no CPU path).

Distributions are duck-typed exactly as in the reference (only `.loc` and `.scale` are read, coder.py:427-430),
e.g. torch.distributions.Normal with CPU or cuda (HIP) float32 tensors.
"""
import ctypes

import numpy as np
import torch

from .coder import GaussianCoder
from .pending import MorePartitionsNeeded, PendingCode, SplitNotResident  # noqa: F401 (the import path of every caller)
from .utils import CodingError
from .. import _lib
from ..engine import Engine


class BeamSearchCoder(GaussianCoder):
    def __init__(self, kl_per_partition, n_beams, extra_samples=1., extrapolate_auxiliary_ratios=True,
                 name="gaussian_encoder", **kwargs):
        """beam_search_coder.py:15-30.  Extension: `engine=` (an `irec.Engine` built with the caller's own quantile table,
        irec_create_ex) instead of the device's default engine."""
        engine = kwargs.pop("engine", None)
        super().__init__(name=name, kl_per_partition=kl_per_partition, sampler=None,
                         extrapolate_auxiliary_ratios=extrapolate_auxiliary_ratios, **kwargs)
        self.engine = engine
        self.n_beams = n_beams
        self.n_samples = int(np.exp(kl_per_partition * extra_samples))
        self.big_prime = 10007
        self.force_generic = False   # debugging / testing knob: IREC_FLAG_FORCE_GENERIC
        self.fused_philox = False    # debugging / testing knob: IREC_FLAG_FUSED_PHILOX
        self.one_table = False       # debugging / testing knob: IREC_FLAG_ONE_TABLE
        self.team = False            # debugging / testing knob: IREC_FLAG_TEAM (the team encoder also for small calls)
        self.no_split = False        # the caller's knob: IREC_FLAG_NO_SPLIT on every call (no block is ever shared between workgroups / teams)
        self._split_pause = 0        # calls still to be issued without sharing after a give-up (_split_strikes), see _split_gave_up
        self._test_split_orphan = False  # test hook (IREC_FLAG_TEST_SPLIT_ORPHAN): the split encoder's partners leave at once
        self.team_shape = "default"  # diagnostics: IREC_FLAG_SHAPE_* workgroup shape of the team encoder
        self.reuse_tables = True     # IREC_FLAG_REUSE_TABLES: a call whose proposal tables are already in the stream's scratch
                                     # (same seed, S, dims and window: the 24 residual blocks of an image) does not rebuild them
        self.table_steps = 0         # partitions the per-call proposal tables cover; 0 = sized from the partition counts
                                     # this coder has seen so far (_K_seen + 4, at least 8; the library bounds the bytes);
                                     # blocks with more are coded by the fused-Philox kernel in a second pass of the same call

    # ---- small host-side mirrors ---------------------------------------------------------------------------------
    def simple_hash(self, matrix):
        """beam_search_coder.py:33-35 (int32 arithmetic, floormod)."""
        m = np.asarray(matrix, dtype=np.int64).reshape(len(matrix), -1)
        w = np.arange(69, 69 + m.shape[1], dtype=np.int64)
        s = ((m * w).sum(axis=1) + 2 ** 31) % 2 ** 32 - 2 ** 31  # int32 wrap-around
        return (np.mod(s, self.big_prime - 1) + 1).astype(np.int32)

    def get_codelength(self, indicies):
        """beam_search_coder.py:150-151."""
        return len(indicies) * np.log(self.n_samples)

    # ---- plumbing --------------------------------------------------------------------------------------------------
    def table_window(self):
        """Partitions the per-call proposal tables cover: `table_steps`, or the running hint from the partition counts read
        back so far (the tables cost set-up time and scratch per step they cover; typical K is ~8)."""
        if self.table_steps:
            return int(self.table_steps)
        return min(_lib.IREC_TABLE_STEPS_MAX, max(8, (self._K_seen + 4 + 3) // 4 * 4))

    # ---- recovery from a give-up (round 5; until then one give-up set no_split for the life of the coder) -----------
    SPLIT_PAUSE_MAX = 64
    SPLIT_STRIKES_FINAL = 8    # consecutive give-ups after which the coder never shares a block again (no_split = True)

    def _split_gave_up(self):
        """A cooperative call of this coder read back K = -2 (partners not resident within 100 ms).  Bounded back-off: the
        n-th consecutive give-up keeps the next 2^(n-1) calls -- the first of which codes the failed blocks again -- free of
        shared blocks (1, 2, 4, ... at most SPLIT_PAUSE_MAX calls); then the cooperative form is tried again, and the first
        shared call that comes back whole resets the count.  One transient co-tenant therefore costs ONE call its 100 ms and
        a recode, not every later small call a factor of two."""
        self._split_strikes = min(self._split_strikes + 1, 1 + self.SPLIT_PAUSE_MAX.bit_length())
        self._split_pause = min(1 << (self._split_strikes - 1), self.SPLIT_PAUSE_MAX)
        if self._split_strikes >= self.SPLIT_STRIKES_FINAL:
            # a PERMANENT co-tenant (another stream's gangs hold the CUs for good): every retry costs its 100 ms, a recode and -- under
            # HIP-graph replay -- a re-capture; after this many give-ups in a row (127 calls of back-off in between) the coder stops sharing
            self.no_split = True

    def _take_sharing_turn(self):
        """May the call about to be issued share blocks?  Consumes one call of a running pause."""
        if self.no_split:
            return False
        if self._split_pause > 0:
            self._split_pause -= 1
            return False
        return True

    def _params(self, table_steps=None, shared=None):
        if shared is None:
            shared = not self.no_split and self._split_pause == 0
        if not self.extrapolate_auxiliary_ratios:
            self.get_auxiliary_ratio(0)          # (raises the reference's "has not been initialized yet", coder.py:222-225)
        if not (1 <= self.n_beams <= _lib.MAX_BEAMS):
            raise CodingError(f"n_beams must be in [1, {_lib.MAX_BEAMS}], got {self.n_beams}")
        if self.n_samples < 1:
            raise CodingError(f"n_samples = {self.n_samples} < 1")
        flags = (_lib.IREC_FLAG_FORCE_GENERIC if self.force_generic else 0) | \
                (_lib.IREC_FLAG_FUSED_PHILOX if self.fused_philox else 0) | \
                (_lib.IREC_FLAG_ONE_TABLE if self.one_table else 0) | \
                (_lib.IREC_FLAG_TEAM if self.team else 0) | (0 if shared else _lib.IREC_FLAG_NO_SPLIT) | \
                (_lib.IREC_FLAG_REUSE_TABLES if self.reuse_tables else 0) | \
                _lib.IREC_FLAG_SHAPE[self.team_shape] | \
                (_lib.IREC_FLAG_TEST_SPLIT_ORPHAN if self._test_split_orphan and shared else 0)
        steps = int(table_steps) if table_steps else self.table_window()
        return Engine.params(self.kl_per_partition, self.n_samples, self.n_beams, flags, table_steps=steps)

    def encode_tensors_device(self, q_loc, q_scale, p_loc, p_scale, seed, block_size, max_K=None, table_steps=None):
        """Asynchronous core of encode: launches the encoder on the current stream and returns a `PendingCode` -- K,
        indices and sample still on the device, NO host synchronisation.  The caller reads the indices when it needs
        them (`PendingCode.to_lists`, one device-to-host copy; `PendingCode.gather` for many calls at once)."""
        src = torch.as_tensor(q_loc)
        if src.ndim < 2 or src.shape[0] < 1 or src[0].numel() < 1:
            raise CodingError(f"nothing to encode: distributions of shape {tuple(src.shape)} (need [batch >= 1, dims >= 1 ...])")
        eng = self._engine_for(src)
        shared = self._take_sharing_turn()
        params = self._params(table_steps, shared)   # (a model passes ONE window to all its coders: equal keys, tables built once)
        n_tensors = src.shape[0]
        n = src[0].numel()
        shapes = {tuple(torch.as_tensor(t).shape) for t in (q_loc, q_scale, p_loc, p_scale)}
        if len(shapes) != 1:
            raise CodingError("All tensor arguments supplied to split must have the same batch dimensions!")
        ql, qs, pl, ps = (self._dev(t, eng.device) for t in (q_loc, q_scale, p_loc, p_scale))
        lay = eng.layout(n_tensors, n, block_size, seed)
        max_K = self._max_K_hint if max_K is None else int(max_K)
        K, idx, sample = eng.encode_blocks(params, lay, ql, qs, pl, ps, seed, max_K)
        return PendingCode(self, lay, K, idx, sample.reshape(src.shape).to(src.device), max_K, shared, params)

    def encode_tensors(self, q_loc, q_scale, p_loc, p_scale, seed, block_size):
        """Batched core of encode / encode_block: leading dim = independent latent tensors.
        Returns (indices per tensor per block, sample tensor on the input's device)."""
        max_K = None
        while True:
            pending = self.encode_tensors_device(q_loc, q_scale, p_loc, p_scale, seed, block_size, max_K)
            try:
                return pending.to_lists(), pending.sample
            except MorePartitionsNeeded as e:     # a block's KL asks for more partitions than the index buffer holds
                max_K = e.need
            except SplitNotResident:              # partners not resident (the device is shared): the next call -- this loop's --
                if not pending.shared:            # codes the blocks again without sharing, which cannot wait in vain
                    raise
                self._split_gave_up()

    def decode_tensors(self, p_loc, p_scale, indices, seed, block_size):
        src = torch.as_tensor(p_loc)
        if src.ndim < 2 or src.shape[0] < 1 or src[0].numel() < 1:
            raise CodingError(f"nothing to decode: coding distribution of shape {tuple(src.shape)} (need [batch >= 1, dims >= 1 ...])")
        eng = self._engine_for(src)
        params = self._params()
        pl, ps = (self._dev(t, eng.device) for t in (p_loc, p_scale))
        lay = eng.layout(src.shape[0], src[0].numel(), block_size, seed)
        K, idx = self._rows_of_lists(lay, indices, self.MIN_INDICES, self.n_samples, eng.device)
        sample = eng.decode_blocks(params, lay, pl, ps, seed, K, idx)
        return sample.reshape(src.shape).to(src.device)

    MIN_INDICES = 0     # a zero-KL block of the beam-search coder emits no index

    def decode_tensors_device(self, p_loc, p_scale, K, idx, seed, block_size, rows=None, status=None):
        """decode_tensors for rows that are on the device already (GaussianCoder.decode_tensors_device has the arguments): the row
        check into `status`, then the decode, with no host copy, no synchronisation and no Python loop over blocks.  Tensors that fit
        the LDS take irec_beam_decode_tensors with `rows` as its block_row, so packed arrays are read where they lie (a strided view
        is copied once: that entry point takes contiguous rows); otherwise the rows are gathered into layout order and decoded
        block-wise (irec_beam_decode_ws)."""
        src = torch.as_tensor(p_loc)
        if src.ndim < 2 or src.shape[0] < 1 or src[0].numel() < 1:
            raise CodingError(f"nothing to decode: coding distribution of shape {tuple(src.shape)} (need [batch >= 1, dims >= 1 ...])")
        params = self._params()
        eng, lay, pl, ps, Kf, ks, If, ist = self._device_rows(p_loc, p_scale, K, idx, seed, block_size, rows, status, self.n_samples)
        bs_eff = lay.n if lay.block_size is None else int(lay.block_size)
        if eng.lib.irec_decode_tensors_supported(ctypes.byref(params), lay.n, bs_eff):
            if ks != 1 or ist != If.shape[1]:
                Kf, If = Kf.contiguous(), If.contiguous()
            block_row = rows if rows is not None else lay.identity_rows_dev()
            sample = eng.decode_blocks(params, lay, pl, ps, seed, Kf, If, mode="tensors", block_row=block_row)
        else:
            K_lay, idx_lay = self._rows_in_layout_order(lay, Kf, If, rows)
            sample = eng.decode_blocks(params, lay, pl, ps, seed, K_lay, idx_lay, mode="tables")
        return sample.reshape(src.shape).to(src.device)

    # ---- reference API -----------------------------------------------------------------------------------------------
    def encode_block(self, target_dist, coding_dist, seed, update_sampler=False, numpy=True):
        """beam_search_coder.py:53-122.  Returns (list of K indices, sample with the shape of loc)."""
        if target_dist.loc.shape[0] != 1:
            raise CodingError("For encoding, batch size must be 1.")
        idx, sample = self.encode_tensors(target_dist.loc, target_dist.scale, coding_dist.loc, coding_dist.scale,
                                          seed, None)
        indices = idx[0][0]
        if numpy:
            indices = [np.int32(v) for v in indices]
        return list(indices), sample

    def decode_block(self, coding_dist, indices, seed):
        """beam_search_coder.py:124-148.  (The reference reverses the caller's list in place, :127; this does not.)"""
        indices = [int(v) for v in indices]
        loc = torch.as_tensor(coding_dist.loc)
        batched = loc if loc.shape[0] == 1 else loc.reshape((1,) + tuple(loc.shape))
        scale = torch.as_tensor(coding_dist.scale).reshape(batched.shape)
        out = self.decode_tensors(batched, scale, [[indices]], seed, None)
        return out.reshape(loc.shape)

    def encode(self, target_dist, coding_dist, seed, **kwargs):
        """GaussianCoder.encode, coder.py:412-457.  Extensions (the reference rejects N != 1, beam_search_coder.py:54-55):
        `batched=True`: a leading batch dim N > 1 encodes N independent latent tensors in one launch;
        `defer=True`: returns (PendingCode, sample) without any host synchronisation -- the model shims use it to keep
        the 24 sequential residual blocks of an image on the device and read all indices once at the end."""
        batched = kwargs.pop("batched", False)
        defer = kwargs.pop("defer", False)
        if self.block_size is None and not batched and not defer:
            return self.encode_block(target_dist, coding_dist, seed, **kwargs)
        if target_dist.loc.shape[0] != 1 and not batched:
            raise CodingError("For encoding, batch size must be 1.")
        if defer:
            pending = self.encode_tensors_device(target_dist.loc, target_dist.scale, coding_dist.loc, coding_dist.scale,
                                                 seed, self.block_size, kwargs.pop("max_K", None),
                                                 kwargs.pop("table_steps", None))
            return pending, pending.sample
        idx, sample = self.encode_tensors(target_dist.loc, target_dist.scale, coding_dist.loc, coding_dist.scale,
                                          seed, self.block_size)
        if self.block_size is None:
            idx = [blocks[0] for blocks in idx]
        return (idx if batched else idx[0]), sample

    def _decode_lists(self, coding_dist, indices, seed, batched):
        """GaussianCoder.decode (coder.py:459-491) of host lists: always the kernels."""
        if self.block_size is None and not batched:
            return self.decode_block(coding_dist, indices, seed)
        per_tensor = indices if batched else [indices]
        if self.block_size is None:
            per_tensor = [[ix] for ix in per_tensor]
        return self.decode_tensors(coding_dist.loc, coding_dist.scale, per_tensor, seed, self.block_size)
