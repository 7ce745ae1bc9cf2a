"""What a deferred encode call leaves behind, and how a pass of such calls is read back: `PendingCode` (K, index rows and sample
still on the device), the two errors a read-back can ask a recode with, and `recode`, the one loop that answers them.  Both coders
(coder.py, beam_search_coder.py) issue PendingCodes; the models, the harness and the sharded encoder gather them.
"""
import gc

import numpy as np
import torch

from .utils import CodingError
from .. import _lib


class MorePartitionsNeeded(CodingError):
    """A block has K = ceil(KL / Omega) > max_K: it was NOT coded; encode again with max_K >= need."""

    def __init__(self, need):
        super().__init__(f"a block needs {need} partitions: encode again with max_K >= {need}")
        self.need = need


class SplitNotResident(CodingError):
    """A cooperative encoder (the split encoder: several workgroups per block of a small call; shared rows: several teams per
    row of a mid-size call) gave up waiting for partners that were not resident -- other work held the CUs.  The blocks were NOT
    coded.  The coder that issued the call has been told (`BeamSearchCoder._split_gave_up`): its next call -- the one that
    codes these blocks again -- goes out without sharing; see there for when sharing comes back."""


class _RaggedShares:
    """K [N, T] seen as the packed checks index it, K[:, r, :]: the columns [first[r], first[r + 1]) of call r."""

    def __init__(self, K, first):
        self.K, self.first = K, first

    def __getitem__(self, key):
        r = key[1]
        return self.K[:, self.first[r]:self.first[r + 1]]


class PendingCode:
    """Result of one asynchronous encode call: everything stays on the device until the host asks.
    K [n_blocks] int32, idx [n_blocks, max_K] int32 (rows in layout order), sample (input shape)."""

    min_indices = 0   # indices a coded row holds at least: 1 for the sequential coder, whose zero-KL block emits one (coder.py:548-557)

    def __init__(self, coder, lay, K, idx, sample, max_K, shared=False, params=None):
        self.coder, self.lay, self.K, self.idx, self.sample, self.max_K = coder, lay, K, idx, sample, max_K
        self.shared, self.params = shared, params   # the call was allowed to share blocks between workgroups / teams; its irec_params

    def _check(self, K_host):
        """Errors and hints from the partition counts read back (shared by the list and the packed read-backs)."""
        if (K_host == -2).any():
            raise SplitNotResident("the cooperating workgroups of a shared block were not all resident (other work on this device, "
                                   "or two cooperating calls in flight on different streams): the call is coded again without sharing")
        if self.shared and self.coder._split_strikes and self.params is not None and K_host.size:
            # a call that did share blocks came back whole: the device is ours again, the back-off starts over
            eng = self.coder._engine_for(self.K)
            if eng.plan(self.params, self.lay, self.max_K)["split"] >= 2:
                self.coder._split_strikes = 0
        if (K_host < 0).any():
            raise CodingError("a block exceeded the engine's dimension bound")
        need = int(K_host.max()) if K_host.size else 0
        limit = getattr(self.coder._engine_for(self.K), "max_partitions", _lib.MAX_PARTITIONS) if not self.coder.extrapolate_auxiliary_ratios else _lib.MAX_PARTITIONS
        if need > limit:                 # fitted ratios: GaussianCoder.get_auxiliary_ratio raises for the first index past the table
            self.coder.get_auxiliary_ratio(need - 1)
        if need > _lib.MAX_PARTITIONS:   # (before any hint is touched: one degenerate block -- an infinite KL reads back as
            # 10^9 partitions -- must not leave the coder, or the model that shares its hints, asking for more than the library takes)
            raise CodingError(f"KL divergence needs {need} partitions; this build supports {_lib.MAX_PARTITIONS}")
        self.coder._max_K_hint = min(max(self.coder._max_K_hint, need), _lib.MAX_PARTITIONS)
        c = self.coder            # table window hint: what covers the bulk of the blocks read back (a few outliers take the
        if K_host.size:           # second pass instead of stretching every later call's tables), decaying by an eighth per read
            flat = K_host.reshape(-1)
            upper_quartile = int(np.partition(flat, (3 * (flat.size - 1)) // 4)[(3 * (flat.size - 1)) // 4])   # (np.quantile
            bulk = (5 * upper_quartile + 3) // 4                       #  costs 40 us a call: 1 ms per 24-block image)
            c._K_seen = bulk if c._K_reads == 0 else max(bulk, c._K_seen - max(1, c._K_seen // 8))
        c._K_reads += 1
        if need > self.max_K:
            raise MorePartitionsNeeded(need)

    def _lists(self, K_host, idx_host):
        self._check(K_host)
        lay = self.lay
        bpt = lay.blocks_per_tensor
        # One C-speed conversion, the per-block lists are slices of it; the cyclic collector is paused meanwhile (a batched
        # model pass makes tens of thousands of small lists, none of them garbage: generation-2 passes triggered by the
        # allocation count alone cost more than the conversion).
        gc_was_on = gc.isenabled()
        gc.disable()
        try:
            rows, ks = idx_host.tolist(), (np.maximum(K_host, self.min_indices) if self.min_indices else K_host).tolist()
            nat = lay.natural.tolist() if hasattr(lay.natural, "tolist") else list(lay.natural)
            return [[rows[r][:ks[r]] for r in nat[i * bpt:(i + 1) * bpt]] for i in range(lay.n_tensors)]
        finally:
            if gc_was_on:
                gc.enable()

    def to_lists(self):
        """Indices per tensor per block (host lists): ONE device-to-host copy (K and the index rows together)."""
        both = torch.cat([self.K[:, None], self.idx], dim=1).cpu().numpy()
        return self._lists(both[:, 0], both[:, 1:])

    # ---- a pass: the calls of one model pass (the residual blocks of an image batch), read back together ----------------------
    @staticmethod
    def _joined(pendings):
        """The rows of a list of calls, call after call in layout order, as ONE device tensor [rows][1 + width]: K in column 0, the
        index rows zero-padded to the widest call's."""
        width = max(p.idx.shape[1] for p in pendings)
        rows = []
        for p in pendings:
            r = torch.cat([p.K[:, None], p.idx], dim=1)
            if r.shape[1] < width + 1:
                r = torch.nn.functional.pad(r, (0, width + 1 - r.shape[1]))
            rows.append(r)
        return torch.cat(rows, dim=0)

    @staticmethod
    def _check_calls(pendings, check):
        """check(r, call) for EVERY call of a pass, so that every coder's hint is raised before the caller codes again; then one
        error for the pass.  A call that gave up makes every distinct coder of the pass step back, once; a MorePartitionsNeeded
        wins over a SplitNotResident, and among several the largest need."""
        retry, gave_up = None, False
        for r, p in enumerate(pendings):
            try:
                check(r, p)
            except MorePartitionsNeeded as e:
                if not isinstance(retry, MorePartitionsNeeded) or e.need > retry.need:
                    retry = e
            except SplitNotResident as e:
                gave_up = True
                if retry is None:
                    retry = e
        if gave_up:
            for coder in {id(p.coder): p.coder for p in pendings}.values():
                coder._split_gave_up()
        if retry is not None:
            raise retry

    @staticmethod
    def gather(pendings):
        """Indices of many calls (e.g. the 24 residual blocks of a model pass) with ONE device-to-host copy in all."""
        if not pendings:
            return []
        both = PendingCode._joined(pendings).cpu().numpy()
        first = np.concatenate([[0], np.cumsum([p.K.shape[0] for p in pendings])]).tolist()
        out = []
        PendingCode._check_calls(pendings, lambda r, p: out.append(
            p._lists(both[first[r]:first[r + 1], 0], both[first[r]:first[r + 1], 1:1 + p.idx.shape[1]])))
        return out

    @staticmethod
    def _joined_packed(pendings):
        """The rows of R calls on the SAME layout as ONE device tensor [N, R, bpt, 1 + width], image-major, K in column 0."""
        lay = pendings[0].lay
        same = all((p.lay.n_tensors, p.lay.n, p.lay.block_size, p.lay.n_blocks) == (lay.n_tensors, lay.n, lay.block_size, lay.n_blocks)
                   and (p.lay.block_size is None or p.lay.seed == lay.seed) for p in pendings)
        if not same or lay.natural is None:
            raise CodingError("gather_packed needs calls on one block layout (same tensor count, size, block_size and seed)")
        both = PendingCode._joined(pendings)
        n, bpt, R = lay.n_tensors, lay.blocks_per_tensor, len(pendings)
        sel = lay.packed_index(R)                                             # row of (image i, residual block r, block j)
        return both.index_select(0, sel).reshape(n, R, bpt, both.shape[1])

    @staticmethod
    def _joined_ragged(pendings):
        """The rows of R calls that share a tensor count and seed but NOT a layout (the two levels of the lossy model: 13 and 302 blocks
        per image) as ONE device tensor [N, T, 1 + width], image-major, K in column 0: call r's blocks of image i in natural block order
        from row i T + first[r].  Returns (tensor, blocks_per_res)."""
        lay = pendings[0].lay
        if any(p.lay.natural is None or p.lay.n_tensors != lay.n_tensors or p.lay.seed != lay.seed for p in pendings):
            raise CodingError("gather_packed_ragged needs whole calls on one tensor count and seed")
        both = PendingCode._joined(pendings)
        n, bpr = lay.n_tensors, [p.lay.blocks_per_tensor for p in pendings]
        cache = lay.__dict__.setdefault("_ragged_index", {})
        key = tuple((p.lay.n, p.lay.block_size) for p in pendings)       # (`natural` is a function of these and the tensor count)
        if key not in cache:
            base = np.concatenate([[0], np.cumsum([p.lay.n_blocks for p in pendings])])
            sel = np.concatenate([base[r] + np.asarray(p.lay.natural, dtype=np.int64).reshape(n, bpr[r]) for r, p in enumerate(pendings)], axis=1)
            cache[key] = torch.from_numpy(np.ascontiguousarray(sel.reshape(-1))).to(pendings[0].K.device)
        return both.index_select(0, cache[key]).reshape(n, sum(bpr), both.shape[1]), bpr

    @staticmethod
    def _gather_packed(pendings, ragged, on_device):
        """The four packed gathers: the joined tensor (uniform [N, R, bpt, 1 + width] / ragged [N, T, 1 + width]), every call's checks on
        its own share of the partition counts read back, the min_indices clamp, and K / idx -- numpy arrays after ONE device-to-host
        copy of the whole tensor, or (on_device) its VIEWS, with K alone copied for the checks."""
        if ragged:
            both, bpr = PendingCode._joined_ragged(pendings)
        else:
            both = PendingCode._joined_packed(pendings)
        if not on_device:
            both = both.cpu().numpy()
        K, idx = both[..., 0], both[..., 1:]
        K_host = K.cpu().numpy() if on_device else K
        shares = _RaggedShares(K_host, np.concatenate([[0], np.cumsum(bpr)])) if ragged else K_host
        PendingCode._check_calls(pendings, lambda r, p: p._check(shares[:, r, :]))
        least = pendings[0].min_indices
        if on_device:
            if least:
                K.clamp_(min=least)
        else:
            K, idx = np.ascontiguousarray(np.maximum(K, least) if least else K), np.ascontiguousarray(idx)
        return (K, idx, bpr) if ragged else (K, idx)

    @staticmethod
    def gather_packed(pendings):
        """Indices of R calls on the SAME layout (the residual blocks of a batched model pass) as packed arrays, image-major:
        K [N, R, bpt] int32, idx [N, R, bpt, max_K] int32 (numpy; rows are valid up to K) -- ONE gather on the device and ONE
        device-to-host copy, no per-index Python object.  irec.io.encode_files takes them as they are."""
        return PendingCode._gather_packed(pendings, ragged=False, on_device=False)

    @staticmethod
    def gather_packed_device(pendings):
        """gather_packed with the indices left on the device: the K [N, R, bpt] and idx [N, R, bpt, max_K] VIEWS of the one joined
        tensor, which irec.io.encode_files_device takes as they are (strided).  Only K is read back, for the same checks
        (SplitNotResident, MorePartitionsNeeded, the hints, min_indices)."""
        return PendingCode._gather_packed(pendings, ragged=False, on_device=True)

    @staticmethod
    def gather_packed_ragged(pendings):
        """gather_packed for calls on DIFFERENT layouts: (K [N, T] int32, idx [N, T, max_K] int32, blocks_per_res), numpy, max_K the widest
        call's, T = sum(blocks_per_res) -- ONE gather on the device and ONE device-to-host copy.  irec.io.encode_files_ragged takes them
        as they are.  The checks of gather_packed run on each call's own share of K."""
        return PendingCode._gather_packed(pendings, ragged=True, on_device=False)

    @staticmethod
    def gather_packed_ragged_device(pendings):
        """gather_packed_ragged with the indices left on the device: the K [N, T] and idx [N, T, max_K] VIEWS of the one joined tensor, which
        irec.io.encode_files_device_ragged takes as they are (strided).  Only K is read back, for the same checks."""
        return PendingCode._gather_packed(pendings, ragged=True, on_device=True)


def recode(code_pass, gather, coders, attempts=6):
    """Code a pass until its read-back is whole: `code_pass()` -> (pendings, rest) launches it, `gather(pendings)` reads it back.
    A block that needs more index slots than the coders' hint (the hints are raised by the read-back), or a shared block whose
    partners were not resident (every coder's next call goes out unshared): the pass is coded again, `attempts` times in all.
    Returns (gather's result, rest).  The only place that answers these two errors with a recode; anything else passes through."""
    for _ in range(attempts):
        pendings, rest = code_pass()
        try:
            return gather(pendings), rest
        except (MorePartitionsNeeded, SplitNotResident):
            continue
    raise MorePartitionsNeeded(max(c._max_K_hint for c in coders) + 1)
