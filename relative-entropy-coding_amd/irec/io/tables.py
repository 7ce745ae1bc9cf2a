"""Empirical symbol tables for the `.rec` container on the batched and the device paths (include/irec.h: irec_rec_tables_build,
irec_rec_*_tables, irec_rec_hist_rows*), and the histograms they are fitted from.

The reference's container has a second symbol model next to the near-uniform default: write_compressed_code(..., index_counts_file=,
num_aux_var_counts_file=) loads count tables (rec/io/utils.py:31-56), sets header words 6 and 7 and, with count tables, writes
0xFFFFFFFF for the largest partition counts.  A table is the counts of the terminator (entry 0) and of the values 0, 1, ... after it;
the index streams share one table, the partition-count streams have one per residual block.  The reference only loads such tables;
hist_rows and tables_from_histograms make them from packed rows.
"""
from dataclasses import dataclass

import numpy as np

from .. import _lib

TABLE_TOTAL_MAX = 1 << 30            # the 32-bit coder's range holds a model total of at most a quarter of it


def _build_cum(counts, what):
    """irec_rec_tables_build: the cumulative uint32 [n + 1] of counts [n]; ValueError with the library's text."""
    lib = _lib.load()
    counts = np.ascontiguousarray(np.asarray(counts).reshape(-1))
    if counts.size and not np.issubdtype(counts.dtype, np.integer):
        raise ValueError(f"{what}: counts must be integers, got {counts.dtype}")
    counts = counts.astype(np.int64)
    cum = np.zeros(counts.size + 1, dtype=np.uint32)
    if lib.irec_rec_tables_build(counts.ctypes.data if counts.size else None, counts.size, cum.ctypes.data) != 0:
        raise ValueError(f"{what}: {lib.irec_last_error().decode()}")
    return counts, cum


class SymbolTables:
    """The count tables of a call: index_counts, a 1-D integer array (terminator, then one count per index value), and
    num_aux_var_counts, one such array per residual block (their lengths may differ); either may be None, which is the default model
    for that kind of stream.  Every count >= 1 and every table's total <= 2^30 (irec_rec_tables_build refuses anything else)."""

    def __init__(self, index_counts=None, num_aux_var_counts=None):
        self.index_counts = self.index_cum = None
        self.num_aux_var_counts = self.count_cum = self.count_first = None
        self._device = {}
        if index_counts is not None:
            self.index_counts, self.index_cum = _build_cum(index_counts, "SymbolTables: index_counts")
        if num_aux_var_counts is not None:
            built = [_build_cum(c, f"SymbolTables: num_aux_var_counts[{r}]") for r, c in enumerate(num_aux_var_counts)]
            if not built:
                raise ValueError("SymbolTables: num_aux_var_counts holds no table")
            self.num_aux_var_counts = [b[0] for b in built]
            self.count_cum = np.ascontiguousarray(np.concatenate([b[1] for b in built]))
            self.count_first = np.concatenate([[0], np.cumsum([b[1].size for b in built])]).astype(np.int32)

    @property
    def n_index_symbols(self):
        return 0 if self.index_cum is None else self.index_cum.size - 1

    @property
    def n_res_blocks(self):
        """Residual blocks the count tables are for (None without count tables)."""
        return None if self.count_first is None else self.count_first.size - 1

    @property
    def max_K(self):
        """The largest partition count the count tables hold a symbol for (None without count tables)."""
        return None if self.num_aux_var_counts is None else max(c.size - 2 for c in self.num_aux_var_counts)

    def save(self, index_counts_file=None, num_aux_var_counts_file=None):
        """The reference's two .npy forms (what its np.load calls read): a 1-D int array; an object array of per-residual-block arrays."""
        if index_counts_file is not None:
            if self.index_counts is None:
                raise ValueError("SymbolTables.save: there is no index table to save")
            np.save(index_counts_file, self.index_counts)
        if num_aux_var_counts_file is not None:
            if self.num_aux_var_counts is None:
                raise ValueError("SymbolTables.save: there are no count tables to save")
            arr = np.empty(len(self.num_aux_var_counts), dtype=object)
            for r, c in enumerate(self.num_aux_var_counts):
                arr[r] = c
            np.save(num_aux_var_counts_file, arr, allow_pickle=True)

    @classmethod
    def load(cls, index_counts_file=None, num_aux_var_counts_file=None):
        index = None if index_counts_file is None else np.load(index_counts_file)
        counts = None if num_aux_var_counts_file is None else list(np.load(num_aux_var_counts_file, allow_pickle=True))
        return cls(index, counts)

    def host_args(self, n_res_blocks, what):
        """(index_cum, n_index_symbols, count_cum, count_first, n_count_cum) of the host entry points, as addresses."""
        if self.count_first is not None and self.n_res_blocks != int(n_res_blocks):
            raise ValueError(f"{what}: count tables for {self.n_res_blocks} residual blocks, the call has {int(n_res_blocks)}")
        return (None if self.index_cum is None else self.index_cum.ctypes.data, self.n_index_symbols,
                None if self.count_cum is None else self.count_cum.ctypes.data,
                None if self.count_first is None else self.count_first.ctypes.data, 0 if self.count_cum is None else self.count_cum.size)

    def to(self, device):
        """The tables on a device, copied once per device: a DeviceTables whose tensors the device entry points read."""
        import torch
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._device:
            as_i32 = lambda a: None if a is None else torch.from_numpy(a.view(np.int32).copy()).to(device)   # (the uint32 words, bit for bit)
            self._device[device] = DeviceTables(self, as_i32(self.index_cum), as_i32(self.count_cum), as_i32(self.count_first))
        return self._device[device]


@dataclass
class DeviceTables:
    host: SymbolTables
    index_cum: object
    count_cum: object
    count_first: object

    def device_args(self, n_res_blocks, what):
        h = self.host
        if h.count_first is not None and h.n_res_blocks != int(n_res_blocks):
            raise ValueError(f"{what}: count tables for {h.n_res_blocks} residual blocks, the call has {int(n_res_blocks)}")
        return (None if self.index_cum is None else self.index_cum.data_ptr(), h.n_index_symbols,
                None if self.count_cum is None else self.count_cum.data_ptr(),
                None if self.count_first is None else self.count_first.data_ptr(), 0 if self.count_cum is None else self.count_cum.numel())


@dataclass
class RowHistograms:
    """What hist_rows accumulates: index [n_index_values], counts [R, n_count_values], streams [1 + R] (index streams, then count
    streams per residual block), rejected [1] -- 64-bit integers, numpy arrays (uint64) or tensors of one device (int64)."""
    index: object
    counts: object
    streams: object
    rejected: object

    def numpy(self):
        if isinstance(self.index, np.ndarray):
            return self
        return RowHistograms(*(t.cpu().numpy().view(np.uint64) for t in (self.index, self.counts, self.streams, self.rejected)))


def hist_rows(K, idx, blocks_per_res, n_index_values, n_count_values, into=None):
    """Histograms of packed rows K [N, T], idx [N, T, max_K] (T = sum(blocks_per_res)), added INTO `into` (a RowHistograms of an earlier
    call with the same sizes; None: fresh zeros): irec_rec_hist_rows_device for CUDA tensors -- asynchronous on the current stream,
    nothing read back --, irec_rec_hist_rows for host arrays.  A K outside [0, min(max_K, n_count_values - 1)] or an index outside
    [0, n_index_values) is not counted and adds one to `rejected`."""
    lib = _lib.load()
    bpr = np.ascontiguousarray(np.asarray(blocks_per_res, dtype=np.int64).reshape(-1)).astype(np.int32)
    R, T = bpr.size, int(bpr.sum())
    niv, ncv = int(n_index_values), int(n_count_values)
    if hasattr(K, "is_cuda") and K.is_cuda:
        import torch
        from .utils import _row_strides
        if not (idx.is_cuda and K.dtype == torch.int32 and idx.dtype == torch.int32 and K.dim() == 2 and idx.dim() == 3
                and K.shape[1] == T and tuple(idx.shape[:2]) == tuple(K.shape)):
            raise ValueError(f"hist_rows: K {tuple(K.shape)} and idx {tuple(idx.shape)} are not int32 [N, {T}] and [N, {T}, max_K] on one device")
        dev = K.device
        if into is None:
            z = lambda *s: torch.zeros(*s, dtype=torch.int64, device=dev)
            into = RowHistograms(z(max(niv, 0)), z(R, max(ncv, 0)), z(1 + R), z(1))
        elif not (hasattr(into.index, "is_cuda") and into.index.device == dev):
            raise ValueError("hist_rows: `into` lives elsewhere than the rows")
        if tuple(into.index.shape) != (niv,) or tuple(into.counts.shape) != (R, ncv):
            raise ValueError("hist_rows: `into` was made for other sizes")
        n, max_K = K.shape[0], idx.shape[2]
        Kc, ks, ic, ist = _row_strides(K, idx)
        args = (into.index.data_ptr(), into.counts.data_ptr(), into.streams.data_ptr(), into.rejected.data_ptr())
        with torch.cuda.device(dev):
            st = lib.irec_rec_hist_rows_device(n, R, bpr.ctypes.data, max_K, Kc.data_ptr(), ks, ic.data_ptr() if ic.numel() else None, ist,
                                               niv, ncv, *args, torch.cuda.current_stream().cuda_stream)
    else:
        K = np.ascontiguousarray(K, dtype=np.int32)
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        if K.ndim != 2 or K.shape[1] != T or idx.ndim != 3 or idx.shape[:2] != K.shape:
            raise ValueError(f"hist_rows: K {K.shape} and idx {idx.shape} are not [N, {T}] and [N, {T}, max_K]")
        if into is None:
            z = lambda *s: np.zeros(s, dtype=np.uint64)
            into = RowHistograms(z(max(niv, 0)), z(R, max(ncv, 0)), z(1 + R), z(1))
        elif not isinstance(into.index, np.ndarray):
            raise ValueError("hist_rows: `into` lives elsewhere than the rows")
        if tuple(into.index.shape) != (niv,) or tuple(into.counts.shape) != (R, ncv):
            raise ValueError("hist_rows: `into` was made for other sizes")
        n, max_K = K.shape[0], idx.shape[2]
        args = (into.index.ctypes.data, into.counts.ctypes.data, into.streams.ctypes.data, into.rejected.ctypes.data)
        st = lib.irec_rec_hist_rows(n, R, bpr.ctypes.data, max_K, K.ctypes.data, 1, idx.ctypes.data if idx.size else None, max_K, niv, ncv, *args)
    if st == _lib.IREC_E_INVALID:
        raise ValueError(lib.irec_last_error().decode())
    _lib.check(st, "irec_rec_hist_rows")
    return into


def _table_from_histogram(hist, streams):
    """Counts [1 + len(hist)] in Python integers: the terminator once per stream seen, every value once more than it was seen, halved
    (never below 1) until the total fits the coder."""
    c = [max(1, int(streams))] + [1 + int(h) for h in hist]
    while sum(c) > TABLE_TOTAL_MAX:
        c = [max(1, v >> 1) for v in c]
    return np.array(c, dtype=np.int64)


def tables_from_histograms(hist, index=True, counts=True):
    """SymbolTables fitted to a RowHistograms (one read-back if it lives on a device), pure integer arithmetic:
    c[0] = max(1, streams), c[m] = 1 + hist[m - 1], and while the total exceeds 2^30, c = max(1, c >> 1).
    index / counts: which of the two kinds to make a table for."""
    h = hist.numpy()
    index_counts = _table_from_histogram(h.index, h.streams[0]) if index else None
    count_tables = [_table_from_histogram(h.counts[r], h.streams[1 + r]) for r in range(h.counts.shape[0])] if counts else None
    return SymbolTables(index_counts, count_tables)
