"""What the batched file calls of irec.io share (utils.py: the `.rec` container; residual.py: the `.res` container): a blob of N files
with offsets [N + 1] and one status per file, written into a buffer that may turn out short and read under offsets nobody trusts."""
import numpy as np

from .. import _lib


def raise_first_status(status, text_of):
    """ValueError with text_of(status) and an "(image i)" suffix for the first image whose status is nonzero."""
    bad = np.flatnonzero(status)
    if bad.size:
        i = int(bad[0])
        raise ValueError(f"{text_of(int(status[i]))} (image {i})")


def check_status(st, name):
    """The irec_status of library call `name`: ValueError with the library's text for refused arguments, IrecLibraryError for the rest."""
    if st == _lib.IREC_E_INVALID:
        raise ValueError(_lib.load().irec_last_error().decode())
    _lib.check(st, name)


# ---- offsets of a reader: no file's range may leave the blob ------------------------------------------------------------------------
def host_offsets(offsets, blob_bytes, who, n=None):
    """offsets (numpy, CPU or CUDA tensor) as a contiguous int64 host array, checked against a blob of blob_bytes bytes.
    n: the images the call has (None: as many as the offsets say, at least none)."""
    off = np.ascontiguousarray(offsets.cpu().numpy() if hasattr(offsets, "cpu") else offsets, dtype=np.int64)
    if (off.size < 1 if n is None else off.size != n + 1) or off[0] < 0 or (np.diff(off) < 0).any() or off[-1] > blob_bytes:
        raise ValueError(f"{who}: offsets must be {'' if n is None else '[N + 1], '}non-decreasing and end inside the blob")
    return off


def device_offsets(offsets, blob, dev, on_device, who, n=None):
    """The offsets of a device reader as an int64 tensor on `dev`.  Host offsets are checked against the blob (host_offsets) and copied;
    on_device: offsets that ARE on a device stay there -- they are clamped into the blob and made non-decreasing by two small device
    operations instead, so that no file's range leaves the blob whatever they hold (a range that was wrong reads as a damaged file),
    nothing is read back and the call can be captured in a HIP graph."""
    import torch
    if on_device and hasattr(offsets, "is_cuda") and offsets.is_cuda:
        if offsets.dtype != torch.int64 or offsets.dim() != 1 or (offsets.numel() < 1 if n is None else offsets.numel() != n + 1):
            raise ValueError(f"{who}: device offsets must be int64 [N + 1]")
        return torch.cummax(offsets.to(dev).clamp(0, blob.numel()), dim=0).values.contiguous()
    return torch.from_numpy(host_offsets(offsets, blob.numel(), who, n).copy()).to(dev)   # (a copy: the caller's array may be read-only)


def gather_heads(blob, offsets, head_bytes):
    """The first head_bytes bytes of every file of a blob on the device, gathered there and copied to the host in ONE read-back:
    (bytes uint8 numpy [N head_bytes], offsets int64 [N + 1] into them) -- what a host function over (blob, offsets) takes.  A file
    shorter than that, or whose range leaves the blob, reads as zeros; no files or no bytes: an empty blob, nothing read back."""
    import torch
    dev = blob.device
    off = offsets.to(dev) if hasattr(offsets, "is_cuda") else torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.int64)).to(dev)
    n = off.numel() - 1
    if n < 1 or blob.numel() < 1:
        return np.zeros(0, np.uint8), np.zeros(1, np.int64)
    at = (off[:-1, None] + torch.arange(head_bytes, device=dev)).clamp_(0, blob.numel() - 1)
    whole = (off[1:] - off[:-1] >= head_bytes) & (off[:-1] >= 0) & (off[1:] <= blob.numel())
    head = blob.reshape(-1)[at] * whole[:, None].to(torch.uint8)
    return head.cpu().numpy().reshape(-1), np.arange(n + 1, dtype=np.int64) * head_bytes


# ---- a device writer: offsets and status in one buffer, one read-back, a second run at the size the first one reports ----------------
def offsets_and_status(n, dev):
    """(offsets int64 [N + 1], status int32 [N], both): views of one int64 device buffer `both`, which one copy fetches."""
    import torch
    both = torch.empty(n + 1 + (n + 1) // 2, dtype=torch.int64, device=dev)
    return both[:n + 1], both[n + 1:].view(torch.int32)[:n], both


def encode_device(launch, n, out, text_of, name):
    """launch(out) -> (offsets, status, both) as offsets_and_status gives them, the files in `out` only if they fit it.  One read-back
    per run; a short `out` costs a second run at exactly the size the first one reports.  (blob, offsets) on the device."""
    import torch
    for _attempt in range(2):
        offsets, _, both = launch(out)
        host = both.cpu().numpy()
        raise_first_status(host[n + 1:].view(np.int32)[:n], text_of)
        total = int(host[n])
        if total <= out.numel():
            return out[:total], offsets
        out = torch.empty(total, dtype=torch.uint8, device=out.device)
    raise ValueError(f"{name}: the files did not fit the size the call itself reported")


# ---- a host writer that reports the size it needs ----------------------------------------------------------------------------------------
def encode_host(call, cap):
    """call(out uint8 [cap]) -> the bytes the files take (it raises for its own errors); once more at that size if cap was short."""
    while True:
        out = np.empty(cap, dtype=np.uint8)
        total = call(out)
        if total <= cap:
            return out[:total]
        cap = int(total)
