"""An arena with canaries: the memory contract of include/irec.h held against the entry points (tests/test_guarded_arena_host.py on
the host twins, tests/test_memory_contract_gpu.py on the device).  A helper, no tests in it.

An Arena is ONE uint8 tensor (cuda or cpu) filled with GUARD_BYTE; regions are contiguous views carved out of it, each with at least
GUARD_BYTES canary bytes before and after it, so that a stray store of a kernel lands in a canary of the same allocation instead of a
neighbouring tensor of PyTorch's caching allocator (which nothing would notice) or unmapped memory.  Every byte of the arena that is
not inside a region is a canary.

  role "in"       snapshotted by arm(); check() compares the bytes (so NaNs compare equal and 0.0 differs from -0.0)
  role "out"      pre-filled with a recognisable value per dtype (PREFILL): what a call leaves "untouched" is still that value
  role "scratch"  filled with the pattern the caller names (a uint32 pattern; workspaces)

NATURAL is the hostile but legal placement: include/irec.h asks 256-byte alignment of workspaces and nothing of data arrays, so a
float32 / int32 array starts 4 bytes past a 256-byte boundary (4 mod 16: no 8- or 16-byte vector access is aligned), an int64 array
8 bytes past one, and a workspace on the boundary with exactly the bytes its sizing function returned and a canary directly behind."""
import numpy as np
import torch

GUARD_BYTES = 4096
GUARD_BYTE = 0xC3
PREFILL_I32 = 0x5A5A5A5A
PREFILL_F32_BITS = 0x7FC5A5A5          # a quiet NaN with a payload
PREFILL_U8 = 0xAB
PREFILL_I64 = 0x5A5A5A5A5A5A5A5A
PREFILL = {torch.int32: PREFILL_I32, torch.float32: PREFILL_F32_BITS, torch.uint8: PREFILL_U8, torch.int64: PREFILL_I64}
NATURAL = {torch.float32: 4, torch.int32: 4, torch.int64: 8, torch.uint8: 0, "workspace": 0}
_BITS = {torch.int32: torch.int32, torch.float32: torch.int32, torch.uint8: torch.uint8, torch.int64: torch.int64}


def _signed(value, bits):
    value &= (1 << bits) - 1
    return value - (1 << bits) if value >> (bits - 1) else value


def slack(n_regions):
    """Bytes an arena needs on top of its regions' own: guards, alignment, and the arena's own start."""
    return (n_regions + 1) * (GUARD_BYTES + 512) + 512


def as_bytes(t):
    """The tensor's memory as a flat uint8 tensor (a view)."""
    return t.reshape(-1).view(torch.uint8)


class Region:
    def __init__(self, name, role, offset, nbytes, view):
        self.name, self.role, self.offset, self.nbytes, self.view = name, role, offset, nbytes, view
        self.snapshot = None


class Arena:
    def __init__(self, nbytes, device="cpu"):
        self.buf = torch.full((int(nbytes),), GUARD_BYTE, dtype=torch.uint8, device=device)
        self.base = self.buf.data_ptr()
        self.cursor = 0
        self.regions = []

    # ---- carving ---------------------------------------------------------------------------------------------------------
    def region(self, dtype, shape, role, align=None, name=None, fill=None):
        """A contiguous view of `shape` elements of `dtype` whose data_ptr() is `align` modulo 256 (None: NATURAL[dtype])."""
        assert role in ("in", "out", "scratch"), role
        shape = (int(shape),) if np.isscalar(shape) else tuple(int(s) for s in shape)
        item = torch.empty((), dtype=dtype).element_size()
        nbytes = item * int(np.prod(shape, dtype=np.int64))
        align = NATURAL[dtype] if align is None else int(align)
        assert 0 <= align < 256 and align % item == 0, (align, dtype)
        off = self.cursor + GUARD_BYTES
        off += (align - (self.base + off)) % 256           # from the arena's ACTUAL address, not from 0
        assert off + nbytes + GUARD_BYTES <= self.buf.numel(), f"arena of {self.buf.numel()} bytes is full at region {name!r}"
        view = self.buf[off:off + nbytes].view(dtype).view(shape)
        assert view.data_ptr() % 256 == align and view.is_contiguous()
        name = name or f"region{len(self.regions)}"
        if role == "out":
            self._fill(view, PREFILL[dtype] if fill is None else fill)
        elif role == "scratch":
            assert fill is not None, "a scratch region names its pattern"
            self._fill(view, fill)
        self.regions.append(Region(name, role, off, nbytes, view))
        self.cursor = off + nbytes
        return view

    def workspace(self, nbytes, fill, name="workspace"):
        """Exactly `nbytes` bytes on a 256-byte boundary filled with the uint32 pattern `fill`; the canary starts at byte nbytes."""
        return self.region(torch.uint8, (int(nbytes),), "scratch", align=NATURAL["workspace"], name=name, fill=fill)

    def put(self, array, role="in", name=None, align=None):
        """A region of `role` ("in", or "scratch" for an in/out argument) holding a copy of the numpy array (int32 / int64 / float32 /
        uint8; uint32 goes in as its int32 bits)."""
        assert role in ("in", "scratch"), role
        a = np.ascontiguousarray(array)
        if a.dtype == np.uint32:
            a = a.view(np.int32)
        t = torch.from_numpy(a.copy())
        r = self.region(t.dtype, tuple(a.shape) if a.ndim else (1,), role, align=align, name=name, fill=0)
        as_bytes(r).copy_(as_bytes(t).to(r.device))
        return r

    @staticmethod
    def _fill(view, pattern):
        """int64: the 64-bit pattern; uint8 with a pattern of one byte: that byte; everything else: the uint32 pattern, little endian."""
        flat, pattern = as_bytes(view), int(pattern)
        if view.dtype == torch.int64:
            view.fill_(_signed(pattern, 64))
        elif view.dtype == torch.uint8 and pattern <= 0xFF:
            flat.fill_(pattern)
        else:
            whole = flat.numel() // 4 * 4
            flat[:whole].view(torch.int32).fill_(_signed(pattern, 32))
            for i in range(whole, flat.numel()):
                flat[i] = (pattern >> (8 * (i - whole))) & 0xFF

    # ---- checking --------------------------------------------------------------------------------------------------------
    def arm(self):
        """Snapshot every `in` region (after the caller has filled them, before the call under test)."""
        for r in self.regions:
            if r.role == "in":
                r.snapshot = as_bytes(r.view).clone()

    def _gaps(self):
        at, out = 0, []
        for i, r in enumerate(self.regions):
            out.append((at, r.offset, f"guard before {r.name!r}" + (f" / after {self.regions[i - 1].name!r}" if i else ""), r, i))
            at = r.offset + r.nbytes
        out.append((at, self.buf.numel(), f"guard after {self.regions[-1].name!r}" if self.regions else "arena", None, len(self.regions)))
        return out

    def _guard_damage(self):
        """None, or the text naming the first canary byte that changed."""
        gaps = self._gaps()
        bad = torch.nonzero(torch.cat([self.buf[a:b] for a, b, *_ in gaps]) != GUARD_BYTE)
        if not bad.numel():
            return None
        first = int(bad[0])
        for a, b, what, nxt, i in gaps:
            if first < b - a:
                at = a + first
                prev = self.regions[i - 1] if i else None
                if prev is not None and (nxt is None or at - (prev.offset + prev.nbytes) < nxt.offset - at):
                    where = f"{at - (prev.offset + prev.nbytes) + 1} byte(s) past the end of {prev.name!r} (byte offset {at - prev.offset} of the region)"
                else:
                    where = f"{nxt.offset - at} byte(s) before {nxt.name!r} (byte offset {at - nxt.offset} of the region)"
                return f"{what}: canary byte changed to 0x{int(self.buf[at]):02X} {where}; {int(bad.numel())} canary byte(s) changed in all"
            first -= b - a
        raise AssertionError("unreachable")

    def _input_damage(self):
        """None, or the text naming the first byte of an `in` region that differs from its snapshot."""
        for r in self.regions:
            if r.role != "in":
                continue
            assert r.snapshot is not None, f"arena.arm() was not called before check() ({r.name!r})"
            bad = torch.nonzero(as_bytes(r.view) != r.snapshot)
            if bad.numel():
                return f"input {r.name!r} was modified: first at byte offset {int(bad[0])}, {int(bad.numel())} byte(s) in all"
        return None

    def check(self):
        """Raises AssertionError naming the region and the first offending byte offset if a canary byte changed or an `in`
        region differs, as bytes, from its snapshot."""
        for damage in (self._guard_damage(), self._input_damage()):
            if damage:
                raise AssertionError(damage)


def _tail_damage(got, live, prefill, row):
    """None, or the text naming the first slot past a coded row's `live` entries that no longer holds the pre-fill."""
    bad = np.flatnonzero(got[live:] != prefill)
    if bad.size:
        return (f"row {row}: slot {live + int(bad[0])} past the row's {live} entries was written "
                f"(0x{int(got[live + int(bad[0])]) & 0xFFFFFFFF:08X}, pre-fill 0x{int(prefill) & 0xFFFFFFFF:08X})")
    return None


def expect_rows(out_idx, K, rows_expected, prefill=PREFILL_I32, live=lambda k: k):
    """The whole index array [n_rows, max_K] against its expected image.  A coded row (0 <= K <= max_K) holds rows_expected[row] in
    its first live(K) slots and the pre-fill in the rest ("rest untouched", include/irec.h); a row the call reports as not coded
    (K < 0 or K > max_K) is exempt inside itself -- the header promises nothing there."""
    got = out_idx.detach().cpu().numpy() if isinstance(out_idx, torch.Tensor) else np.asarray(out_idx)
    K = K.detach().cpu().numpy() if isinstance(K, torch.Tensor) else np.asarray(K)
    assert got.ndim == 2 and K.shape == (got.shape[0],) and len(rows_expected) == got.shape[0]
    max_K = got.shape[1]
    fill = np.int32(_signed(prefill, 32))
    for row in range(got.shape[0]):
        k = int(K[row])
        if k < 0 or k > max_K:
            continue
        n = live(k)
        want = np.asarray(rows_expected[row], dtype=np.int32)
        assert want.shape == (n,), f"row {row}: the reference holds {want.size} entries for K = {k}"
        assert np.array_equal(got[row, :n], want), f"row {row}: indices {got[row, :n].tolist()} != reference {want.tolist()}"
        damage = _tail_damage(got[row], n, fill, row)
        if damage:
            raise AssertionError(damage)
