"""The cases of the per-channel .res tests (version 2) and of the scale fitter, with restatements in plain Python and numpy that
share no code with the library: the version-2 file (tests/residual_cases.py's version-1 restatement extended by one scale word per
channel and a model that changes at the channel boundaries), the reader's header verdict, and the cost table.  A helper, no tests.

Version-2 file, little-endian: 0 magic 'IRES' u32 | 4 version u16 = 2 | 6 channels u16 | 8 stream_len u32 | 12 height u32 |
16 width u32 | 20 + 4 c float32 bits of s_c, c < channels | 20 + 4 channels checksum u32 | 24 + 4 channels n_streams x u16 byte
length | the streams.  Symbol p belongs to channel p // (height * width)."""
import struct

import numpy as np

import residual_cases as RC

VERSION_2 = 2
TILE = 4096                      # csrc/irec_res_fit_core.h: pixels of a channel per workgroup
INT64_MAX = 2 ** 63 - 1

# (C, H, W), stream_len, N: what the issue names
SHAPES = {
    "cross_3x5x7_L16": ((3, 5, 7), 16, 3),          # streams cross both channel boundaries, at symbols 35 and 70
    "one_pixel": ((1, 1, 1), 1, 3),
    "four_channels_L1": ((4, 2, 2), 1, 3),
    "one_stream_3x4x4": ((3, 4, 4), 4096, 3),       # one stream holds all channels
    "wide_3x80x81_L64": ((3, 80, 81), 64, 2),
}
CHANNEL_SCALES = [0.02, 0.05, 0.11, 1.0]
BITS_SHAPE = (2, 3, 67, 71)      # 4757 pixels per channel: two tiles, the second ragged


def header_bytes(c):
    return 24 + 4 * c


def make(n, chw, seed):
    """pixels [n, C, H, W] uint8 near loc (closer in the first channels), loc float32 in the clamp range, scales float32 [C]."""
    rng = np.random.default_rng(seed)
    c, h, w = chw
    loc = rng.uniform(RC.CLAMP_LO, RC.CLAMP_HI, size=(n, c, h, w)).astype(np.float32)
    centre = np.floor((loc + 0.5) * 256.0)
    spread = np.array([3, 8, 20, 120][:c]).reshape(1, c, 1, 1)
    pixels = np.clip(centre + np.rint(rng.standard_normal((n, c, h, w)) * spread), 0, 255).astype(np.uint8)
    return pixels, loc, np.array(CHANNEL_SCALES[:c], dtype=np.float32)


def make_cases():
    return {name: make(n, chw, 1000 + i) + (L,) for i, (name, (chw, L, n)) in enumerate(SHAPES.items())}


# ---- the file -------------------------------------------------------------------------------------------------------------------------
class _ChannelTables:
    """tables(k) for the k-th symbol of a run that starts at position p0: the counts of (m, scale of the symbol's channel)."""
    def __init__(self, scales, plane, ms):
        self.tables = [RC._Tables(float(s)) for s in scales]
        self.plane, self.ms = plane, ms

    def stream(self, p0, p1):
        class _At:
            def __init__(s, outer):
                s.outer, s.p = outer, p0
            def __call__(s, m):
                t = s.outer.tables[s.p // s.outer.plane](m)
                s.p += 1
                return t
        return _At(self)


def ref_file_v2(pixels, loc, scales, stream_len):
    """The version-2 .res file of one image: pixels [C, H, W] uint8, loc the same shape float32, scales [C]."""
    c, h, w = pixels.shape
    xs = [int(v) for v in pixels.reshape(-1)]
    ms = [RC.ref_m(v) for v in loc.reshape(-1)]
    tables = _ChannelTables(scales, h * w, ms)
    streams = [RC.ref_pack(RC.ref_encode_stream(xs[k:k + stream_len], ms[k:k + stream_len], tables.stream(k, k + stream_len)))
               for k in range(0, len(xs), stream_len)]
    checksum = sum(RC.ref_term(p, x) for p, x in enumerate(xs)) & 0xFFFFFFFF
    head = struct.pack("<IHHIII", RC.MAGIC, VERSION_2, c, stream_len, h, w)
    head += b"".join(struct.pack("<f", float(np.float32(s))) for s in scales) + struct.pack("<I", checksum)
    return head + b"".join(struct.pack("<H", len(s)) for s in streams) + b"".join(streams)


def ref_files_v2(pixels, loc, scales, stream_len):
    return join([ref_file_v2(pixels[i], loc[i], scales, stream_len) for i in range(pixels.shape[0])])


def join(files):
    return np.frombuffer(b"".join(files), dtype=np.uint8), np.concatenate([[0], np.cumsum([len(f) for f in files])]).astype(np.int64)


def split(blob, offsets):
    blob = np.asarray(blob, dtype=np.uint8).tobytes()
    return [blob[int(offsets[i]):int(offsets[i + 1])] for i in range(len(offsets) - 1)]


def ref_head_status_v2(data, chw, stream_len, scales):
    """What the version-2 reader answers before it decodes a stream (0: it goes on to the streams), in its order of checks: 6 bytes
    for magic and version, the whole header, the shape, the scale words, the stream length words, the streams' total."""
    c, h, w = chw
    ns = -(-(c * h * w) // stream_len)
    head = header_bytes(c)
    if len(data) < 6:
        return RC.E_TRUNCATED_HEADER
    if struct.unpack_from("<IH", data, 0) != (RC.MAGIC, VERSION_2):
        return RC.E_MAGIC
    if len(data) < head:
        return RC.E_TRUNCATED_HEADER
    if struct.unpack_from("<HIII", data, 6) != (c, stream_len, h, w):
        return RC.E_SHAPE
    words = struct.unpack_from(f"<{c}I", data, 20)
    if any(wd != struct.unpack("<I", struct.pack("<f", float(np.float32(s))))[0] for wd, s in zip(words, scales)):
        return RC.E_SCALE_WORD
    if len(data) < head + 2 * ns:
        return RC.E_TRUNCATED_HEADER
    if head + 2 * ns + sum(struct.unpack_from(f"<{ns}H", data, head)) > len(data):
        return RC.E_TRUNCATED_STREAMS
    return RC.OK


def header_cuts(c, ns, n_bytes):
    """Truncation lengths at every header boundary of a version-2 file (and one byte either side of the last two)."""
    head = header_bytes(c)
    cuts = {0, 4, 5, 6, 8, 12, 16, 20, head - 4, head - 1, head, head + 1, head + 2 * ns - 1, head + 2 * ns, n_bytes - 1}
    cuts |= {20 + 4 * ch for ch in range(c + 1)}
    return sorted(x for x in cuts if 0 <= x < n_bytes)


def damaged_sets(files, v1_files, chw, stream_len, scales, victim=1):
    """[(label, files with the victim's replaced, the victim's expected status)] for header-level damage of image `victim`."""
    c, h, w = chw
    ns = -(-(c * h * w) // stream_len)
    good = files[victim]
    out = []

    def put(label, data):
        data = bytes(data)
        out.append((label, files[:victim] + [data] + files[victim + 1:], ref_head_status_v2(data, chw, stream_len, scales)))
    for ch in range(c):
        bad = bytearray(good)
        bad[20 + 4 * ch] ^= 0x01                                     # the last mantissa bit of one channel's scale word
        put(f"scale_word_ch{ch}", bad)
    put("version_1_file", v1_files[victim])
    for cut in header_cuts(c, ns, len(good)):
        put(f"cut_{cut}", good[:cut])
    bad = bytearray(good)
    bad[6] ^= 0x01
    put("channels_word", bad)
    return out


def another_loc(loc, victim=1):
    """loc with the LAST symbol of image `victim` moved by a quarter of the range towards 0: the decoder reads another pixel there
    (its table is 64 symbols away) and nothing after it, so the streams stay whole and the verdict is the checksum's."""
    moved = loc.copy()
    last = moved[victim].reshape(-1)
    last[-1] -= np.float32(0.25) * np.sign(last[-1])
    return moved


# ---- the cost table -------------------------------------------------------------------------------------------------------------------
def ref_cost_table():
    n = np.arange(1, 65537, dtype=np.float64)
    return np.concatenate([[0], np.rint((16.0 - np.log2(n)) * 65536.0)]).astype(np.int64)


def candidates(c, n_cand, seed=5):
    """scales float32 [c, n_cand]: log-uniform over [e^-7, e^1], each channel its own."""
    rng = np.random.default_rng(seed + n_cand)
    return np.exp(rng.uniform(-7.0, 1.0, size=(c, n_cand))).astype(np.float32)


def plain_scale_bits(res, pixels, loc, scales):
    """bits [n, c, n_cand] from irec_res_symbol_counts and the restated table: sum of cost[count] per (image, channel, candidate)."""
    lib = __import__("irec")._lib.load()
    cost = ref_cost_table()
    n, c = pixels.shape[:2]
    out = np.zeros((n, c, scales.shape[1]), dtype=np.int64)
    for i in range(n):
        for ch in range(c):
            px, lc = np.ascontiguousarray(pixels[i, ch]), np.ascontiguousarray(loc[i, ch])
            for k in range(scales.shape[1]):
                count = np.zeros(px.size, dtype=np.uint32)
                assert lib.irec_res_symbol_counts(px.ctypes.data, lc.ctypes.data, float(scales[ch, k]), px.size, count.ctypes.data) == 0
                out[i, ch, k] = cost[count].sum()
    return out


# ---- the recovery set of the fitter ---------------------------------------------------------------------------------------------------
TRUE_SCALES = (0.01, 0.03, 0.1)


def logistic_images(n=8, size=32, seed=20240611):
    """n images of 3 x size x size: loc uniform in [-0.45, 0.45], pixels = the bin of loc + a logistic draw of the channel's true
    scale (x stands for x / 256 - 0.5, bin k covers [k / 256 - 0.5, (k + 1) / 256 - 0.5))."""
    rng = np.random.default_rng(seed)
    loc = rng.uniform(-0.45, 0.45, size=(n, 3, size, size)).astype(np.float32)
    u = rng.uniform(1e-12, 1.0 - 1e-12, size=loc.shape)
    noise = np.log(u / (1.0 - u)) * np.array(TRUE_SCALES).reshape(1, 3, 1, 1)
    pixels = np.clip(np.floor((loc.astype(np.float64) + noise + 0.5) * 256.0), 0, 255).astype(np.uint8)
    return pixels, loc
