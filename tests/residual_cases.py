"""The cases of the .res tests, and a restatement of the residual model and of its stream coder in plain Python integers and numpy
float64, written from the format's description (DESIGN.md §3 "residual", INTEGRATION.md ".res") and sharing no code with the library.

Model: symbol x in [0, 255]; m = rint(loc * 4096) clamped to [-2048, 2047]; inv = 1 / (4096 s) in float64;
C(0) = 0, C(256) = 65536, C(k) = k + floor(G(k) * 65280), G(k) = 1 / (1 + exp(-(16 k - 2048 - m) * inv)), the argument of exp clamped
to [-700, 700]; exp(x) = 2^k * P(r) with k = floor(x * log2(e) + 1/2), r = (x - k * LN2_HI) - k * LN2_LO and P the degree-13 Taylor
polynomial in Horner form -- every operation a correctly rounded float64 one, in this order.
Checksum: the sum mod 2^32 over an image's symbols of mix(((p << 8) | x) + 0x9E3779B9), p the position, mix the 32-bit finalizer
h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16."""
import struct

import numpy as np

WHOLE, HALF, QUARTER = 1 << 32, 1 << 31, 1 << 30
MAGIC, VERSION, HEADER = 0x53455249, 1, 28
LOG2E, LN2_HI, LN2_LO = 1.4426950408889634, 0.693147180369123816490, 1.90821492927058770002e-10
FACT = [6227020800.0, 479001600.0, 39916800.0, 3628800.0, 362880.0, 40320.0, 5040.0, 720.0, 120.0, 24.0, 6.0]

(OK, E_SCALE, E_LOC, E_TRUNCATED_HEADER, E_MAGIC, E_SHAPE, E_SCALE_WORD, E_TRUNCATED_STREAMS, E_CORRUPT, E_CHECKSUM) = range(10)


def ref_exp(x):
    """float64 array in [-700, 700] -> exp, by the written operation sequence."""
    x = np.asarray(x, dtype=np.float64)
    kf = np.floor(x * LOG2E + 0.5)
    r = (x - kf * LN2_HI) - kf * LN2_LO
    p = np.full_like(x, 1.0 / FACT[0])
    for f in FACT[1:]:
        p = p * r + 1.0 / f
    p = p * r + 0.5
    p = p * r + 1.0
    p = p * r + 1.0
    return p * np.ldexp(1.0, kf.astype(np.int64))


def ref_counts(m, scale):
    """C(0 .. 256) of one (m, scale) as int64 [257]."""
    inv = 1.0 / (4096.0 * float(np.float32(scale)))
    k = np.arange(1, 256, dtype=np.int64)
    t = np.clip((16 * k - 2048 - int(m)).astype(np.float64) * inv, -700.0, 700.0)
    G = 1.0 / (1.0 + ref_exp(-t))
    C = np.zeros(257, dtype=np.int64)
    C[1:256] = k + np.floor(G * 65280.0).astype(np.int64)
    C[256] = 65536
    return C


def ref_m(loc):
    v = np.float32(loc) * np.float32(4096.0)
    return int(min(max(np.rint(v), -2048), 2047))


def ref_term(p, x):
    h = ((((p << 8) & 0xFFFFFFFF) | x) + 0x9E3779B9) & 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    return h ^ (h >> 16)


class _Tables:
    def __init__(self, scale):
        self.scale, self.cache = scale, {}

    def __call__(self, m):
        if m not in self.cache:
            self.cache[m] = [int(c) for c in ref_counts(m, self.scale)]
        return self.cache[m]


def ref_encode_stream(xs, ms, tables):
    """The code bits (a list of 0 / 1) of symbols xs under the tables of ms."""
    low, high, s, bits = 0, WHOLE, 0, []

    def put(bit, follow):
        bits.append(bit)
        bits.extend([bit ^ 1] * follow)
    for x, m in zip(xs, ms):
        C = tables(m)
        width = high - low
        high = low + ((width * C[x + 1]) >> 16)
        low = low + ((width * C[x]) >> 16)
        while high < HALF or low > HALF:
            if high < HALF:
                put(0, s); s = 0; low *= 2; high *= 2
            else:
                put(1, s); s = 0; low = (low - HALF) * 2; high = (high - HALF) * 2
        while low > QUARTER and high < 3 * QUARTER:
            s += 1; low = (low - QUARTER) * 2; high = (high - QUARTER) * 2
    s += 1
    put(0 if low <= QUARTER else 1, s)
    return bits


def ref_pack(bits):
    bits = list(bits) + [0] * (-len(bits) % 8)
    return bytes(int("".join(map(str, bits[i:i + 8])), 2) for i in range(0, len(bits), 8))


def ref_file(pixels, loc, scale, stream_len):
    """The .res file of one image: pixels [C, H, W] uint8, loc the same shape float32."""
    c, h, w = pixels.shape
    xs = [int(v) for v in pixels.reshape(-1)]
    ms = [ref_m(v) for v in loc.reshape(-1)]
    tables = _Tables(scale)
    streams = [ref_pack(ref_encode_stream(xs[k:k + stream_len], ms[k:k + stream_len], tables)) for k in range(0, len(xs), stream_len)]
    checksum = sum(ref_term(p, x) for p, x in enumerate(xs)) & 0xFFFFFFFF
    scale_word = struct.unpack("<I", struct.pack("<f", float(np.float32(scale))))[0]
    head = struct.pack("<IHHIIIII", MAGIC, VERSION, c, stream_len, h, w, scale_word, checksum)
    return head + b"".join(struct.pack("<H", len(s)) for s in streams) + b"".join(streams)


def ref_files(pixels, loc, scale, stream_len):
    files = [ref_file(pixels[i], loc[i], scale, stream_len) for i in range(pixels.shape[0])]
    return np.frombuffer(b"".join(files), dtype=np.uint8), np.concatenate([[0], np.cumsum([len(f) for f in files])]).astype(np.int64)


def ref_model_bits(pixels, loc, scale):
    """The ideal bits per image from the referee's counts."""
    tables = _Tables(scale)
    out = []
    for i in range(pixels.shape[0]):
        bits = 0.0
        for x, v in zip(pixels[i].reshape(-1), loc[i].reshape(-1)):
            C = tables(ref_m(v))
            bits += 16.0 - np.log2(float(C[int(x) + 1] - C[int(x)]))
        out.append(bits)
    return np.array(out)


# ---- the cases: name -> (pixels [N, C, H, W] uint8, loc float32, scale, stream_len) ---------------------------------------------------
CLAMP_LO, CLAMP_HI = -0.5 + 1.0 / 512.0, 0.5 - 1.0 / 512.0


def _near(rng, shape, spread):
    """loc in the clamp range and pixels within `spread` symbols of it."""
    loc = rng.uniform(CLAMP_LO, CLAMP_HI, size=shape).astype(np.float32)
    centre = np.floor((loc + 0.5) * 256.0)
    pixels = np.clip(centre + rng.integers(-spread, spread + 1, size=shape), 0, 255).astype(np.uint8)
    return pixels, loc


def make_cases():
    rng = np.random.default_rng(20240607)
    cases = {}
    p, l = _near(rng, (2, 3, 2, 2), 6)
    cases["ragged_2x2_L5"] = (p, l, 0.05, 5)                       # 12 symbols: streams of 5, 5, 2
    cases["L1"] = (p, l, 0.05, 1)
    cases["one_stream"] = (p, l, 0.05, 4096)                       # L >= 3 H W
    ends = np.zeros((1, 3, 2, 2), dtype=np.uint8)
    ends.reshape(-1)[::2] = 255
    loc_ends = np.full((1, 3, 2, 2), CLAMP_LO, dtype=np.float32)
    loc_ends.reshape(-1)[[2, 3, 6, 7, 10, 11]] = CLAMP_HI           # pixels 0 and 255 under loc at both clamp ends
    cases["clamp_ends"] = (ends, loc_ends, 0.05, 5)
    far = rng.integers(0, 256, size=(1, 3, 4, 4)).astype(np.uint8)
    loc_far = rng.uniform(CLAMP_LO, CLAMP_HI, size=(1, 3, 4, 4)).astype(np.float32)
    cases["tiny_scale_far"] = (far, loc_far, 1e-4, 16)             # count-1 symbols, 16 bits each, long follow-bit runs
    p2, l2 = _near(rng, (2, 3, 4, 4), 100)
    cases["near_uniform"] = (p2, l2, 100.0, 7)
    cases["all_equal"] = (np.full((1, 3, 4, 4), 77, dtype=np.uint8), np.full((1, 3, 4, 4), 77 / 256.0 - 0.5 + 1 / 512.0, dtype=np.float32), 2.0 ** -8, 5)
    return cases


def size_allowance_bits(c, h, w, stream_len):
    """Bits a file may take beyond the ideal (test_residual_host.test_size_bound has the derivation)."""
    n_sym = c * h * w
    ns = -(-n_sym // stream_len)
    return 8 * HEADER + ns * (16 + 2 + 7) + n_sym * np.log2(1.0 / (1.0 - 2.0 ** -14))
