"""Index rows no encoder would write, for every decoder build (tests/test_decode_corners_host.py, tests/test_decode_corners_gpu.py).

The decoder compares no scores: for any row (K, indices) in the domain every decode mode returns the reference's decode_block
(rec/coding/beam_search_coder.py:124-148) bit for bit, and a row outside the domain decodes to p.loc.  So rows can be written down:
K on the edges of the 64-step lane vector and of the table window, the first and the last sample index, garbage behind K.

numpy only.  The priors are laid out in SHUFFLED order (Coder.split's, coder.py:62-83) and scattered through the permutation, so that
"dims [4, 8)" of a family are one lane quad of the first unit of a tensor's first block whatever the shuffle.

dispatch() restates which __global__ build of csrc/irec_decode.hip a call takes: make_dec_plan (csrc/irec_host.cpp), decode_tensor_waves
and launch_decode (csrc/irec_decode.hip), with the constants of include/irec.h and csrc/irec_kernels.h they read."""
import collections
import functools

import numpy as np

SEED = 42
PAD = 0x7FFFFFFF                            # every entry of an index row behind K
MODES = ("auto", "tables", "fused", "legacy", "tensors", "tensors_fused")
TABLE_STEPS = (0, 64, 128)                  # 0: the default window
FAMILIES = ("plain", "wide", "zeros", "tiny_quad", "offset")
K_LADDER = (0, 1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 66, 67, 127, 128, 129, 193)
MAX_K = 200

# ---- the library's constants (include/irec.h, csrc/irec_kernels.h, csrc/irec_decode.hip) ------------------------------------------------
TABLE_STEPS_DEFAULT, TABLE_STEPS_MAX, TABLE_STEPS_FLOOR = 32, 4096, 8
TABLE_BYTES_MAX, TABLE_BYTES_HARD = 64 << 20, 1 << 30
LDS_LIMIT = 160 * 1024                      # FAST_LDS_LIMIT
DEC_LUT_BYTES, DEC_DLOG_BYTES = 40032, 20016
DEC_WMAX, DEC_RMAX_SMALL, DEC_RMAX_BIG = 12, 3, 5
MAX_SAMPLES = 1 << 24                       # check_params: n_samples at most


def _ceil(a, b):
    return -(-a // b)


def _up(a, b):
    return _ceil(a, b) * b


class Lay(collections.namedtuple("Lay", "n_tensors n block_size")):
    """n_tensors tensors of n dims in blocks of block_size dims (the last one short): what engine.layout() describes."""
    __slots__ = ()

    @property
    def bs(self):
        return min(self.block_size, self.n)

    @property
    def bpt(self):
        return _ceil(self.n, self.bs)

    @property
    def n_blocks(self):
        return self.n_tensors * self.bpt

    @property
    def block_dims(self):
        """Dims of block j of a tensor, j = 0 .. bpt - 1."""
        return [min(self.bs, self.n - j * self.bs) for j in range(self.bpt)]

    @property
    def distinct_dims(self):
        return sorted(set(self.block_dims), reverse=True)


# ---- the dispatch, restated ---------------------------------------------------------------------------------------------------------------
def tensor_waves(n, bs, table):
    """decode_tensor_waves: (waves per workgroup, LDS bytes) of the staged decode, (0, 0) where the tensor does not fit."""
    if n < 1 or bs < 1:
        return 0, 0
    upt = _ceil(n, bs) * _ceil(bs, 256)
    lds = DEC_LUT_BYTES + (0 if table else DEC_DLOG_BYTES) + _up(4 * n, 16) + 16
    if _ceil(upt, DEC_WMAX) > DEC_RMAX_BIG or lds > LDS_LIMIT:
        return 0, 0
    return min(upt, DEC_WMAX), lds


def staged_rmax(n, bs):
    """DEC_RMAX of the decode_tensor_kernel build launch_decode picks for tensors of n dims in blocks of bs."""
    bs = min(bs, n)
    nw, _ = tensor_waves(n, bs, True)
    assert nw > 0, (n, bs)
    upt = _ceil(n, bs) * _ceil(bs, 256)
    return DEC_RMAX_SMALL if _ceil(upt, nw) <= DEC_RMAX_SMALL else DEC_RMAX_BIG


def tensors_supported(n, bs):
    """irec_decode_tensors_supported."""
    if n < 1 or bs < 1:
        return False
    bs = min(bs, n)
    return tensor_waves(n, bs, True)[0] > 0 and tensor_waves(n, bs, False)[0] > 0


def staged_grid(n_cu, lay, table):
    """Workgroups launch_decode starts for the staged decode of `lay`."""
    _, lds = tensor_waves(lay.n, lay.bs, table)
    per_cu = 1 if LDS_LIMIT // lds < 2 else 2
    return min(lay.n_tensors, per_cu * n_cu)


def _table_window(dims, S, max_K, table_steps):
    per_step = sum(S * _up(d, 4) * 2 for d in dims)
    kt = min(table_steps if table_steps > 0 else TABLE_STEPS_DEFAULT, TABLE_STEPS_MAX, max_K)
    return min(kt, max(TABLE_BYTES_MAX // per_step, min(TABLE_STEPS_FLOOR, TABLE_BYTES_HARD // per_step)))


def workspace_bytes(dims, S, max_K, table_steps, fused=False):
    """irec_decode_workspace_bytes of parameters with table_dims = dims (at most four, 0 none)."""
    dims = [d for d in dims if d > 0]
    if not dims or max_K < 1 or fused:
        return 0
    kt = _table_window(dims, S, max_K, table_steps)
    return sum(_up(kt * S * _up(d, 4) * 2, 256) for d in dims) if kt >= 1 else 0


def k_tab(dims, S, max_K, table_steps, n_blocks, have_ws, fused=False):
    """make_dec_plan's table window of a call: 0 = no tables (the draw is fused into the kernel)."""
    dims = [d for d in dims if d > 0]
    if not have_ws or not dims or max_K < 1 or fused or S > 2 * n_blocks:
        return 0
    return max(_table_window(dims, S, max_K, table_steps), 0)


def dispatch(n_cu, mode, lay, S, max_K, table_steps=0):
    """(name of the __global__ build as kernel_names.compiled_kernels() spells it, K_tab) of engine.decode_blocks(mode=mode) on a device
    of n_cu compute units; (None, 0) where the mode does not apply to the layout."""
    b = lambda v: "true" if v else "false"
    dims = lay.distinct_dims
    fits = tensors_supported(lay.n, lay.bs)
    if mode == "auto":
        mode = "tensors" if fits else "tables"
    if mode in ("tensors", "tensors_fused"):
        if not fits:
            return None, 0
        fused = mode == "tensors_fused"
        have_ws = workspace_bytes(dims, S, max_K, table_steps, fused) > 0
        kt = k_tab(dims, S, max_K, table_steps, lay.n_blocks, have_ws, fused)
        return f"decode_tensor_kernel<{b(kt > 0)},{staged_rmax(lay.n, lay.bs)}>", kt
    if mode == "legacy":                                      # no dim hints: the unit count per block is not known
        return f"decode_kernel<{b(lay.n_blocks >= 16 * n_cu)}>", 0
    if mode == "fused":                                       # dim hints, no workspace
        return "decode_wave_kernel<false>", 0
    assert mode == "tables", mode
    have_ws = workspace_bytes(dims, S, max_K, table_steps) > 0
    kt = k_tab(dims, S, max_K, table_steps, lay.n_blocks, have_ws)
    return f"decode_wave_kernel<{b(kt > 0)}>", kt


# ---- priors and rows ------------------------------------------------------------------------------------------------------------------------
def prior(D, family, seed):
    """(mp, sp) float32 [D]."""
    rng = np.random.default_rng([FAMILIES.index(family), int(D), int(seed)])
    mp = rng.normal(0.0, 1.0, D).astype(np.float32)
    sp = np.exp(rng.normal(0.0, 6.0 if family == "wide" else 0.25, D)).astype(np.float32)
    if family == "zeros":
        sp[2::3] = 0.0                                        # every third dim: next to ordinary ones in every quad
    elif family == "tiny_quad":
        sp[4:8] *= np.float32(1e-16)                          # sigma_p^2 ~ 1e-32 < 2^-96: one lane of one unit leaves the fast sqrt
    elif family == "offset":
        mp += np.float32(200.0)
    return mp, sp


def rows(S, Ks, max_K, seed):
    """(K int32 [len(Ks)], indices int32 [len(Ks), max_K]): uniform indices in [0, S), the last sample at step 1 and the first at
    step 2 where the row is that long, PAD behind K."""
    rng = np.random.default_rng([int(S), int(max_K), int(seed)])
    K = np.asarray(Ks, dtype=np.int32)
    idx = np.full((len(K), max_K), PAD, dtype=np.int32)
    for b, k in enumerate(K):
        k = int(k)
        if 0 < k <= max_K:
            idx[b, :k] = rng.integers(0, S, k)
            if k > 1:
                idx[b, 1] = S - 1
            if k > 2:
                idx[b, 2] = 0
    return K, idx


def ladder_Ks(lay, ladder=K_LADDER):
    """Block j of tensor i takes ladder[(i + j) % len]: natural (tensor, block) order."""
    return [ladder[(i + j) % len(ladder)] for i in range(lay.n_tensors) for j in range(lay.bpt)]


class Case:
    """One decode call: layout, S, priors [n_tensors, n], rows in natural (tensor, block) order, the blocks that are not decodable."""

    def __init__(self, name, lay, S, family="plain", max_K=MAX_K, Ks=None, seed=0, modes=MODES, table_steps=TABLE_STEPS):
        self.name, self.lay, self.S, self.family, self.max_K, self.seed = name, lay, S, family, max_K, seed
        self.modes, self.table_steps = tuple(modes), tuple(table_steps)
        self.K, self.idx = rows(S, ladder_Ks(lay) if Ks is None else Ks, max_K, seed)
        self.bad = set()                                      # natural block numbers that decode to p.loc
        self.aux = None                                       # fitted auxiliary-variance ratios of the call's context, or None

    def priors(self, perm):
        """(p_loc, p_scale) float32 [n_tensors, n]; perm: the shuffle of the layout (oracle.tf_shuffle_perm(SEED, n))."""
        lay = self.lay
        mp, sp = np.empty((lay.n_tensors, lay.n), np.float32), np.empty((lay.n_tensors, lay.n), np.float32)
        for i in range(lay.n_tensors):
            m, s = prior(lay.n, self.family, 1000 * self.seed + i)
            mp[i, perm], sp[i, perm] = m, s
        return mp, sp

    def routes(self, n_cu):
        """[(mode, table_steps, build, K_tab)] of every call the GPU test makes of this case."""
        out = []
        for mode in self.modes:
            for ts in self.table_steps:
                name, kt = dispatch(n_cu, mode, self.lay, self.S, self.max_K, ts)
                if name is not None:
                    out.append((mode, ts, name, kt))
        return out

    def __repr__(self):
        return f"Case({self.name})"


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------------
N_LADDER = len(K_LADDER)
LADDER_LAYOUTS = ((1, 1), (7, 4), (261, 256), (512, 255), (514, 257), (2047, 1024), (2050, 1025))
# (n, block_size) -> (unit slots, build, float4 staging) of the staged kernel; 9473 adds a last block of one dim to the big build
STAGED_LAYOUTS = {(9216, 256): (36, 3, True), (9472, 256): (37, 5, True), (9470, 256): (37, 5, False), (9473, 256): (38, 5, False),
                  (15360, 256): (60, 5, True), (1, 1): (1, 3, False)}
STAGED_UNSUPPORTED = (15361, 256)


def ladder_S(n):
    return 20 if n >= 2047 else 36


def ladder_families(n, bs):
    return FAMILIES if (n, bs) == (261, 256) else ("plain", "zeros", "tiny_quad")


@functools.lru_cache(maxsize=None)
def ladder_case(n, bs, family):
    return Case(f"ladder-{n}-{bs}-{family}", Lay(N_LADDER, n, bs), ladder_S(n), family, seed=n + bs)


@functools.lru_cache(maxsize=None)
def staged_case(n, bs):
    # (one wave: six samples, so that three blocks share rows and the call builds tables -- make_dec_plan's n_samples <= 2 n_blocks)
    return Case(f"staged-{n}-{bs}", Lay(3, n, bs), 6 if n == 1 else 20, seed=n, modes=("tensors", "tensors_fused"), table_steps=(0, 128))


@functools.lru_cache(maxsize=None)
def loop_case(n_cu):
    """Three passes of the staged kernel's tensor loop for some workgroups, two for the others (two workgroups per CU)."""
    return Case(f"loop-{n_cu}", Lay(4 * n_cu + 3, 70, 7), 20, seed=3, table_steps=(0,))


@functools.lru_cache(maxsize=None)
def grid_case(n_cu, ragged=False):
    """16 blocks per CU and more: decode_kernel<true> in legacy mode.  ragged: blocks of 4 and 3 dims (a partial quad, less than a quad)."""
    if ragged:
        c = Case(f"grid-ragged-{n_cu}", Lay(8 * n_cu + 2, 7, 4), 36, seed=5, table_steps=(0,))
        assert c.K[12] == 31
        c.K[9], c.idx[12, 30] = -1, c.S                       # two rows that are not decodable, for the build no other case gives any
        c.bad = {9, 12}
        return c
    return Case(f"grid-{n_cu}", Lay(16 * n_cu + 4, 8, 8), 36, seed=4, table_steps=(0,))


WRAP_SUMS = (0, 1157627835, -1962934411, -771752146, 436207334, 1660944029)
WRAP_HASHES = {"int32": (1, 3678, 2646, 629, 5771, 8066), "uint32": (1, 3678, 4508, 2491, 5771, 8066),
               "int64": (1, 3678, 4508, 2491, 7633, 9928)}


@functools.lru_cache(maxsize=None)
def wrap_case():
    """The int32 hash sum wraps negative (before steps 2 and 3) and positive again (before 4 and 5): S = 2^24, every index S - 1."""
    S, K = MAX_SAMPLES, 6
    c = Case("wrap", Lay(1, 3, 2), S, max_K=8, Ks=[K, K], seed=6, table_steps=(0,))
    c.idx[:, :K] = S - 1
    true = np.cumsum([0] + [(S - 1) * (69 + t) for t in range(K - 1)]).tolist()
    i32 = [((s + (1 << 31)) % (1 << 32)) - (1 << 31) for s in true]
    assert tuple(i32) == WRAP_SUMS
    assert tuple(s % 10006 + 1 for s in i32) == WRAP_HASHES["int32"]             # (Python's % is floormod)
    assert tuple((s % (1 << 32)) % 10006 + 1 for s in true) == WRAP_HASHES["uint32"]
    assert tuple(s % 10006 + 1 for s in true) == WRAP_HASHES["int64"]
    # the three groups: all readings agree | wrapped negative | past 2^32 and positive again
    assert [s == t for s, t in zip(i32, true)] == [True, True, False, False, False, False]
    assert [s < 0 for s in i32] == [False, False, True, True, False, False] and all(t >= 1 << 32 for t in true[4:])
    h = WRAP_HASHES
    assert all(h["int32"][t] == h["uint32"][t] == h["int64"][t] for t in (0, 1))
    assert all(h["int32"][t] != h["uint32"][t] == h["int64"][t] for t in (2, 3))
    assert all(h["int32"][t] == h["uint32"][t] != h["int64"][t] for t in (4, 5))
    return c


BAD_LAYOUTS = ((261, 256), (9472, 256))
BAD_PLANTS = ((0, "S"), (63, "S"), (64, "S"), (128, "S"), (70, -1), (3, PAD))   # (step, value); "S": n_samples, the first value past the domain


@functools.lru_cache(maxsize=None)
def bad_case(n, bs):
    """Eight separate blocks that are not decodable among ordinary ones: six rows of K = 129 with one entry that is no sample index,
    K = -1 and K = max_K + 1.  On (261, 256) they take blocks of both dims."""
    base = ladder_case(n, bs, "plain") if (n, bs) in LADDER_LAYOUTS else staged_case(n, bs)
    lay, S = base.lay, base.S
    Ks = ladder_Ks(lay)
    at = [2 + (3 if lay.n_blocks < 104 else 13) * k for k in range(8)]           # (an odd stride: full and short blocks in turn)
    assert max(at) < lay.n_blocks and len({lay.block_dims[b % lay.bpt] for b in at}) == len(lay.distinct_dims)
    for b in at[:6]:
        Ks[b] = 129
    c = Case(f"bad-{n}-{bs}", lay, S, Ks=Ks, seed=7 + n, table_steps=(0, 128))
    for b, (t, v) in zip(at[:6], BAD_PLANTS):
        c.idx[b, t] = S if v == "S" else v
    c.K[at[6]], c.K[at[7]] = -1, MAX_K + 1
    c.idx[at[6]] = PAD
    c.bad = set(at)
    return c


AUX_RATIOS = (1.0, 0.62, 0.45, 0.37, 0.3, 0.27, 0.22, 0.2)   # a ratio table of 8 entries: K = 8 is the last row it covers


@functools.lru_cache(maxsize=None)
def fitted_case():
    """Rows of K = 8 (and a few shorter) and of K = 9 under a context whose ratio table has 8 entries: K = 9 decodes to p.loc."""
    lay = Lay(N_LADDER, 261, 256)
    Ks = [(8, 9, 8, 9, 5, 9, 8, 1)[(i + 3 * j) % 8] for i in range(lay.n_tensors) for j in range(lay.bpt)]
    c = Case("fitted", lay, 36, max_K=16, Ks=Ks, seed=8, table_steps=(0,))
    c.bad = {b for b, k in enumerate(Ks) if k > len(AUX_RATIOS)}
    c.aux = np.asarray(AUX_RATIOS, dtype=np.float32)
    return c


def all_cases(n_cu):
    """Every case of tests/test_decode_corners_gpu.py on a device of n_cu compute units."""
    out = [ladder_case(n, bs, f) for n, bs in LADDER_LAYOUTS for f in ladder_families(n, bs)]
    out += [staged_case(n, bs) for n, bs in STAGED_LAYOUTS]
    out += [loop_case(n_cu), grid_case(n_cu), grid_case(n_cu, True), wrap_case(), fitted_case()]
    out += [bad_case(n, bs) for n, bs in BAD_LAYOUTS]
    return out


# ---- what the oracle says (cached: the CPU side is the cost of these tests) ---------------------------------------------------------------
_perms, _expected = {}, {}


def perm_of(n):
    from oracle import oracle as O
    if n not in _perms:
        _perms[n] = O.tf_shuffle_perm(SEED, n)
    return _perms[n]


def expected(case):
    """(p_loc, p_scale, want) float32 [n_tensors, n], read-only: the oracle's decode_block of every decodable block, merged through the
    shuffle, and p_loc on the blocks of case.bad.  Cached per case name."""
    if case.name in _expected:
        return _expected[case.name]
    from oracle import oracle as O
    lay = case.lay
    perm = perm_of(lay.n)
    mp, sp = case.priors(perm)
    want = mp.copy()
    if case.aux is not None:
        O.set_aux_ratios(case.aux)
    try:
        for i in range(lay.n_tensors):
            for j, (lo, hi) in enumerate(O.split_blocks(lay.n, lay.bs)):
                b = i * lay.bpt + j
                if b in case.bad:
                    continue
                g = perm[lo:hi]
                want[i, g] = O.decode_block(mp[i, g], sp[i, g], case.idx[b, :case.K[b]], SEED, case.S)
    finally:
        if case.aux is not None:
            O.set_aux_ratios(None)
    for a in (mp, sp, want):
        a.setflags(write=False)
    _expected[case.name] = (mp, sp, want)
    return _expected[case.name]
