"""The seed domain: the ladder of coding seeds, the seeds a file header cannot hold, and the inputs and calls the seed tests run
(tests/test_seed_domain_host.py, tests/test_seed_domain_gpu.py, tests/golden/make_golden_refpy_seeds.py).

The seed is the one input that reaches every random stream of the product: the shuffle of a layout, the Philox step seeds seed + t of
every encoder and decoder, the normal and Gumbel tables of the importance coder, the normal table of the ratio fit, and the header
of every .rec / .recs file.  The rules (include/irec.h, "Seeds"):
  * the step seed seed + t is reduced modulo M = 2^31 - 1 (TensorFlow's truncation of both halves of a seed pair), and the residue 0
    becomes the pair (0, M): make_step_seed of csrc/irec_device.h;
  * a coding seed is any int64 up to SEED_BOUND = INT64_MAX - 65538, so that no seed + step overflows;
  * a seed that goes into a file header lies in [0, 2^32).

The ladder.  With a table window of TABLE_STEPS = 4 steps and blocks of K >= 8 partitions (check_partitions):
  0                the first step is the zero step, the pair (0, M)
  M - 1, M - 3     the zero step is step 1 / step 3: inside the table window
  M - 6            the zero step is step 6: in the fused draw behind the window
  M, 2M - 3        congruent to 0 and to M - 3: the same bits are demanded (seeds congruent mod M code identically)
  2^31, 2^32 - 1   the first seeds an int32 / a uint32 cannot hold; 2^32 - 1 is the last a header can
  2^32 + 5         what a uint32 field would wrap to 5
  -1, -M - 3       negative: the residue of a C `%` is negative and has to be lifted (-M - 3 is congruent to M - 3)
  2^40 + 5         the high word of the table stamps
  SEED_BOUND       the largest coding seed
"""
import functools

import numpy as np

M = 2 ** 31 - 1
INT64_MAX = 2 ** 63 - 1
SEED_BOUND = INT64_MAX - 65538                    # IREC_SEED_MAX: INT64_MAX - (IREC_MAX_PARTITIONS + 2)
SEEDS = (0, M - 1, M - 3, M - 6, M, 2 * M - 3, 2 ** 31, 2 ** 32 - 1, 2 ** 32 + 5, -1, -M - 3, 2 ** 40 + 5, SEED_BOUND)
CONGRUENT = ((M, 0), (2 * M - 3, M - 3), (-M - 3, M - 3))     # (seed, the ladder seed it is congruent to mod M)
HEADER_BAD = (-1, 2 ** 32, 2 ** 32 + 5, 2 ** 63)
HEADER_GOOD = (2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1)               # the seeds the file tests round-trip
TABLE_STEPS = 4
MIN_K = 8                                          # the zero step of M - 6 is step 6: a block of K >= 8 runs it and one more


def seed_id(seed):
    """A readable test id: the seed as an offset from the power of two or the multiple of M it sits at."""
    names = {0: "0", M - 1: "M-1", M - 3: "M-3", M - 6: "M-6", M: "M", 2 * M - 3: "2M-3", 2 ** 31: "2^31", 2 ** 32 - 1: "2^32-1",
             2 ** 32 + 5: "2^32+5", -1: "-1", -M - 3: "-M-3", 2 ** 40 + 5: "2^40+5", SEED_BOUND: "bound", 2 ** 32: "2^32", 2 ** 63: "2^63"}
    return names.get(seed, str(seed))


@functools.lru_cache(maxsize=None)
def inputs(dim, n_blocks):
    """(mq, sq, mp, sp), each float32 [n_blocks, dim], read-only: block j is latent_families.block("sharp", dim, j, 1.0, 32) -- one
    informative dim of up to ~22 nats in benign ones (with the oracle at Omega = 1 and 64 dims: K = 10 for block 0, 5 to 23 over the
    first dozen blocks; check_partitions is what every case asserts of them)."""
    import latent_families as L
    host = L.stack([L.block("sharp", dim, j, 1.0, 32) for j in range(n_blocks)])
    for a in host:
        a.setflags(write=False)
    return host


def check_partitions(Ks, what):
    """The condition of every case, from the oracle's K alone: at least a third of the blocks have K >= MIN_K partitions, so that the
    zero step of M - 1, M - 3 and M - 6 lies inside the steps actually run (with TABLE_STEPS = 4: that of M - 3 in the table, that of
    M - 6 in the fused draw behind it).  A condition on the inputs, not a tolerance."""
    Ks = np.asarray(Ks).reshape(-1)
    assert 3 * int((Ks >= MIN_K).sum()) >= Ks.size, (what, Ks.tolist())


# ---- the encoder calls: one per family of kernel_names.FAMILIES ------------------------------------------------------------------------
def _plan(n_cu, omega, S, B, flags, dim, n_blocks, max_K):
    """The canonical kernel name irec_test_plan gives a call with a table window of TABLE_STEPS on a device of n_cu compute units."""
    import ctypes
    import kernel_names as kn
    lib, _lib, Engine = kn._planner()
    info, det = _lib.IrecPlanInfo(), _lib.IrecPlanDetail()
    p = Engine.params(omega, S, B, flags, [dim], TABLE_STEPS)
    st = lib.irec_test_plan(n_cu, 2400, ctypes.byref(p), n_blocks, dim, max_K, ctypes.byref(info), ctypes.byref(det))
    assert st == 0, lib.irec_last_error()
    return kn.canonical(info.kernel.decode(), info.split)


@functools.lru_cache(maxsize=None)
def family_cases(n_cu=256):
    """family -> dict(name, B, S, n_blocks, flags, dim, max_K, omega): the family's cheapest planned name (kernel_names.family_members)
    with its B, S, flags and block count, at 64 dims -- 192 where the name does not serve 64 --, the chunk families at 1025 dims under
    the Omega kernel_names.call_stats finds for them, the others under Omega = 1 (the inputs' own); the next cheapest name where the
    planner gives that call another kernel.  None for a family the planner names no kernel of."""
    import kernel_names as kn
    from oracle import oracle as O
    plans = kn.enumerate_plans(n_cu)
    out = {}
    for family in kn.FAMILIES:
        out[family] = None
        for name in kn.family_members(plans, family):
            ex = plans[name]
            for dim in ((1025,) if name.startswith("encode_chunk_kernel<") else (64, 192)):
                omega = kn.call_stats(O, dim, ex["n_blocks"])[0] if dim > 1024 else 1.0
                if _plan(n_cu, omega, ex["S"], ex["B"], ex["flags"], dim, ex["n_blocks"], kn.max_K_of(dim)) == name:
                    out[family] = dict(name=name, B=ex["B"], S=ex["S"], n_blocks=ex["n_blocks"], flags=ex["flags"], dim=dim,
                                       max_K=kn.max_K_of(dim), omega=omega)
                    break
            if out[family]:
                break
    return out


@functools.lru_cache(maxsize=None)
def encoder_reference(family, seed, n_cu=256):
    """(indices [n_blocks][K], sample [n_blocks, dim]) of oracle.encode_tensors_omp for a family's call at one seed, one block a
    tensor (the engine's layout of n_blocks tensors of dim dims in blocks of dim); the partition condition is asserted here."""
    from oracle import oracle as O
    c = family_cases(n_cu)[family]
    ridx, rs, _ = O.encode_tensors_omp(*inputs(c["dim"], c["n_blocks"]), seed, c["omega"], c["S"], c["B"], c["dim"], max_K=c["max_K"])
    ridx = [r[0] for r in ridx]
    check_partitions([len(r) for r in ridx], (family, seed_id(seed)))
    rs.setflags(write=False)
    return ridx, rs


# ---- the decoder layouts ----------------------------------------------------------------------------------------------------------------------
DECODE_LAYOUTS = {"3x448": (3, 448, 192), "4x1000": (1, 4000, 1000)}    # id -> (tensors, dims of a tensor, block_size)


@functools.lru_cache(maxsize=None)
def tensor_inputs(n_tensors, n):
    """inputs() for whole tensors: tensor i is the sharp block of n dims of seed i."""
    return inputs(n, n_tensors)
