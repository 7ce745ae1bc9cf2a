"""The seed domain without a GPU (tests/seed_cases.py has the ladder and the rules):
  (a) the host streams a seed reaches -- the shuffle, the Philox uniform draw, the normal and the Gumbel tables of the importance coder
      -- equal the oracle's at every seed of the ladder, bit for bit;
  (b) a .rec / .recs header holds a seed of [0, 2^32) only: RecHeader.pack and every host writer round-trip 2^32 - 1 and refuse every
      seed of HEADER_BAD before a byte exists (ctypes would wrap them into the uint32 field: 2^32 + 5 -> 5, and the file would decode
      under another seed to another image, without an error);
  (c) the C entry points that take a coding seed answer IREC_E_INVALID above IREC_SEED_MAX = INT64_MAX - 65538, name the seed in
      irec_last_error, write nothing, and accept the bound itself;
  (d) Python refuses an int that does not fit int64 instead of handing ctypes a value it wraps.
"""
import ctypes
import ctypes.util
import os

import numpy as np
import pytest
import torch

import seed_cases as SC

pytestmark = [pytest.mark.both_suites, pytest.mark.usefixtures("suite")]

SIZES = (1, 2, 65, 1000)
_ids = [SC.seed_id(s) for s in SC.SEEDS]
_bad_ids = [SC.seed_id(s) for s in SC.HEADER_BAD]


# ==== (a) the host streams ==================================================================================================================
@pytest.mark.parametrize("seed", SC.SEEDS, ids=_ids)
def test_shuffle_and_uniform_draw_equal_the_oracle(oracle, seed):
    from irec import engine
    for n in SIZES:
        assert np.array_equal(engine.tf_shuffle_perm(seed, n), oracle.tf_shuffle_perm(seed, n)), n
        assert np.array_equal(engine.philox_uniform_int(seed, n), oracle.uniform_int(seed, n)), n


def test_congruent_seeds_draw_the_same_uniforms_and_other_shuffles(oracle):
    """The Philox draw of the beam-search coders sees seed mod M only; the shuffle's op seed is CPython's random.Random(seed), which sees
    every bit -- so congruent seeds code a block identically but cut a tensor into other blocks.  Both as the oracle has them."""
    from irec import engine
    for seed, twin in SC.CONGRUENT:
        assert np.array_equal(engine.philox_uniform_int(seed, 1000), engine.philox_uniform_int(twin, 1000)), (seed, twin)
        assert oracle.py_first_randint31(seed) != oracle.py_first_randint31(twin)
        assert not np.array_equal(engine.tf_shuffle_perm(seed, 1000), engine.tf_shuffle_perm(twin, 1000)), (seed, twin)


@pytest.mark.parametrize("seed", SC.SEEDS, ids=_ids)
def test_normal_table_equals_the_oracle(oracle, seed):
    """entry [j, d, s] = element s * dim + d of the stream of seed + j (include/irec.h); n = S * dim elements a step."""
    from irec.engine import build_normal_table
    steps = 3
    for S, dim in ((1, 1), (2, 1), (13, 5), (40, 25)):                    # 1, 2, 65 and 1000 elements a step
        tab = build_normal_table(seed, S, dim, steps)
        assert tab.shape == (steps, dim, -(-S // 16) * 16)
        for j in range(steps):
            want = oracle.tf_random_normal(seed + j, S * dim).reshape(S, dim).T
            assert np.array_equal(tab[j, :, :S], want), (S, dim, j)
            assert not tab[j, :, S:].any()


_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.logf.restype, _libm.logf.argtypes = ctypes.c_float, [ctypes.c_float]


def _gumbel_of(z):
    """-logf(-logf(z)) with libm's float32 logarithm, element by element (rec/coding/utils.py:9-12 as the library states it)."""
    out = np.empty(z.size, dtype=np.float32)
    with np.errstate(all="ignore"):
        for i, v in enumerate(z.tolist()):
            out[i] = -_libm.logf(np.float32(-_libm.logf(v)))
    return out


@pytest.mark.parametrize("seed", SC.SEEDS, ids=_ids)
def test_gumbel_table_equals_the_oracle(oracle, seed):
    """row j = -logf(-logf(z)), z = the oracle's stateless_normal([S], [seed + j + 1, seed + j + 2])."""
    from irec.engine import build_gumbel_table
    steps = 3
    for S in SIZES:
        tab = build_gumbel_table(seed, S, steps)
        for j in range(steps):
            want = _gumbel_of(oracle.tf_stateless_normal(seed + j + 1, seed + j + 2, S))
            got = tab[j, :S]
            assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)]), (S, j)
            assert not tab[j, S:].any()


# ==== (b) the header ===========================================================================================================================
SHAPE, BLOCK_SIZE, MAX_INDEX = (32, 48, 3), 1000, 20
BPR = (3, 2)                                                             # blocks per residual block


def _rows():
    rng = np.random.default_rng(5)
    K = rng.integers(1, 5, (2, sum(BPR))).astype(np.int32)
    idx = rng.integers(0, MAX_INDEX, (2, sum(BPR), 4)).astype(np.int32)
    return K, np.where(np.arange(4)[None, None, :] < K[..., None], idx, 0).astype(np.int32)


def _lists(K, idx, i):
    first = np.concatenate([[0], np.cumsum(BPR)])
    return [[idx[i, b, :K[i, b]].tolist() for b in range(first[r], first[r + 1])] for r in range(len(BPR))]


def _index_tables():
    from irec.io import SymbolTables
    return SymbolTables(np.ones(MAX_INDEX + 1, dtype=np.int64), None)


def _blob_writers():
    """name -> (write(seed) -> (blob, offsets), read(blob, offsets) -> the header seeds of the files): every host writer of N files."""
    from irec import io as IO
    K, idx = _rows()
    K3, idx4 = K[:, :4].reshape(2, 2, 2).copy(), idx[:, :4].reshape(2, 2, 2, 4).copy()
    tables = _index_tables()
    return {
        "encode_files": (lambda s: IO.encode_files(s, SHAPE, BLOCK_SIZE, K3, idx4, MAX_INDEX),
                         lambda b, o: IO.decode_files(b, o, 2, 2, 4)[0][:, 0]),
        "encode_files_ragged": (lambda s: IO.encode_files_ragged(s, SHAPE, BLOCK_SIZE, K, idx, MAX_INDEX, BPR),
                                lambda b, o: IO.decode_files_ragged(b, o, BPR, 4)[0][:, 0]),
        "encode_files_tables": (lambda s: IO.encode_files(s, SHAPE, BLOCK_SIZE, K3, idx4, MAX_INDEX, tables=tables),
                                lambda b, o: IO.decode_files(b, o, 2, 2, 4, tables=tables)[0][:, 0]),
        "encode_files_ragged_tables": (lambda s: IO.encode_files_ragged(s, SHAPE, BLOCK_SIZE, K, idx, MAX_INDEX, BPR, tables=tables),
                                       lambda b, o: IO.decode_files_ragged(b, o, BPR, 4, tables=tables)[0][:, 0]),
        "encode_files_segmented": (lambda s: IO.encode_files_segmented(s, SHAPE, BLOCK_SIZE, K, idx, MAX_INDEX, BPR, 2),
                                   lambda b, o: IO.decode_files_segmented(b, o, BPR, 4)[0][:, 0]),
    }


_WRITERS = ("encode_files", "encode_files_ragged", "encode_files_tables", "encode_files_ragged_tables", "encode_files_segmented")


def test_header_seed_helper():
    from irec.io import header_seed
    for seed in (0, 5, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, np.int64(7), np.uint32(2 ** 32 - 1)):
        assert header_seed(seed, "t") == int(seed) and type(header_seed(seed, "t")) is int
    for seed in SC.HEADER_BAD + (SC.SEED_BOUND, -2 ** 63, 2 ** 40 + 5):
        with pytest.raises(ValueError, match=r"who: seed %d .*\[0, 2\^32\)" % seed):
            header_seed(seed, "who")
    for seed in (1.5, "5", None, float("inf")):
        with pytest.raises(ValueError, match="who: seed must be an integer"):
            header_seed(seed, "who")
    assert header_seed(7.0, "t") == 7 and header_seed(np.array(7), "t") == 7        # (what int() takes without changing its value)
    with pytest.raises(ValueError, match=r"seed 4294967296 .*\[0, 2\^32\)"):
        header_seed(2.0 ** 32, "who")


def test_rec_header_pack():
    from irec.io.utils import RecHeader
    import io
    make = lambda seed: RecHeader(seed, 1000, 20, (4, 5, 3), False, False, [2], [3], [4], [1])    # noqa: E731
    for seed in (0,) + SC.HEADER_GOOD:
        assert RecHeader.read(io.BytesIO(make(seed).pack())).seed == seed
    for seed in SC.HEADER_BAD:
        with pytest.raises(ValueError, match=r"seed %d .*\[0, 2\^32\)" % seed):
            make(seed).pack()


@pytest.mark.parametrize("path", ["native", "per_stream"])
def test_write_compressed_code_round_trips_the_last_header_seed_and_refuses_the_rest(tmp_path, path):
    from irec import io as IO
    K, idx = _rows()
    lists = _lists(K, idx, 0)
    fi = None
    if path == "per_stream":                       # an index-count file takes the reference-shaped writer, one coder call per stream
        fi = str(tmp_path / "index_counts.npy")
        _index_tables().save(fi, None)
    for seed in SC.HEADER_GOOD:
        f = str(tmp_path / f"good_{seed}.rec")
        IO.write_compressed_code(f, seed, SHAPE, BLOCK_SIZE, lists, MAX_INDEX, index_counts_file=fi)
        got = IO.read_compressed_code(f, index_counts_file=fi)
        assert got[0] == seed and tuple(got[1]) == SHAPE and got[2] == BLOCK_SIZE and [list(map(list, rb)) for rb in got[3]] == lists
        assert IO.rec_header_words(open(f, "rb").read())["seed"] == seed
    before = sorted(os.listdir(tmp_path))
    for seed in SC.HEADER_BAD:
        f = str(tmp_path / f"bad_{SC.seed_id(seed)}.rec")
        with pytest.raises(ValueError, match=r"write_compressed_code: seed %d .*\[0, 2\^32\)" % seed):
            IO.write_compressed_code(f, seed, SHAPE, BLOCK_SIZE, lists, MAX_INDEX, index_counts_file=fi)
        assert not os.path.exists(f)
    assert sorted(os.listdir(tmp_path)) == before


@pytest.mark.parametrize("writer", _WRITERS)
def test_batched_writers_round_trip_the_last_header_seed(writer):
    write, read = _blob_writers()[writer]
    ref_blob, ref_off = write(5)
    for seed in SC.HEADER_GOOD:
        blob, off = write(seed)
        assert np.array_equal(off, ref_off)                       # (the seed is four header bytes: nothing else of a file moves)
        assert read(blob, off).tolist() == [seed, seed]
        diff = np.flatnonzero(np.asarray(blob) != np.asarray(ref_blob))
        starts = np.asarray(off[:-1])
        seed_at = 8 if writer == "encode_files_segmented" else 0           # (the segmented file: magic, version, reserved, then the seed)
        assert all(((d - starts >= seed_at) & (d - starts < seed_at + 4)).any() for d in diff), writer


@pytest.mark.parametrize("seed", SC.HEADER_BAD, ids=_bad_ids)
@pytest.mark.parametrize("writer", _WRITERS)
def test_batched_writers_refuse_a_seed_no_header_holds(writer, seed):
    write, _ = _blob_writers()[writer]
    with pytest.raises(ValueError, match=r"seed %d .*\[0, 2\^32\)" % seed):
        write(seed)


# ==== (c) the C ABI above the bound ============================================================================================================
ABOVE = (SC.SEED_BOUND + 1, SC.INT64_MAX)


def _c_calls():
    """name -> (call(seed) -> (status, outputs that must stay as they were)): the host entry points that take a coding seed, and -- with a
    null context, which they look at only after the seed -- the device ones."""
    from irec import _lib
    lib = _lib.load()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)       # noqa: E731
    p = _lib.IrecParams(3.0, 20, 10, 0, (ctypes.c_int32 * 4)(64, 0, 0, 0), 4)

    def normal(seed):
        out = np.full(2 * 3 * 16, 7.0, dtype=np.float32)
        return lib.irec_normal_table_build(seed, 5, 3, 2, vp(out), 1), out

    def gumbel(seed):
        out = np.full(2 * 16, 7.0, dtype=np.float32)
        return lib.irec_gumbel_table_build(seed, 5, 2, vp(out), 1), out

    def encode(seed):
        out = np.full(8, 7, dtype=np.int32)
        return lib.irec_beam_encode(None, ctypes.byref(p), 1, None, None, None, 64, None, None, None, None, None, seed, 8, vp(out), vp(out),
                                    vp(out), None, 0, None), out

    def encode_ex(seed):
        out = np.full(8, 7, dtype=np.int32)
        return lib.irec_beam_encode_ex(None, ctypes.byref(p), 1, None, None, None, 64, None, None, None, None, None, seed, 8, vp(out), vp(out),
                                       vp(out), None, None, 0, None), out

    def decode(seed):
        out = np.full(8, 7, dtype=np.int32)
        return lib.irec_beam_decode(None, ctypes.byref(p), 1, None, None, None, None, None, None, seed, 8, None, None, vp(out), None), out

    def decode_ws(seed):
        out = np.full(8, 7, dtype=np.int32)
        return lib.irec_beam_decode_ws(None, ctypes.byref(p), 1, None, None, None, 64, None, None, None, seed, 8, None, None, vp(out), None, 0,
                                       None), out

    def decode_tensors(seed):
        out = np.full(8, 7, dtype=np.int32)
        return lib.irec_beam_decode_tensors(None, ctypes.byref(p), 1, 64, 64, None, None, None, None, seed, 8, None, None, vp(out), None, 0,
                                            None), out

    def proposal_table(seed):
        out = np.full(8, 7, dtype=np.int32)
        return lib.irec_test_proposal_table(None, seed, 20, 64, 2, vp(out), None), out
    return {"irec_normal_table_build": normal, "irec_gumbel_table_build": gumbel, "irec_beam_encode": encode, "irec_beam_encode_ex": encode_ex,
            "irec_beam_decode": decode, "irec_beam_decode_ws": decode_ws, "irec_beam_decode_tensors": decode_tensors,
            "irec_test_proposal_table": proposal_table}


_C_NAMES = ("irec_normal_table_build", "irec_gumbel_table_build", "irec_beam_encode", "irec_beam_encode_ex", "irec_beam_decode",
            "irec_beam_decode_ws", "irec_beam_decode_tensors", "irec_test_proposal_table")


@pytest.mark.parametrize("name", _C_NAMES)
def test_c_entry_points_refuse_a_seed_above_the_bound(name):
    from irec import _lib
    lib = _lib.load()
    call = _c_calls()[name]
    for seed in ABOVE:
        st, out = call(seed)
        text = lib.irec_last_error().decode()
        assert st == _lib.IREC_E_INVALID and str(seed) in text and "IREC_SEED_MAX" in text and str(SC.SEED_BOUND) in text, (name, seed, st, text)
        assert (out == 7).all(), name                          # nothing written
    # the bound itself (and a seed below every int64 a caller is likely to hold) passes the seed check: the table builders succeed, the
    # device entry points go on to refuse their null context
    for seed in (SC.SEED_BOUND, -2 ** 63):
        st, out = call(seed)
        text = lib.irec_last_error().decode()
        if name.endswith("_table_build"):
            assert st == _lib.IREC_OK and not (out == 7).any(), (name, seed, text)
        else:
            assert st == _lib.IREC_E_INVALID and "IREC_SEED_MAX" not in text and ("null context" in text or "bad arguments" in text), (name, text)


def test_the_host_sampler_takes_step_seeds_up_to_int64_max_less_two():
    """irec_importance_encode / _decode and irec_tf_stateless_gumbel take the seed of ONE step (their caller forms coding seed + t) and add
    at most 2 to it."""
    from irec import _lib
    lib = _lib.load()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)       # noqa: E731
    loc, scale = np.zeros(4, np.float32), np.ones(4, np.float32)
    for seed, ok in ((SC.INT64_MAX - 2, True), (SC.INT64_MAX - 1, False), (SC.INT64_MAX, False)):
        index, out = ctypes.c_int64(-7), np.full(4, 7.0, np.float32)
        st = lib.irec_importance_encode(vp(loc), vp(scale), vp(loc), vp(scale), 4, 3.0, 2.0, seed, ctypes.byref(index), vp(out))
        assert (st == 0) == ok and (ok or (index.value == -7 and (out == 7).all() and str(seed).encode() in lib.irec_last_error()))
        out = np.full(4, 7.0, np.float32)
        st = lib.irec_importance_decode(vp(loc), vp(scale), 4, 0, seed, vp(out))
        assert (st == 0) == ok and (ok or (out == 7).all())
        out = np.full(4, 7.0, np.float32)
        st = lib.irec_tf_stateless_gumbel(seed, 4, vp(out))
        assert (st == 0) == ok and (ok or (out == 7).all())


# ==== (d) Python refuses what int64 cannot hold ===================================================================================================
def test_python_refuses_a_seed_that_does_not_fit_int64():
    import irec
    from irec import _lib, engine
    from irec.coding.utils import stateless_gumbel_sample
    assert ctypes.c_int64(2 ** 63).value == -2 ** 63            # what ctypes alone makes of it
    N = torch.distributions.Normal
    q = N(torch.zeros(1, 8) + 0.5, torch.ones(1, 8) * 0.5, validate_args=False)
    p = N(torch.zeros(1, 8), torch.ones(1, 8), validate_args=False)
    coder = irec.GaussianCoder(kl_per_partition=3.0, sampler=irec.ImportanceSampler(coding_bits=3.0))
    sampler = irec.ImportanceSampler(coding_bits=3.0)
    calls = {
        "tf_shuffle_perm": lambda s: engine.tf_shuffle_perm(s, 4),
        "philox_uniform_int": lambda s: engine.philox_uniform_int(s, 4),
        "build_normal_table": lambda s: engine.build_normal_table(s, 4, 2, 2),
        "build_gumbel_table": lambda s: engine.build_gumbel_table(s, 4, 2),
        "stateless_gumbel_sample": lambda s: stateless_gumbel_sample((4,), s),
        "coded_sample": lambda s: sampler.coded_sample(q, p, s),
        "decode_sample": lambda s: sampler.decode_sample(p, 0, s),
        "GaussianCoder.encode_block": lambda s: coder.encode_block(q, p, s),
        "GaussianCoder.decode_block": lambda s: coder.decode_block(p, [0], s),
        "GaussianCoder.encode": lambda s: coder.encode(q, p, s),
        "GaussianCoder.decode": lambda s: coder.decode(p, [0], s),
    }
    for name, call in calls.items():
        for seed in (2 ** 63, -2 ** 63 - 1, 2 ** 64 + 5):
            with pytest.raises(ValueError, match="seed %d is out of range" % seed):
                call(seed)
        call(5)                                                  # (the call itself is a valid one)
    # the raw binding: ctypes reports the same refusal as an ArgumentError instead of wrapping
    out = np.zeros(4, np.int64)
    with pytest.raises(ctypes.ArgumentError, match="out of range"):
        _lib.load().irec_tf_shuffle_perm(2 ** 63, 4, out.ctypes.data_as(ctypes.c_void_p))
    # a coding seed above the bound on the host path of the sequential coder, which forms seed + t itself
    for call in (calls["GaussianCoder.encode_block"], calls["GaussianCoder.decode_block"]):
        with pytest.raises(ValueError, match="IREC_SEED_MAX"):
            call(SC.SEED_BOUND + 1)
        call(SC.SEED_BOUND)
    for name in ("build_normal_table", "build_gumbel_table"):
        with pytest.raises(_lib.IrecLibraryError, match="IREC_SEED_MAX"):
            calls[name](SC.SEED_BOUND + 1)
