"""Every decoder build on index rows no encoder would write (tests/decode_cases.py): each decode mode of engine.decode_blocks against the
oracle's decode_block (rec/coding/beam_search_coder.py:124-148), np.array_equal on the float32 samples -- the decoder compares no scores,
so its contract has no tolerance -- and p.loc on every block whose row is outside the domain.  Which __global__ build a call takes is
restated by decode_cases.dispatch; tests/test_decode_corners_host.py proves that every build and every corner is reached."""
import ctypes

import numpy as np
import pytest
import torch

import decode_cases as dc

pytestmark = pytest.mark.gpu


def _n_cu(engine):
    return engine.plan(engine.params(3.0, 36, 20), engine.layout(1, 192, 192, 42), 8)["n_cu"]


def _upload(eng, case, block_row=None):
    """(layout, p_loc, p_scale, K, indices) on the device: rows in layout order, or (block_row given) where block_row says."""
    lay = eng.layout(case.lay.n_tensors, case.lay.n, case.lay.bs, dc.SEED)
    assert lay.n_blocks == case.lay.n_blocks and lay.blocks_per_tensor == case.lay.bpt
    mp, sp, _ = dc.expected(case)
    at = lay.natural if block_row is None else block_row
    K, idx = np.empty_like(case.K), np.empty_like(case.idx)
    K[at], idx[at] = case.K, case.idx
    dev = lambda a: torch.from_numpy(np.array(a)).to(eng.device)               # (a copy: the cached arrays are read-only)
    return lay, dev(mp), dev(sp), dev(K), dev(idx)


def _blocks_off(case, got, want):
    """The natural blocks whose elements differ, as (block, K, dims): what a failure is reported with."""
    perm, lay, out = dc.perm_of(case.lay.n), case.lay, []
    for i in range(lay.n_tensors):
        for j, d in enumerate(lay.block_dims):
            g = perm[j * lay.bs:j * lay.bs + d]
            if not np.array_equal(got[i, g], want[i, g]):
                out.append((i * lay.bpt + j, int(case.K[i * lay.bpt + j]), d))
    return out[:12]


def _check(eng, case, n_cu, block_row=None, keep=None):
    """Every call of case.routes() against the oracle's samples; returns how many calls ran.  keep: dict that receives the samples' bytes."""
    want = dc.expected(case)[2]
    lay, pl, ps, K, idx = _upload(eng, case, block_row)
    rows = None if block_row is None else torch.from_numpy(block_row.astype(np.int32)).to(eng.device)
    bad, calls = [], 0
    for mode, ts, build, kt in case.routes(n_cu):
        if rows is not None and mode not in ("tensors", "tensors_fused"):
            continue
        params = eng.params(3.0, case.S, 20, 0, (), ts)
        rec = eng.decode_blocks(params, lay, pl, ps, dc.SEED, K, idx, mode=mode, block_row=rows)
        got = rec.cpu().numpy()
        calls += 1
        if keep is not None:
            keep[(mode, ts)] = got.tobytes()
        if not np.array_equal(got, want):
            bad.append((mode, ts, build, kt, _blocks_off(case, got, want)))
    assert not bad, (case, bad)
    assert calls > 0
    return calls


LADDER = [(n, bs, f) for n, bs in dc.LADDER_LAYOUTS for f in dc.ladder_families(n, bs)]


@pytest.mark.parametrize("n,bs,family", LADDER)
def test_ladder(engine, oracle, n, bs, family):
    """K on 0 .. 5, 31 .. 33, 63 .. 67, 127 .. 129 and 193 in every mode at table windows of 32, 64 and 128 steps."""
    case = dc.ladder_case(n, bs, family)
    calls = _check(engine, case, _n_cu(engine))
    assert calls == len(dc.MODES) * len(dc.TABLE_STEPS)        # every ladder layout fits the staged kernel: no mode is left out


@pytest.mark.parametrize("n,bs", sorted(dc.STAGED_LAYOUTS))
def test_staged_kernel(engine, oracle, n, bs):
    """36 / 37 / 38 / 60 unit slots and one wave, float4 and scalar staging, rows in layout order and through a permuted block_row."""
    case = dc.staged_case(n, bs)
    n_cu = _n_cu(engine)
    assert _check(engine, case, n_cu) == 4
    block_row = np.random.default_rng(n).permutation(case.lay.n_blocks)
    assert _check(engine, case, n_cu, block_row=block_row) == 4


def test_staged_limit_is_refused(engine):
    n, bs = dc.STAGED_UNSUPPORTED
    lay = engine.layout(1, n, bs, dc.SEED)
    z = torch.zeros(n, dtype=torch.float32, device=engine.device)
    K, idx = torch.zeros(lay.n_blocks, dtype=torch.int32, device=engine.device), torch.zeros((lay.n_blocks, 4), dtype=torch.int32, device=engine.device)
    with pytest.raises(ValueError):
        engine.decode_blocks(engine.params(3.0, 20, 20), lay, z, z + 1, dc.SEED, K, idx, mode="tensors")
    assert torch.equal(engine.decode_blocks(engine.params(3.0, 20, 20), lay, z, z + 1, dc.SEED, K, idx, mode="auto"), z)   # K = 0: p.loc


def test_tensor_loop_and_run_to_run(engine, oracle):
    """4 n_cu + 3 tensors of ten 7-dim blocks: workgroups of the staged kernel refill their LDS region two and three times, their waves
    leaving a tensor at different times (K from the ladder).  Twice: the same bytes."""
    n_cu = _n_cu(engine)
    case = dc.loop_case(n_cu)
    first, second = {}, {}
    assert _check(engine, case, n_cu, keep=first) == len(dc.MODES)
    _check(engine, case, n_cu, keep=second)
    assert first.keys() == second.keys() and all(first[k] == second[k] for k in first)


@pytest.mark.parametrize("ragged", (False, True))
def test_large_grid(engine, oracle, ragged):
    """16 blocks per CU and more: the legacy kernel with the quantile table in LDS, next to every other mode."""
    n_cu = _n_cu(engine)
    case = dc.grid_case(n_cu, ragged)
    assert dc.dispatch(n_cu, "legacy", case.lay, case.S, case.max_K)[0] == "decode_kernel<true>"
    assert _check(engine, case, n_cu) == len(dc.MODES)


def test_hash_sum_wraps(engine, oracle):
    """S = 2^24, six steps of index S - 1: the int32 sum is negative before steps 2 and 3 and past 2^32 before steps 4 and 5.  A decoder
    that took the modulo of the uint32 value, or summed in 64 bits, draws other quantiles (decode_cases.WRAP_HASHES)."""
    case = dc.wrap_case()
    assert _check(engine, case, _n_cu(engine)) == len(dc.MODES)


@pytest.mark.parametrize("n,bs", dc.BAD_LAYOUTS)
def test_bad_rows(engine, oracle, n, bs):
    """An index that is no sample index at steps 0, 63, 64 and 128 (S), 70 (-1) and 3 (0x7FFFFFFF) of rows of K = 129, K = -1 and
    K = max_K + 1: p.loc on exactly those eight blocks, the oracle's sample on every other."""
    case = dc.bad_case(n, bs)
    mp, _, want = dc.expected(case)
    perm, lay = dc.perm_of(n), case.lay
    for b in case.bad:
        i, j = divmod(b, lay.bpt)
        g = perm[j * lay.bs:j * lay.bs + lay.block_dims[j]]
        assert np.array_equal(want[i, g], mp[i, g])
    assert len(case.bad) == 8 and not np.array_equal(want, mp)
    assert _check(engine, case, _n_cu(engine)) == 2 * len(case.modes)


def test_fitted_ratio_table(engine, oracle):
    """A context created with a ratio table of 8 entries (irec_create_with, as BeamSearchCoder.set_auxiliary_variance_ratios does):
    K = 8 decodes as the oracle does under the same table, K = 9 comes out as p.loc -- in the kernels, not only in the Python coder."""
    from irec.engine import Engine
    case = dc.fitted_case()
    eng = Engine(engine.device, aux_ratios=case.aux)
    assert eng.max_partitions == len(dc.AUX_RATIOS) == 8
    mp, _, want = dc.expected(case)                            # (sets the oracle's table and resets it in a finally)
    assert oracle.aux_ratio(1) != np.float32(dc.AUX_RATIOS[1])
    assert {int(k) for k in case.K} >= {8, 9} and len(case.bad) >= 10
    assert _check(eng, case, _n_cu(engine)) == len(dc.MODES)
    power_law = dc.Case("fitted-power-law", case.lay, case.S, max_K=case.max_K, Ks=[int(k) for k in case.K], seed=case.seed, table_steps=(0,))
    assert not np.array_equal(dc.expected(power_law)[2], want)  # (the table matters)


def test_restated_workspace_bytes_match_the_library(engine):
    """decode_cases.workspace_bytes against irec_decode_workspace_bytes (it takes a context): the table window's clamps."""
    lib = engine.lib
    grid = [((256, 5), 36), ((1, ), 36), ((4, 3), 36), ((1025, ), 20), ((1024, 1023), 20), ((1000, 192), 8103), ((1000, 192, 7, 1), 8103),
            ((1024, ), 1 << 24), ((7, ), 1 << 24), ((1, ), 1 << 24), ((), 36)]
    n = 0
    for dims, S in grid:
        for max_K in (0, 1, 7, 8, 9, 32, 33, 200, 4096, 65536):
            for ts in (0, 1, 8, 64, 128, 4096, 5000):
                p = engine.params(3.0, S, 20, 0, dims, ts)
                assert lib.irec_decode_workspace_bytes(engine.ctx, ctypes.byref(p), max_K) == dc.workspace_bytes(dims, S, max_K, ts), (dims, S, max_K, ts)
                n += 1
    assert n == len(grid) * 70
