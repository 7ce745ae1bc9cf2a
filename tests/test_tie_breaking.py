"""Every encoder's tie-breaking and non-finite ordering against the oracle.

The coders' outputs are decided by comparisons: the top-B of S * B scores at each beam step, the arg-max of S weights at each
importance step.  The contract (oracle/irec_oracle.c: cand_before; tests/gc_referee.py: importance_step) says what happens when the
comparison does not decide: value descending, exact ties to the lower flat index s * B_cur + b, a NaN after every number; greatest
weight, first s on ties, a NaN never chosen.  test_top_b_selection pins that on the shared selection routine only; the other
encoders carry their own selection code and meet an exact tie 98 times in 589 824 blocks of ordinary inputs.  Here ties are the
common case, through the two inputs that produce the candidates and are the caller's data already: the quantile table
(irec.Engine(lut=...) / oracle.set_lut) and the normal proposal table (irec.engine.build_normal_table).  tests/tie_tables.py builds
the tables.

  1 (both suites)  the tables are fit for purpose -- conditions the ORACLE alone must meet: for every kernel name, under the table
                   pick_lambda chooses, a tie that decides what is emitted in at least 25 % of the (block, step) pairs that reject a
                   candidate (before the last step score[rank B - 1] == score[rank B]; at the last step, whose beam 0 alone is
                   emitted, score[rank 0] == score[rank 1]), at least one such tie for every name, at most 6 names under 25 %, a
                   non-zero index in every case -- and the proof of power itself: the oracle switched to the WRONG rule (exact ties
                   to the higher flat index; for the poisoned tables, a NaN before every number: oracle.set_wrong_order) emits other
                   indices or samples for every name's call.  A kernel with that rule fails the GPU test of that name.
  2 (GPU)          every planned kernel under its spiky table equals the oracle: K, indices, samples, margins, decode.
  3 (GPU)          one call per encoder family under a constant table (every candidate of every step ties) and under a poisoned one
                   (scores of +inf, -inf and NaN).
  4 (GPU)          the importance coder over normal tables whose columns repeat, and with NaN / -inf weights.

The calls.  tests/test_kernel_coverage.py codes, for every kernel name, the cheapest call of the planner grid that launches it; for
33 of the 68 names that call has ONE sample, whose selection has nothing to reject, and nearly all are one block of 192 dims with
two partitions, whose only rejecting step is the last.  The calls here are the cheapest ones of 1000 or 2048 dims (7 to 35
partitions) that reject a candidate by their second step (kernel_names.rejects_by_step_two): same grid, same inputs.

Names under 25 % at the rung chosen for them: none (measured 25 % to 88 %).  The calls of few beams and 54 to 1339 samples do not
reach 25 % on the ladder (0.5, 0.1, 0.02) with spikes of +-0.5 .. +-2: a table has at least one spike, S * D / 10006 samples of a
step meet it, and one of them wins.  The ladder goes on to spikes of +-32 .. +-1024 for them (tie_tables.LADDER).

The poisoned table.  +-2**64 does not take a score out of the float32 range (the term is (G + H z) z with |H| well below 1, and
H * 2**128 stays finite), so the poison is +-2**96; and the posteriors of synthetic_latent are narrower than their priors in every
dim (H < 0: no score can reach +inf under any table), so the poisoned calls widen every eighth dim's posterior
(tie_tables.case_inputs(widen=True)).  The oracle-side condition -- a NaN, a +inf and a -inf score, the NaN in a step whose
selected set would be another if NaN ranked first -- is asserted for every family."""
import functools
import os
import re

import numpy as np
import pytest

import gc_referee as R
import kernel_names as kn
import tie_tables as T
from conftest import GOLDEN_DIR

SEED = 42
OMEGA = 3.0
MAX_UNDER = 6


@functools.lru_cache(maxsize=None)
def _plans(n_cu=256):
    return kn.enumerate_plans(n_cu, dims=kn.DIMS[1:], accept=kn.rejects_by_step_two)


def _names():
    try:
        return sorted(_plans())
    except Exception:        # (the library is missing: test_tables_are_fit_for_purpose says so)
        return []


@functools.lru_cache(maxsize=None)
def _pick(name, n_cu=256):
    """(rung, stats, table) of a kernel name's call."""
    from oracle import oracle as O
    case = _plans(n_cu)[name]
    rung, st = T.pick_lambda(O, case)
    return rung, st, T.spiky_lut(case["dim"], rung[0], 0, rung[1])


FAMILIES = {"ten": r"encode_ten_kernel<", "team": r"encode_team_kernel<\d+,3,1,false,false,false,false>$", "lone": r"encode_lone_kernel$",
            "fast": r"encode_fast_kernel<", "chunk": r"encode_chunk_kernel<.*,false>$", "chunk-gang": r"encode_chunk_kernel<.*,true>$",
            "generic": r"encode_generic_kernel$"}


@functools.lru_cache(maxsize=None)
def _poison(family, n_cu=256):
    """((lambda, seed), stats) of the poisoned table of a family's call."""
    from oracle import oracle as O
    return T.pick_poison(O, _family_case(family, n_cu)[1])


def _family_case(family, n_cu=256):
    """(name, call): the cheapest call of the grid that launches a kernel of the family."""
    plans = _plans(n_cu)
    names = [n for n in plans if re.match(FAMILIES[family], n)]
    assert names, family
    name = min(names, key=lambda n: (plans[n]["cost"], n))
    return name, plans[name]


# 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.both_suites
@pytest.mark.usefixtures("suite")
def test_helpers_build_the_tables_they_say(oracle):
    for dim, lam in ((192, 0.5), (1000, 0.1), (2048, 0.02)):
        lut = T.spiky_lut(dim, lam)
        assert lut.dtype == np.float32 and lut.shape == (10007,) and lut[0] == 0 and np.isfinite(lut).all()
        assert np.array_equal(lut, T.spiky_lut(dim, lam)) and not np.array_equal(lut, T.spiky_lut(dim, lam, seed=1))
        spikes = np.flatnonzero(lut[1:] != T.BASE) + 1
        assert len(spikes) == max(1, round(10006 * lam / dim)) and set(np.abs(lut[spikes]).tolist()) <= {0.5, 1.0, 2.0}
        bad = T.poisoned_lut(dim, lam)
        moved = np.flatnonzero(bad != lut)
        assert np.isfinite(bad).all() and np.isin(moved, spikes).all() and len(moved) == (len(spikes) + 1) // 2
        assert (np.abs(bad[moved]) == T.POISON).all()
    # the table is restored whatever happens inside
    before = oracle.encode_block(*oracle.synthetic_latent(11, 192), SEED, OMEGA, 20, 10)
    with pytest.raises(ZeroDivisionError):
        with T.oracle_table(oracle, T.constant_lut()):
            assert oracle.encode_block(*oracle.synthetic_latent(11, 192), SEED, OMEGA, 20, 10)[0] != before[0]
            1 / 0
    after = oracle.encode_block(*oracle.synthetic_latent(11, 192), SEED, OMEGA, 20, 10)
    assert before[0] == after[0] and np.array_equal(before[1], after[1])
    # rank() is cand_before
    sc = np.array([1.0, np.nan, -np.inf, 1.0, np.inf, -0.0, 0.0, np.nan, -np.inf], dtype=np.float32)
    assert T.rank(sc).tolist() == [4, 0, 3, 5, 6, 2, 8, 1, 7]


@pytest.mark.both_suites
@pytest.mark.usefixtures("suite")
def test_tables_are_fit_for_purpose(oracle):
    """The oracle alone: under the table chosen for it, every kernel name's call ties where the tie decides what is emitted, and
    the oracle with the WRONG tie rule (exact ties to the higher flat index) emits something else: a kernel with that rule fails
    test_every_planned_kernel_under_its_spiky_table."""
    plans = _plans()
    assert set(plans) == set(kn.enumerate_plans()), "a kernel name without a call of the grid that rejects a candidate"
    under, report = [], []
    for name in sorted(plans):
        (lam, values), st, _ = _pick(name)
        report.append(f"{name:52s} B={plans[name]['B']:3d} S={plans[name]['S']:4d} D={plans[name]['dim']:4d} blocks={plans[name]['n_blocks']:3d}"
                      f"  lambda={lam} spikes=+-{sorted(set(abs(float(v)) for v in values))}  deciding ties {st['cutoff_ties']}/{st['rejecting']}"
                      f"  blocks the wrong rule changes {st['exposed']}  steps with a tie inside the set {st['inner_ties']}")
        assert st["rejecting"] >= 1 and st["cutoff_ties"] >= 1, (name, st)
        assert st["nonzero"], (name, "every index is 0: the row an untouched output buffer would show")
        assert st["exposed"] >= 1, (name, "ties to the higher index emit the same indices and samples: the call has no power", st)
        if st["share"] < T.MIN_SHARE:
            under.append((name, st["share"]))
    print("\n".join(report))                       # (pytest -s shows the table: the rung and the share of every name)
    assert len(under) <= MAX_UNDER, under
    assert not under, f"names under {T.MIN_SHARE:.0%} that the module docstring does not list: {under}"


@pytest.mark.both_suites
@pytest.mark.usefixtures("suite")
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_storm_tables_are_fit_for_purpose(oracle, family):
    name, case = _family_case(family)
    host = T.case_inputs(oracle, case)
    with T.oracle_table(oracle, T.constant_lut()):
        ridx, rs, _ = oracle.encode_tensors_omp(*host, SEED, OMEGA, case["S"], case["B"], case["dim"], max_K=case["max_K"])
        for i in range(min(case["n_blocks"], 4)):
            tr = oracle.encode_block(*(h[i] for h in host), SEED, OMEGA, case["S"], case["B"], max_K=case["max_K"], trace=True)[2]
            for t, N, Bnew, sc in T.steps_of(tr, case["S"], case["B"]):
                assert N >= 2 and (sc == sc[0]).all(), (name, i, t)          # every candidate of every step ties
    assert all(v == 0 for blk in ridx for v in blk[0]) and max(len(blk[0]) for blk in ridx) >= 2
    assert not np.array_equal(rs, host[2])
    assert T.exposes(oracle, T.constant_lut(), case, ties_to_higher=True) == case["n_blocks"]
    (lam, seed), st = _poison(family)
    assert st["nan"] >= 1 and st["pinf"] >= 1 and st["ninf"] >= 1, (name, lam, seed, st)
    assert st["nan_decides"] >= 1, (name, "no NaN in a step where it would change what is emitted if NaN ranked first", st)
    assert st["exposed"] >= 1, (name, "a NaN ranked before every number emits the same indices and samples", st)


# 2 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engines(engine):
    """Private engines, one per distinct quantile table; released when the module is done."""
    import torch
    import irec
    cache = {}

    def get(lut):
        key = lut.tobytes()
        if key not in cache:
            cache[key] = irec.Engine(engine.device, lut=lut)
        return cache[key]
    yield get
    torch.cuda.synchronize()
    cache.clear()


def _run(eng, case, host, name):
    """One call of `case` on `eng`, encoded and decoded: -> (K, indices, sample [n_blocks, dim], margins or None, decoded sample
    [n_blocks, dim], layout).  name: the kernel the plan must name, None for whichever the planner gives the shape."""
    import torch
    from irec import _lib
    B, S, n_blocks, dim, max_K, flags = case["B"], case["S"], case["n_blocks"], case["dim"], case["max_K"], case["flags"]
    margins = bool(flags & _lib.IREC_FLAG_MARGINS)
    ql, qs, pl, ps = (torch.from_numpy(a).cuda().contiguous() for a in host)
    lay = eng.layout(n_blocks, dim, dim, SEED)
    assert lay.n_blocks == n_blocks and lay.max_dim == dim
    params = eng.params(OMEGA, S, B, flags & ~_lib.IREC_FLAG_MARGINS)
    plan = eng.plan(params, lay, max_K, margins=margins)
    assert name is None or kn.canonical(plan["kernel"], plan["split"]) == name, (plan, case)
    mg = None
    if margins:
        K, idx, sample, mg = eng.encode_blocks_margins(params, lay, ql, qs, pl, ps, SEED, max_K)
    else:
        K, idx, sample = eng.encode_blocks(params, lay, ql, qs, pl, ps, SEED, max_K)
    dec = eng.decode_blocks(params, lay, pl, ps, SEED, K, idx, mode="auto")
    torch.cuda.synchronize()
    Kh, ih, sh = K.cpu().numpy(), idx.cpu().numpy(), sample.cpu().numpy().reshape(n_blocks, dim)
    assert Kh.min() >= 0 and Kh.max() <= max_K, (name, int(Kh.min()), int(Kh.max()))
    return Kh, ih, sh, None if mg is None else mg.cpu().numpy(), dec.cpu().numpy().reshape(n_blocks, dim), lay


def _n_cu(engine):
    return engine.plan(engine.params(3.0, 36, 20), engine.layout(1, 192, 192, 42), 8)["n_cu"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names())
def test_every_planned_kernel_under_its_spiky_table(engine, engines, oracle, name):
    n_cu = _n_cu(engine)
    case = _plans(n_cu)[name]
    rung, st, lut = _pick(name, n_cu)
    host = T.case_inputs(oracle, case)
    Kh, ih, sh, mh, dec, lay = _run(engines(lut), case, host, name)
    with T.oracle_table(oracle, lut):
        ridx, rs, _, rm = oracle.encode_tensors_omp(*host, SEED, OMEGA, case["S"], case["B"], case["dim"], max_K=case["max_K"], margins=True)
    for i in range(case["n_blocks"]):
        row = lay.natural[i]
        assert Kh[row] == len(ridx[i][0]) and ih[row, :Kh[row]].tolist() == ridx[i][0], (name, i)
    assert np.array_equal(sh, rs), name
    assert np.array_equal(dec, sh), name
    if mh is not None:
        for i in range(case["n_blocks"]):
            assert np.array_equal(mh[lay.natural[i]], rm[i, 0]), (name, i, mh[lay.natural[i]], rm[i, 0])
        for i, tied in enumerate(st["tied_blocks"]):      # a cut-off tie before the last step: the smallest gap is no gap
            if tied:
                assert mh[lay.natural[i], 0] == 0.0 and not np.signbit(mh[lay.natural[i], 0]), (name, i)


# The grid's cheapest calls are small (two beams for the ten-beam encoder, 192 dims for the team encoder): the shapes of the
# benchmark and of the README's configurations once more, whatever kernel the planner gives them.
HEADLINE = {"B20_S36": dict(B=20, S=36, dim=1000, n_blocks=16, max_K=32, flags=0),
            "B10_S20": dict(B=10, S=20, dim=1000, n_blocks=12, max_K=32, flags=0),
            "B30_S148": dict(B=30, S=148, dim=1000, n_blocks=3, max_K=32, flags=0)}


@functools.lru_cache(maxsize=None)
def _pick_headline(key):
    from oracle import oracle as O
    rung, st = T.pick_lambda(O, HEADLINE[key])
    return rung, st, T.spiky_lut(HEADLINE[key]["dim"], rung[0], 0, rung[1])


@pytest.mark.both_suites
@pytest.mark.usefixtures("suite")
@pytest.mark.parametrize("key", sorted(HEADLINE))
def test_headline_tables_are_fit_for_purpose(oracle, key):
    rung, st, _ = _pick_headline(key)
    assert st["rejecting"] >= 8 and st["share"] >= T.MIN_SHARE and st["nonzero"] and st["inner_ties"] >= 1, (key, rung, st)


@pytest.mark.gpu
@pytest.mark.parametrize("key", sorted(HEADLINE))
def test_headline_calls_under_spiky_tables(engine, engines, oracle, key):
    case = HEADLINE[key]
    rung, st, lut = _pick_headline(key)
    host = T.case_inputs(oracle, case)
    Kh, ih, sh, mh, dec, lay = _run(engines(lut), case, host, None)
    with T.oracle_table(oracle, lut):
        ridx, rs, _ = oracle.encode_tensors_omp(*host, SEED, OMEGA, case["S"], case["B"], case["dim"], max_K=case["max_K"])
    for i in range(case["n_blocks"]):
        row = lay.natural[i]
        assert Kh[row] == len(ridx[i][0]) and ih[row, :Kh[row]].tolist() == ridx[i][0], (key, i)
    assert np.array_equal(sh, rs) and np.array_equal(dec, sh), key


# 3 ---------------------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    """tests/test_gc_importance_gpu.py's: NaN positions equal, everything else bit-equal."""
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


@pytest.mark.gpu
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_tie_storm(engine, engines, oracle, family):
    """lut[k] = 0.25: every candidate of every step ties, the indices are all 0."""
    name, case = _family_case(family, _n_cu(engine))
    host = T.case_inputs(oracle, case)
    lut = T.constant_lut()
    Kh, ih, sh, mh, dec, lay = _run(engines(lut), case, host, name)
    with T.oracle_table(oracle, lut):
        ridx, rs, _ = oracle.encode_tensors_omp(*host, SEED, OMEGA, case["S"], case["B"], case["dim"], max_K=case["max_K"])
    assert Kh.max() >= 2, "no block selects twice"
    for i in range(case["n_blocks"]):
        row = lay.natural[i]
        assert Kh[row] == len(ridx[i][0]) and not ih[row, :Kh[row]].any(), (name, i, ih[row, :Kh[row]])
    assert np.array_equal(sh, rs) and np.array_equal(dec, sh), name
    assert not np.array_equal(sh, host[2]), "the sample is p_loc: nothing was coded"


@pytest.mark.gpu
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_non_finite_scores(engine, engines, oracle, family):
    """Scores of +inf, -inf and NaN (poisoned_lut): NaN after every number, -inf before NaN, ties among them to the lower index."""
    name, case = _family_case(family, _n_cu(engine))
    (lam, seed), st = _poison(family, _n_cu(engine))
    assert min(st.values()) >= 1, (name, st)
    lut = T.poisoned_lut(case["dim"], lam, seed)
    host = T.case_inputs(oracle, case, widen=True)
    Kh, ih, sh, mh, dec, lay = _run(engines(lut), case, host, name)
    with T.oracle_table(oracle, lut):
        ridx, rs, _ = oracle.encode_tensors_omp(*host, SEED, OMEGA, case["S"], case["B"], case["dim"], max_K=case["max_K"])
    for i in range(case["n_blocks"]):
        row = lay.natural[i]
        assert Kh[row] == len(ridx[i][0]) and ih[row, :Kh[row]].tolist() == ridx[i][0], (name, i, ih[row, :Kh[row]].tolist(), ridx[i][0])
    assert _same(sh, rs) and _same(dec, sh), name


# 4 ---------------------------------------------------------------------------------------------------------------------------------
def _golden_block():
    """tests/golden/block_D192_cfg2: 3.76 nats, K = 4 at one nat a partition."""
    g = np.load(os.path.join(GOLDEN_DIR, "block_D192_cfg2.npz"))
    return [g[k][None] for k in ("q_loc", "q_scale", "p_loc", "p_scale")], 1.0


def _wide_blocks():
    """Two rows of latent_families.mixed at 1025 dims (benign, K = 9; tiny, K = 8)."""
    import latent_families as lf
    rows = lf.mixed(1025, 5, 3.0, max_K=24)
    return list(lf.stack([rows[0], rows[4]])), 3.0


def _gc_call(monkeypatch, engine, oracle, host, omega, S, doctor, seed=17):
    """One gc_encode_blocks / gc_decode_blocks call of a FRESH engine (its table cache must never hold a doctored table for anyone
    else) over normal tables `doctor` rewrote, against the referee over the same tables.
    -> (device indices per block, referee indices per block, referee weights per block and step)."""
    import torch
    import irec
    real, tables = irec.engine.build_normal_table, {}

    def fake(seed_, n_samples, dim, steps, n_threads=0):
        out = real(seed_, n_samples, dim, steps, n_threads)
        assert seed_ == seed and n_samples == S and out.shape[0] == steps and out.shape[1] == dim and not out[:, :, S:].any()
        doctor(out)
        assert not out[:, :, S:].any(), "the padding stays zero"
        tables[dim] = out.copy()
        return out

    monkeypatch.setattr(irec.engine, "build_normal_table", fake)
    eng = irec.Engine(engine.device)
    n, D = host[0].shape
    Ks = [oracle.num_aux(oracle.block_kl(*(h[i] for h in host)), omega) for i in range(n)]
    assert min(Ks) >= 3
    max_K = max(Ks)
    ql, qs, pl, ps = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in host)
    lay = eng.layout(n, D, None, seed)
    K, idx, z = eng.gc_encode_blocks(lay, ql, qs, pl, ps, seed, omega, S, max_K)
    dec = eng.gc_decode_blocks(lay, pl, ps, seed, S, K, idx)
    torch.cuda.synchronize()
    assert D in tables, "the doctored table never reached the engine"
    Kh, ih, zh = K.cpu().numpy(), idx.cpu().numpy(), z.cpu().numpy().reshape(n, D)
    normal = T.referee_normal(tables, seed, S)
    got, want, weights = [], [], []
    for i in range(n):
        w = []
        ridx, rz = R.encode_block(*(h[i] for h in host), seed, S, Ks[i], normal, weights=w)
        row = lay.natural[i]
        assert Kh[row] == Ks[i]
        got.append(ih[row, :Ks[i]].tolist())
        want.append(ridx)
        weights.append(w)
        assert got[-1] == ridx, (i, got[-1], ridx)
        assert _same(zh[i], rz), i
    assert _same(dec.cpu().numpy(), zh), "decode is not encode"
    del eng
    return got, want, weights


# S = 21: one wave.  S = 149, m = 7: ties across waves -- sample 3 (wave 0, lane 3) and sample 66 (wave 1, lane 2) carry column 3, and
# so does every 3 + 7 i up to 143 (wave 2).  S = 1024: the largest workgroup.  S = 1500, m = 1024: a lane owns s and s + 1024, and
# exactly those pairs tie.  D = 1025: the wide kernel, in its tile form (S = 21) and its plain walk (S = 1500).
@pytest.mark.gpu
@pytest.mark.parametrize("wide,S,m", [(False, 21, 7), (False, 149, 7), (False, 1024, 7), (False, 1500, 1024), (True, 21, 7), (True, 1500, 7)])
def test_importance_coder_repeated_columns(monkeypatch, engine, oracle, wide, S, m):
    host, omega = _wide_blocks() if wide else _golden_block()
    got, want, weights = _gc_call(monkeypatch, engine, oracle, host, omega, S, lambda tab: T.repeat_columns(tab, S, m))
    for blk, ws in zip(got, weights):
        assert all(0 <= j < m for j in blk), (blk, m)
        for j, w in zip(blk, ws):                 # the referee's own weights: the winner's weight occurs again at every j + m i
            assert all(w[s] == w[j] for s in range(j, S, m))
    assert any(j + m < S for blk in got for j in blk), "no winner has a twin: no step of this call had a tie to break"
    assert any(j for blk in got for j in blk), "every index is 0: the row an untouched output buffer would show"


@pytest.mark.gpu
@pytest.mark.parametrize("wide,S", [(False, 21), (False, 149), (True, 21), (True, 1500)])
def test_importance_coder_non_finite_weights(monkeypatch, engine, oracle, wide, S):
    host, omega = _wide_blocks() if wide else _golden_block()
    m = 7
    clean, _, _ = _gc_call(monkeypatch, engine, oracle, host, omega, S, lambda tab: T.repeat_columns(tab, S, m))
    j0 = clean[0][0]                               # block 0's winner of step 0 under the clean table; j0 + 7 carries the same column

    # (a) NaN columns: 0, 5 and the winner's at step 0 are never chosen; every column of step 1 NaN: index 0, the accumulator's start
    def nans(tab):
        T.repeat_columns(tab, S, m)
        tab[0, :, [0, 5, j0]] = np.nan
        tab[1, :, :S] = np.nan
    got, _, weights = _gc_call(monkeypatch, engine, oracle, host, omega, S, nans)
    for blk, ws in zip(got, weights):
        assert np.isnan(ws[0][[0, 5, j0]]).all() and np.isfinite(np.delete(ws[0], [0, 5, j0])).any()
        assert blk[0] not in (0, 5, j0)
        assert np.isnan(ws[1]).all() and blk[1] == 0
    assert got[0][0] == j0 + m                     # block 0: the same column as before, from the next sample that carries it

    # (b) a weight of -inf loses to any finite weight, and is not a NaN's equal either
    #     3e38: x * x overflows in BOTH log-densities, the term is (-inf) - (-inf), the weight a NaN;
    #     1.5e19: (x / ts)^2 overflows where ts < 0.81 while x * x does not: the target's log-density alone is -inf, and so is the weight
    def infs(tab):
        T.repeat_columns(tab, S, m)
        tab[0, :, j0] = np.float32(3e38)
        tab[0, :, (j0 + m) % S] = np.float32(1.5e19)
    got, _, weights = _gc_call(monkeypatch, engine, oracle, host, omega, S, infs)
    for blk, ws in zip(got, weights):
        assert np.isnan(ws[0][j0]) and ws[0][(j0 + m) % S] == -np.inf, (ws[0][j0], ws[0][(j0 + m) % S])
        assert blk[0] not in (j0, (j0 + m) % S) and np.isfinite(ws[0][blk[0]])
