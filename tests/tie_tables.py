"""Quantile tables and normal proposal tables under which the coders' deciding comparisons do NOT decide (helpers of
tests/test_tie_breaking.py; no test functions here).

The beam coder's score of a candidate is a function of the z vector its D look-ups return (irec_oracle.c: T(s,b) = tree-sum of
(G_bd + H_d z) z).  Under a table that is one constant everywhere except in R "spikes", every sample none of whose look-ups hits a
spike has the same z vector as every other such sample, so its score is bit-identical to theirs whatever the summation order, and
the beams grown from such samples are identical too.  With R = 10006 lambda / D a sample misses every spike with probability
~exp(-lambda): ties are the common case, and the spikes keep the outcome from being trivial.

The contract a tie is settled by (oracle/irec_oracle.c: cand_before): value descending, exact ties to the lower flat index
s * B_cur + b, a NaN after every number."""
import contextlib

import numpy as np

P = 10007
BASE = np.float32(0.25)
SPIKES = np.array([0.5, -0.5, 1.0, -1.0, 2.0, -2.0], dtype=np.float32)
POISON = np.float32(2.0 ** 96)          # finite in float32; H z z, the score term it enters, is not
# The ladder pick_lambda walks: (lambda, spike values).  The last four rungs are for calls of few beams and hundreds of samples: a
# table has at least one spike, S * D / 10006 samples of a step meet it (16 at S = 80, D = 2048; 134 at S = 1339, D = 1000), and a
# tie at the cut-off needs nearly every one of them to lose to the unspiked samples -- which a spike of +-2 does not do often enough,
# and one of +-32 .. +-1024 does.
LADDER = ((0.5, SPIKES), (0.1, SPIKES), (0.02, SPIKES), (0.02, (32.0, -32.0)), (0.02, (64.0, -64.0)), (0.02, (256.0, -256.0)),
          (0.02, (1024.0, -1024.0)))
MIN_SHARE = 0.25


def constant_lut():
    """Every candidate of every step ties."""
    lut = np.full(P, BASE, dtype=np.float32)
    lut[0] = 0.0
    return lut


def _spikes(dim, lam, seed, values=SPIKES):
    """(entries, values) of the spikes: R = max(1, round(10006 lam / dim)) distinct entries of 1..10006."""
    values = np.asarray(values, dtype=np.float32)
    n = max(1, int(round((P - 1) * float(lam) / int(dim))))
    rng = np.random.default_rng([int(dim), int(round(float(lam) * 1e6)), int(seed), 7331])
    at = rng.choice(np.arange(1, P), size=n, replace=False)
    return at, values[rng.integers(0, len(values), size=n)]


def spiky_lut(dim, lam, seed=0, values=SPIKES):
    """float32 [10007]: 0.25 everywhere (entry 0 = 0) except R = max(1, round(10006 lam / dim)) randomly chosen entries, which take
    values from `values` ({+-0.5, +-1, +-2} unless a rung of the ladder says otherwise).  Deterministic from its arguments."""
    lut = constant_lut()
    at, val = _spikes(dim, lam, seed, values)
    lut[at] = val
    assert lut.dtype == np.float32 and lut.shape == (P,) and lut[0] == 0 and np.isfinite(lut).all()
    return lut


def poisoned_lut(dim, lam, seed=0):
    """spiky_lut with half of its spikes (every other one, rounded up) replaced by +-2**96: H z z, the score term the entry enters,
    overflows float32, so the scores contain +-inf and (inf - inf) NaN while every table entry stays finite."""
    lut = spiky_lut(dim, lam, seed)
    at, _ = _spikes(dim, lam, seed)
    bad = at[::2]
    lut[bad] = np.where(np.arange(len(bad)) % 2 == 0, POISON, -POISON).astype(np.float32)
    assert np.isfinite(lut).all()
    return lut


@contextlib.contextmanager
def oracle_table(oracle, lut):
    """The oracle's coder functions under `lut`; the restated table is always restored."""
    oracle.set_lut(lut)
    try:
        yield
    finally:
        oracle.set_lut(None)


def rank(score):
    """Flat indices in the contract's order: value descending, ties to the lower index, NaN last (cand_before)."""
    sc = np.asarray(score, dtype=np.float32)
    key = np.where(np.isnan(sc), -np.inf, sc.astype(np.float64))
    order = np.argsort(-key, kind="stable")                       # (-inf scores and NaN share a key: split them below)
    nan = np.isnan(sc[order])
    return np.concatenate([order[~nan], order[nan]])


def steps_of(trace, S, B):
    """(t, N, B_new, scores [N]) of every step of one encode_block(trace=True) trace."""
    Bcur = 1
    for t in range(trace["K"]):
        N = S * Bcur
        Bnew = min(B, N)
        yield t, N, Bnew, trace["score"][t][:N]
        Bcur = Bnew


def case_inputs(oracle, case, widen=False):
    """kernel_names.case_inputs: the host arrays test_every_planned_kernel_matches_the_oracle codes for a planner case.
    widen: every eighth dim's posterior is 1.5 times as wide as its prior.  synthetic_latent's posteriors are narrower than their
    priors in every dim, so the quadratic coefficient H_d of a score is negative everywhere and no table can drive a score to
    +inf; a wider dim has H_d > 0."""
    import kernel_names as kn
    host = kn.case_inputs(oracle, case)
    if widen:
        host[1][:, ::8] = np.float32(1.5) * host[3][:, ::8]
    return host


def outputs(oracle, lut, case, host, **wrong_order):
    """(indices per block, samples) of the whole call from the oracle under `lut` -- by the contract, or, with ties_to_higher /
    nan_first, by that deliberately wrong ordering (oracle.set_wrong_order); the contract is always restored."""
    with oracle_table(oracle, lut):
        oracle.set_wrong_order(**wrong_order)
        try:
            idx, smp, _ = oracle.encode_tensors_omp(*host, 42, 3.0, case["S"], case["B"], case["dim"], max_K=case["max_K"])
        finally:
            oracle.set_wrong_order()
    return [blk[0] for blk in idx], smp


def exposes(oracle, lut, case, widen=False, **wrong_order):
    """How many blocks of the call come out differently (indices or sample) when the oracle orders candidates wrongly: what a kernel
    with that ordering would get wrong under this table, as seen in what the coder EMITS."""
    host = case_inputs(oracle, case, widen=widen)
    idx0, smp0 = outputs(oracle, lut, case, host)
    idx1, smp1 = outputs(oracle, lut, case, host, **wrong_order)
    same = lambda a, b: np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])
    return sum(idx0[i] != idx1[i] or not same(smp0[i], smp1[i]) for i in range(case["n_blocks"]))


def traces(oracle, lut, case, n_sample=16, margins=False, widen=False):
    """encode_block(trace=True) of the first min(n_blocks, n_sample) blocks of a case under `lut`."""
    host = case_inputs(oracle, case, widen=widen)
    out = []
    with oracle_table(oracle, lut):
        for i in range(min(case["n_blocks"], n_sample)):
            out.append(oracle.encode_block(*(h[i] for h in host), 42, 3.0, case["S"], case["B"], max_K=case["max_K"], trace=True,
                                           margins=margins))
    return out


def cutoff_tie_stats(oracle, lut, case, n_sample=16):
    """Over the first min(n_blocks, n_sample) blocks of a case, from oracle.encode_block(..., trace=True) under `lut`:
      rejecting    (block, step) pairs that reject a candidate (S * B_cur > B_new);
      cutoff_ties  those of them with a tie that DECIDES what is emitted: before the last step score[rank B_new - 1] ==
                   score[rank B_new] exactly -- a kernel with any other tie rule keeps a different candidate set there --, at the
                   last step score[rank 0] == score[rank 1]: the coder emits beam 0 alone, so a tie at rank B of the last step
                   shows in nothing;
      inner_ties   steps with two equal scores inside the selected set (the ORDER of the new beams is at stake);
      nonzero      some index differs from 0;
      tied_blocks  per block: a cut-off tie at a step before the last (the margin m_gap of such a block is exactly 0)."""
    rejecting = cutoff = inner = 0
    nonzero, tied_blocks = False, []
    for idx, _, tr in traces(oracle, lut, case, n_sample):
        nonzero = nonzero or any(idx)
        early = False
        for t, N, Bnew, sc in steps_of(tr, case["S"], case["B"]):
            srt = sc[rank(sc)]
            inner += bool(Bnew >= 2 and (srt[:Bnew - 1] == srt[1:Bnew]).any())
            if N > Bnew:
                rejecting += 1
                if t < tr["K"] - 1:
                    cutoff += bool(srt[Bnew - 1] == srt[Bnew])
                    early = early or bool(srt[Bnew - 1] == srt[Bnew])
                else:
                    cutoff += bool(srt[0] == srt[1])
        tied_blocks.append(early)
    return dict(rejecting=rejecting, cutoff_ties=cutoff, inner_ties=inner, nonzero=nonzero, tied_blocks=tied_blocks,
                share=cutoff / rejecting if rejecting else 0.0)


def pick_lambda(oracle, case, ladder=None):
    """The first rung (lambda, spike values) of the ladder whose table (a) ties decisively in at least MIN_SHARE of the case's
    rejecting (block, step) pairs, (b) moves some index off 0 and (c) makes the oracle EMIT something else when it breaks ties
    towards the higher index; failing that, the rung of the greatest share.
    -> ((lambda, values), its cutoff_tie_stats with `exposed`: the blocks (c) changes)."""
    best = None
    for lam, values in (LADDER if ladder is None else ladder):
        lut = spiky_lut(case["dim"], lam, 0, values)
        st = cutoff_tie_stats(oracle, lut, case)
        st["exposed"] = exposes(oracle, lut, case, ties_to_higher=True)
        if st["rejecting"] and st["share"] >= MIN_SHARE and st["nonzero"] and st["exposed"]:
            return (lam, values), st
        key = lambda x: (x["exposed"] > 0, x["nonzero"], x["share"])
        if best is None or key(st) > key(best[1]):
            best = ((lam, values), st)
    return best


def nonfinite_stats(oracle, lut, case, n_sample=16, widen=True):
    """What the oracle's traced scores under `lut` contain: steps with a NaN, a +inf, a -inf, and steps where a NaN ranked before
    every number would change what is emitted (`nan_decides`): the selected SET of a step before the last, rank 0 of the last."""
    out = dict(nan=0, pinf=0, ninf=0, nan_decides=0)
    for _, _, tr in traces(oracle, lut, case, n_sample, widen=widen):
        for t, N, Bnew, sc in steps_of(tr, case["S"], case["B"]):
            isn = np.isnan(sc)
            out["nan"] += bool(isn.any())
            out["pinf"] += bool((sc == np.inf).any())
            out["ninf"] += bool((sc == -np.inf).any())
            if isn.any() and N > Bnew:
                order = rank(sc)
                nan_first = np.concatenate([order[isn[order]], order[~isn[order]]])
                keep = Bnew if t < tr["K"] - 1 else 1
                out["nan_decides"] += set(order[:keep].tolist()) != set(nan_first[:keep].tolist())
    return out


# ---- the importance coder: a normal proposal table whose columns repeat ------------------------------------------------------
def repeat_columns(table, S, m):
    """out[:, :, s] = out[:, :, s % m] for s < S, in place; the zero padding beyond S stays."""
    src = table[:, :, :m].copy()
    for s in range(m, S):
        table[:, :, s] = src[:, :, s % m]
    return table


def referee_normal(tables, seed0, S):
    """normal(seed, count) for gc_referee.encode_block over doctored tables: {dim: [steps, dim, S_pad]} -> the draws of step
    seed - seed0 in the stream's own [S, dim] order."""
    def normal(seed, count):
        dim = count // S
        assert dim * S == count
        return np.ascontiguousarray(tables[dim][seed - seed0, :, :S].T).reshape(-1)
    return normal


POISON_LADDER = tuple((lam, seed) for lam in (0.5, 1.0, 2.0, 4.0, 8.0) for seed in (0, 1, 2, 3))


def pick_poison(oracle, case):
    """The first (lambda, seed) whose poisoned table puts a NaN, a +inf and a -inf into the oracle's scores of the case, the NaN in a
    step it would decide if it ranked first, and makes the oracle EMIT something else when a NaN does rank first (`exposed`
    blocks); failing that, the last one tried.  -> ((lambda, seed), its nonfinite_stats)."""
    for lam, seed in POISON_LADDER:
        lut = poisoned_lut(case["dim"], lam, seed)
        st = nonfinite_stats(oracle, lut, case)
        if min(st.values()) >= 1:
            st["exposed"] = exposes(oracle, lut, case, widen=True, nan_first=True)
            if st["exposed"]:
                break
    st.setdefault("exposed", 0)
    return (lam, seed), st
