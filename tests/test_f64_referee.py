"""The encoder against an independent float64 referee (tests/f64_referee.py) on latents shaped like a trained model's
(tests/latent_families.py), instead of against the oracle alone on oracle.synthetic_latent.

Every parity test elsewhere asserts GPU == oracle/irec_oracle.c bit for bit, and the oracle's CANONICAL mode follows the kernels'
own algebra: a loss of precision of that algebra would be shared by both and stay invisible.  The referee restates the scores,
K and the sample in float64 from the reference's formulas and bounds the float32 error of each score to first order.

CPU (both_suites): the oracle's CANONICAL and LITERAL modes against the referee -- per-candidate score error under the bound,
the selected set equal to the float64 top-B wherever the gap exceeds twice the bound, K equal to ceil(kl64 / Omega) away from
integer boundaries, the sample within the decode bound -- plus negative controls that the referee must catch.
GPU: every planned kernel on every non-benign family (GPU == oracle bit for bit, and the GPU's path passes the referee), the KL
pre-pass, the margins, the decoders, and the subnormal probe."""
import ctypes
import functools

import numpy as np
import pytest

import f64_referee as R
import kernel_names as kn
import latent_families as L

U = 2.0 ** -24
CONFIGS = ((3.0, 1.2, 20), (3.0, 1.2, 10), (3.0, 1.0, 1), (5.0, 1.0, 30))
DIMS = (1, 37, 256, 1000, 1024)
SEED = 42

# The bound on the float32 error of one score, after the shared per-step constant is removed, is C * u * mag, where mag is the
# referee's first-order sum (f64_referee.rescore / _error_units): every float32 rounding of the step constants, of the beams and
# of the term, propagated through the derivatives of the term, plus the rounding of the sum -- (10 + ng) u sum|term| for the
# CANONICAL tree (4 fma per lane, 6 tree levels, ng - 1 group additions), u sum_k |S_k| for LITERAL's sequential sum.  That is
# a worst case to first order: every rounding at its full u and all of them aligned.  They do not align -- on the committed seeds
# the largest error reaches about 1/16 of that sum for CANONICAL and 1/7 for LITERAL (test_bound_is_tight prints the ratios) --
# so C is that measured fraction with a margin of ~3-4x: small enough to stay within 8x of the worst error seen.
C_SCORE = {0: 0.25, 1: 0.5}
# The decode bound: beams[0] + mu_p is sum_t y_t + mu_p, y_t = sqrt(a_t) z_t.  The sequential float32 sum rounds each partial sum
# ((K + 1 - t) |y_t| over the steps it passes), a_t = rho (var_p - c) inherits c's accumulated error (t + 2) u var_p, which moves
# sqrt(a_t) by that over 2 sqrt(a_t), and the final + mu_p rounds once: mag of f64_referee.decode64.  C = 1.
C_DECODE = 1.0


def _k_ok(K, bl, omega):
    """(K equals K64, or kl/Omega is within 1e-5 * kl/Omega of an integer: K's boundary, where either side is right)"""
    kl = R.kl64(*bl)
    k64, dist = R.K64(kl, omega)
    near = dist <= 1e-5 * kl / omega
    return K == k64 or near, near


def check_steps(steps, trace, B, mode, c=None):
    """Score errors and selections of one traced block against the referee.  Returns (worst ratio, steps with a gap below
    twice the bound, violations)."""
    c = C_SCORE[mode] if c is None else c
    worst, tight, bad = 0.0, 0, []
    for t, st in enumerate(steps):
        N = len(st["score"])
        at = st["at"]
        mag = st["mag_canonical" if mode == 0 else "mag_literal"]
        d = trace["score"][t][:N].astype(np.float64)[at] - st["score"][at]
        # |e_j - median(e)| <= b_j + median(b): the median of the errors is at most the median of their bounds
        err = np.abs(d - np.median(d))
        bound = c * U * (mag + np.median(mag))
        ratio = err / (U * (mag + np.median(mag)))
        worst = max(worst, float(ratio.max()))
        if not (err <= bound).all():                     # (NaN fails too)
            j = int(np.argmax(np.where(np.isnan(err), np.inf, err / bound)))
            bad.append(f"step {t}: candidate {int(at[j])} error {err[j]:.3g} > bound {bound[j]:.3g} (ratio {ratio[j]:.3g})")
        Bnew = min(B, N)
        if N > Bnew:
            rank = np.argsort(-st["score"], kind="stable")
            pos = {int(f): i for i, f in enumerate(at)}
            gap = st["score"][rank[Bnew - 1]] - st["score"][rank[Bnew]]
            b2 = 2.0 * max(bound[pos[int(rank[Bnew - 1])]], bound[pos[int(rank[Bnew])]])
            chosen = {int(s) * st["Bcur"] + int(b) for s, b in trace["sel"][t][:Bnew]}
            if gap > b2:
                if chosen != {int(f) for f in rank[:Bnew]}:
                    bad.append(f"step {t}: selection differs from the float64 top-{Bnew} with gap {gap:.3g} > {b2:.3g}")
            else:
                tight += 1
    return worst, tight, bad


def path_passes(steps, indices, mode=0):
    """The selection check on a coder's index path alone (the GPU's): at every step the candidate on the path is in the float64
    top-Bnew (rank 0 at the last step) unless the float64 gap there is within twice the bound."""
    bad = []
    K = len(indices)
    for t, st in enumerate(steps):
        prefix = tuple(int(i) for i in indices[:t])
        if prefix not in st["paths"]:
            bad.append(f"step {t}: the path's prefix is not one of the beams")
            break
        f = int(indices[t]) * st["Bcur"] + st["paths"].index(prefix)
        N = len(st["score"])
        keep = 1 if t == K - 1 else steps[t + 1]["Bcur"]          # (Bnew of step t)
        rank = np.argsort(-st["score"], kind="stable")
        if f in {int(g) for g in rank[:keep]} or N <= keep:
            continue
        mag = st["mag_canonical" if mode == 0 else "mag_literal"]
        b2 = 2.0 * C_SCORE[mode] * U * (mag.max() + np.median(mag))
        gap = st["score"][rank[keep - 1]] - st["score"][f]
        if gap > b2:
            bad.append(f"step {t}: candidate {f} is {gap:.3g} below the float64 rank {keep - 1} (bound {b2:.3g})")
    return bad


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle import oracle as O
    O.lib()
    return O


@functools.lru_cache(maxsize=None)
def _case(family, mode, cfg, D):
    """Every block of (family, D) encoded by the oracle in `mode` at cfg, traced and rescored: the numbers the CPU tests read."""
    O = _oracle()
    omega, eps1, B = cfg
    S = O.n_samples(omega, eps1)
    out = []
    for bl in L.blocks(family, D, 0, omega):
        idx, samp, tr = O.encode_block(*bl, SEED, omega, S, B, mode, max_K=4096, trace=True)
        steps = _rescore(bl, omega, S, B, tr["sel"].tobytes(), tr["K"]) if tr["K"] else []
        out.append((bl, idx, samp, tr, steps))
    return out


_rescore_cache = {}


def _rescore(bl, omega, S, B, sel_bytes, K):
    # (both modes usually select the same path: rescored once)
    key = (tuple(a.tobytes() for a in bl), omega, S, B, sel_bytes)
    if key not in _rescore_cache:
        sel = np.frombuffer(sel_bytes, dtype=np.int32).reshape(K, B, 2)
        _rescore_cache[key] = R.rescore(*bl, SEED, omega, S, B, sel)
    return _rescore_cache[key]


def _dims(cfg):
    # (5, 1.0, 30) scores 4440 candidates a step: at the two large dims that alone would take most of the CPU budget
    return DIMS if cfg[2] < 30 else DIMS[:3]


@functools.lru_cache(maxsize=None)
def _stats(family, mode):
    """(worst ratio, steps within twice the bound, near-integer K blocks, violations) over the grid."""
    O = _oracle()
    worst, tight, near_n, bad = 0.0, 0, 0, []
    for cfg in CONFIGS:
        S = O.n_samples(cfg[0], cfg[1])
        for D in _dims(cfg):
            for j, (bl, idx, samp, tr, steps) in enumerate(_case(family, mode, cfg, D)):
                where = f"{family} mode {mode} {cfg} D={D} block {j}"
                ok, near = _k_ok(tr["K"], bl, cfg[0])
                near_n += near
                if not ok:
                    bad.append(f"{where}: K {tr['K']} != K64 {R.K64(R.kl64(*bl), cfg[0])}")
                if tr["K"] == 0:
                    continue
                w, tt, b = check_steps(steps, tr, cfg[2], mode)
                worst, tight = max(worst, w), tight + tt
                bad += [f"{where}: {m}" for m in b]
                s64, dmag = R.decode64(bl[2], bl[3], idx, SEED, S)
                derr = np.abs(samp.astype(np.float64) - s64)
                if (derr > C_DECODE * U * dmag).any():
                    i = int(np.argmax(derr / dmag))
                    bad.append(f"{where}: sample dim {i} off by {derr[i]:.3g} > {C_DECODE * U * dmag[i]:.3g}")
    return worst, tight, near_n, bad


@pytest.mark.both_suites
@pytest.mark.usefixtures("suite")
@pytest.mark.parametrize("mode", [0, 1], ids=["canonical", "literal"])
@pytest.mark.parametrize("family", L.FAMILIES)
def test_oracle_against_the_float64_referee(family, mode):
    worst, tight, near_n, bad = _stats(family, mode)
    print(f"{family} mode {mode}: worst error/bound ratio {worst:.3g}, {tight} steps within twice the bound, {near_n} near-integer K")
    assert not bad, "\n".join(bad[:10])
    if family == "mixed":
        assert near_n >= 2 * len(CONFIGS), near_n     # the K-boundary blocks are there and counted, not skipped


@pytest.mark.both_suites
@pytest.mark.usefixtures("suite")
@pytest.mark.parametrize("mode", [0, 1], ids=["canonical", "literal"])
def test_bound_is_tight(mode):
    """C_SCORE may be at most 8x the largest error/bound ratio the committed seeds reach: a bound nothing comes near tests nothing."""
    ratios = {f: _stats(f, mode)[0] for f in L.FAMILIES}
    worst = max(ratios.values())
    print("error/bound ratios:", {f: round(r, 4) for f, r in ratios.items()})
    assert C_SCORE[mode] <= 8.0 * worst, (C_SCORE[mode], ratios)


NEGATIVE = ("ratio_index", "drop_var_term", "sa_for_sa2", "lut_bit")


@pytest.mark.both_suites
@pytest.mark.usefixtures("suite")
@pytest.mark.parametrize("fault", NEGATIVE)
@pytest.mark.parametrize("family,D", [("sharp", 37), ("benign", 256)])
def test_referee_catches_a_planted_mistake(family, D, fault):
    """Negative controls: the referee with one mistake planted -- rho_t for rho_{K-1-t}, the v (var_p - v) / var_p term of var
    dropped, sa in place of sa^2 in v, one flipped bit of a quantile-table entry a step reads -- must fail the score check."""
    O = _oracle()
    omega, eps1, B = CONFIGS[0]
    S = O.n_samples(omega, eps1)
    bl = L.block(family, D, 0, omega)
    idx, samp, tr = O.encode_block(*bl, SEED, omega, S, B, 0, max_K=4096, trace=True)
    assert tr["K"] >= 2
    assert not check_steps(R.rescore(*bl, SEED, omega, S, B, tr["sel"]), tr, B, 0)[2]
    with np.errstate(invalid="ignore"):
        steps = R.rescore(*bl, SEED, omega, S, B, tr["sel"], _faults=(fault,))
    assert check_steps(steps, tr, B, 0)[2], fault


# ---- the reference's own seeded vector ----------------------------------------------------------------------------------------
@pytest.mark.both_suites
@pytest.mark.usefixtures("suite")
def test_reference_notebook_bernoulli_bits():
    """notebooks/Discrete REC.ipynb, cell 2: tf.random.set_seed(42); Bernoulli(probs=0.7).sample(100) -- TFP draws
    uniform([100]) with no op seed and compares it with probs.  The stored output pins the op-seed-None path of the seed
    plumbing: the first auto-seed of global seed 42.  The two wrong hypotheses -- an explicit op seed of 42,
    the second auto-seed -- must not reproduce it."""
    import os
    from conftest import GOLDEN_DIR
    O = _oracle()
    g = np.load(os.path.join(GOLDEN_DIR, "ref_notebook_bernoulli42.npz"))
    bits, seed, probs = g["bits"], int(g["global_seed"]), np.float32(g["probs"])
    assert bits.shape == (100,) and bits.dtype == np.int32
    rng = O.TfEagerRandom(seed)
    first = (rng.uniform(100) < probs).astype(np.int32)
    second = (rng.uniform(100) < probs).astype(np.int32)
    assert np.array_equal(first, bits)
    assert not np.array_equal(second, bits)
    assert not np.array_equal((O.TfEagerRandom(seed).uniform(100, seed=seed) < probs).astype(np.int32), bits)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _plans():
    return kn.enumerate_plans(256)


def _names():
    try:
        return sorted(_plans())
    except Exception:        # (the library is missing: tests/test_kernel_coverage.py says so)
        return []


def _call_blocks(family, n_blocks, dim, max_K, omega, salt):
    """n_blocks blocks of `family` for one call (mixed: its members in turn, starting at `salt`)."""
    if family == "mixed":
        pool = L.mixed(dim, salt, omega, max_K)
        return [pool[(salt + j) % len(pool)] if j < len(pool) else L.mixed(dim, salt + j, omega, max_K)[(salt + j) % len(pool)]
                for j in range(n_blocks)]
    return [L.block(family, dim, salt + j, omega, max_K) for j in range(n_blocks)]


def _encode_gpu(engine, params, lay, host, max_K, margins=False):
    import torch
    ql, qs, pl, ps = (torch.from_numpy(a).cuda().contiguous() for a in host)
    if margins:
        out = engine.encode_blocks_margins(params, lay, ql, qs, pl, ps, SEED, max_K)
    else:
        out = engine.encode_blocks(params, lay, ql, qs, pl, ps, SEED, max_K)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out)


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names())
def test_every_planned_kernel_on_model_shaped_latents(engine, oracle, name):
    """Every kernel name the planner can launch (the cheapest call of tests/kernel_names.py's grid), on every non-benign family:
    K, indices and sample equal to oracle.encode_tensors_omp bit for bit, and the GPU's index paths pass the referee.  The calls at the
    edges of a name's range, with the referee on the call of the most beams that it can afford, are tests/test_kernel_corners.py's."""
    from irec import _lib
    ex = _plans()[name]
    B, S, n_blocks, dim, max_K, flags = ex["B"], ex["S"], ex["n_blocks"], ex["dim"], ex["max_K"], ex["flags"]
    margins = bool(flags & _lib.IREC_FLAG_MARGINS)
    omega = 3.0
    lay = engine.layout(n_blocks, dim, dim, SEED)
    params = engine.params(omega, S, B, flags & ~_lib.IREC_FLAG_MARGINS)
    assert kn.canonical(engine.plan(params, lay, max_K, margins=margins)["kernel"], engine.plan(params, lay, max_K, margins=margins)["split"]) == name
    perm = oracle.tf_shuffle_perm(SEED, dim)
    for fi, family in enumerate(L.NON_BENIGN):
        host = L.stack(_call_blocks(family, n_blocks, dim, max_K, omega, salt=fi + 7 * len(name)))
        Kh, ih, sh = _encode_gpu(engine, params, lay, host, max_K, margins)[:3]
        sh = sh.reshape(n_blocks, dim)
        assert Kh.min() >= 0 and Kh.max() <= max_K, (name, family, int(Kh.min()), int(Kh.max()))
        ridx, rs, _ = oracle.encode_tensors_omp(*host, SEED, omega, S, B, dim, max_K=max_K)
        for i in range(n_blocks):
            row = lay.natural[i]
            assert ih[row, :Kh[row]].tolist() == ridx[i][0], (name, family, i)
        assert np.array_equal(sh, rs), (name, family)
        for i in range(min(n_blocks, 3)):               # the referee on the first blocks of the call (cost)
            row = lay.natural[i]
            if Kh[row] == 0:
                continue
            bl = tuple(a[i][perm] for a in host)
            _, _, tr = oracle.encode_block(*bl, SEED, omega, S, B, trace=True)
            bad = path_passes(R.rescore(*bl, SEED, omega, S, B, tr["sel"], n_spread=32), ih[row, :Kh[row]])
            assert not bad, (name, family, i, bad[:3])


def _family_call(family, D=192, omega=3.0):
    bls = [b for s in range(2) for b in L.blocks(family, D, s, omega)]
    return bls, L.stack(bls)


@pytest.mark.gpu
@pytest.mark.parametrize("family", L.FAMILIES)
def test_block_kl_on_model_shaped_latents(engine, oracle, family):
    """irec_block_kl (the KL pre-pass): within 1e-6 relative of the float64 closed form, K equal to the oracle's."""
    D, omega = 192, 3.0
    bls, host = _family_call(family, D, omega)
    import torch
    lay = engine.layout(len(bls), D, D, SEED)
    params = engine.params(omega, 36, 20)
    dev = [torch.from_numpy(a).cuda().contiguous() for a in host]
    kl, K = engine.block_kl(params, lay, *dev)
    kl, K = kl.cpu().numpy(), K.cpu().numpy()
    perm = oracle.tf_shuffle_perm(SEED, D)
    for i, bl in enumerate(bls):
        row = lay.natural[i]
        k64 = R.kl64(*bl)
        assert abs(float(kl[row]) - k64) <= 1e-6 * k64, (family, i, float(kl[row]), k64)
        assert int(K[row]) == oracle.num_aux(oracle.block_kl(*(a[perm] for a in bl)), omega), (family, i)


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["sharp", "mixed"])
def test_margins_on_model_shaped_latents(engine, oracle, family):
    """irec_beam_encode_ex's margins equal the oracle's bit for bit; wherever the referee's float64 gap between the last selected
    and the best rejected candidate exceeds twice the bound, it has the float32 gap's sign (>= 0)."""
    D, omega, eps1, B = 192, 3.0, 1.2, 20
    S = oracle.n_samples(omega, eps1)
    bls, host = _family_call(family, D, omega)
    lay = engine.layout(len(bls), D, D, SEED)
    params = engine.params(omega, S, B)
    Kh, ih, sh, mg = _encode_gpu(engine, params, lay, host, 64, margins=True)
    ridx, rs, _, rmg = oracle.encode_tensors_omp(*host, SEED, omega, S, B, D, max_K=64, margins=True)
    perm = oracle.tf_shuffle_perm(SEED, D)
    for i, bl in enumerate(bls):
        row = lay.natural[i]
        assert ih[row, :Kh[row]].tolist() == ridx[i][0], (family, i)
        assert np.array_equal(mg[row], rmg[i, 0]), (family, i, mg[row], rmg[i, 0])
        if Kh[row] == 0:
            continue
        pb = tuple(a[perm] for a in bl)
        _, _, tr = oracle.encode_block(*pb, SEED, omega, S, B, trace=True)
        steps = R.rescore(*pb, SEED, omega, S, B, tr["sel"])
        for t, st in enumerate(steps[:-1]):
            N = len(st["score"])
            Bnew = min(B, N)
            if N <= Bnew:
                continue
            order = np.argsort(-(tr["score"][t][:N].astype(np.float32) + np.float32(0)), kind="stable")   # the float32 ranks
            last, rej = int(order[Bnew - 1]), int(order[Bnew])
            gap64 = st["score"][last] - st["score"][rej]
            pos = {int(f): j for j, f in enumerate(st["at"])}
            mag = st["mag_canonical"]
            b2 = 2.0 * C_SCORE[0] * U * (max(mag[pos[last]], mag[pos[rej]]) + np.median(mag))
            assert gap64 >= 0 or -gap64 <= b2, (family, i, t, gap64, b2)


@pytest.mark.gpu
@pytest.mark.parametrize("family", L.FAMILIES)
def test_decoders_on_model_shaped_latents(engine, oracle, family):
    """Every decode mode on the encoded outputs of every family: equal to oracle.decode_tensor bit for bit and within the decode
    bound of the referee's float64 sample.  offset (mu_p ~ 200) and tiny (sigma_p ~ 1e-3) are the ones that matter here."""
    import torch
    D, omega, eps1, B = 192, 3.0, 1.2, 20
    S = oracle.n_samples(omega, eps1)
    bls, host = _family_call(family, D, omega)
    n_t = len(bls)
    lay = engine.layout(n_t, D, D, SEED)
    params = engine.params(omega, S, B)
    ql, qs, pl, ps = (torch.from_numpy(a).cuda().contiguous() for a in host)
    K, idx, sample = engine.encode_blocks(params, lay, ql, qs, pl, ps, SEED, 64)
    assert engine.lib.irec_decode_tensors_supported(ctypes.byref(params), D, D)
    Kh, ih = K.cpu().numpy(), idx.cpu().numpy()
    perm = oracle.tf_shuffle_perm(SEED, D)
    want = np.stack([oracle.decode_tensor(host[2][i], host[3][i], [ih[lay.natural[i], :Kh[lay.natural[i]]].tolist()], SEED, S,
                                          block_size=D) for i in range(n_t)])
    assert np.array_equal(sample.cpu().numpy(), want), family
    for i in range(n_t):
        s64, dmag = R.decode64(host[2][i][perm], host[3][i][perm], ih[lay.natural[i], :Kh[lay.natural[i]]], SEED, S)
        err = np.abs(want[i][perm].astype(np.float64) - s64)
        assert (err <= C_DECODE * U * dmag).all(), (family, i, float((err / dmag).max()))
    for mode in ("auto", "tables", "fused", "legacy", "tensors", "tensors_fused"):
        rec = engine.decode_blocks(params, lay, pl, ps, SEED, K, idx, mode=mode)
        assert np.array_equal(rec.cpu().numpy(), want), (family, mode)


@pytest.mark.gpu
def test_subnormal_probe(engine, oracle):
    """sigma_p ~ 1e-9: var_p ~ 1e-18, the products v * v and var_p * var_p of the step constants sit at ~1e-36, at the bottom of
    float32's normal range.  TensorFlow flushes subnormals on the CPU, so the reference has no defined answer here; asserted:
    GPU == oracle, no NaN.  Finding (MI355X): K, indices and samples equal the oracle's (gcc, IEEE subnormals) bit for bit, no NaN.
    On these seeds (K = 2) the last step's v (var_p - v) / var_p is exactly 0 in both, and one product of one block goes
    subnormal -- so the probe shows the kernels keep the oracle's answer at this edge, not that they would agree on deeply
    subnormal inputs."""
    D, omega, eps1, B = 192, 3.0, 1.2, 20
    S = oracle.n_samples(omega, eps1)
    bls = [L.block("subnormal_probe", D, s, omega) for s in range(4)]
    host = L.stack(bls)
    lay = engine.layout(len(bls), D, D, SEED)
    params = engine.params(omega, S, B)
    Kh, ih, sh = _encode_gpu(engine, params, lay, host, 64)
    ridx, rs, _ = oracle.encode_tensors_omp(*host, SEED, omega, S, B, D, max_K=64)
    assert not np.isnan(sh).any() and not np.isnan(rs).any()
    for i in range(len(bls)):
        row = lay.natural[i]
        assert ih[row, :Kh[row]].tolist() == ridx[i][0], i
    assert np.array_equal(sh.reshape(len(bls), D), rs)
