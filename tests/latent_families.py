"""Seeded generators of (mq, sq, mp, sp) float32 blocks whose statistics look like the latents of a trained model rather than
oracle.synthetic_latent's (sigma_p near 1, a small mean shift, sigma_q within ~5 % of sigma_p).  Shared by tests/test_f64_referee.py.

  benign          oracle.synthetic_latent
  sharp           ~2 % of the dims informative: sigma_q = 0.02 sigma_p, mu_q - mu_p ~ N(0, 3 sigma_p); K in the tens
  collapsed       q == p in every dim except zero to two informative ones: K in {0, 1, 2} at Omega >= 3
  eqvar           sigma_q == sigma_p bit for bit, only the means move (A = 0.5 (1/v - 1/var) is a pure cancellation)
  tiny            sigma_p ~ 1e-3
  wide            sigma_p ~ 1e2
  offset          mu_p ~ 200: the float32 rounding of beams + mu_p
  mixed           blocks of all of the above in ONE call, plus blocks whose KL / Omega sits on an integer (K's boundary)
  subnormal_probe sigma_p ~ 1e-9: the step constants leave the normal float32 range (see its test)

Every family except subnormal_probe keeps every float32 intermediate of the step constants (irec_oracle.c step_constants) a
normal number for the partition counts it produces: TensorFlow flushes subnormals on the CPU, so parity there is undefined."""
import numpy as np

FAMILIES = ("benign", "sharp", "collapsed", "eqvar", "tiny", "wide", "offset", "mixed")
NON_BENIGN = FAMILIES[1:]
_BASE = {f: 100003 * (i + 1) for i, f in enumerate(FAMILIES + ("subnormal_probe",))}


def _f32(*a):
    return tuple(np.asarray(x, dtype=np.float32) for x in a)


def _benign(rng, D, scale=1.0, loc=0.0):
    mp = loc + scale * rng.normal(0.0, 1.0, D)
    lsp = rng.normal(0.0, 0.25, D)
    sp = scale * np.exp(lsp)
    mq = mp + sp * rng.normal(0.0, 0.2, D)
    sq = sp * np.exp(-np.abs(rng.normal(0.0, 0.05, D)))
    return mq, sq, mp, sp


def _sharp(rng, D, n_inf_max=None):
    mq, sq, mp, sp = _benign(rng, D)
    n_inf = max(1, min(int(round(0.02 * D)), n_inf_max or D))
    at = rng.choice(D, n_inf, replace=False)
    sq[at] = 0.02 * sp[at]
    dmu = rng.normal(0.0, 3.0, n_inf)
    if n_inf_max is not None:
        dmu = np.clip(dmu, -6.0, 6.0)             # (at most ~22 nats a dim, so that K stays below a call's max_K)
    mq[at] = mp[at] + dmu * sp[at]
    return mq, sq, mp, sp


def _collapsed(rng, D, omega=3.0):
    mp = rng.normal(0.0, 1.0, D)
    sp = np.exp(rng.normal(0.0, 0.25, D))
    mq, sq = mp.copy(), sp.copy()
    n_inf = int(rng.integers(0, 3)) if D > 1 else int(rng.integers(0, 2))
    at = rng.choice(D, n_inf, replace=False)
    # KL of one dim = 0.5 d^2 with d = (mq - mp) / sp: at most 0.95 Omega per dim, so K <= 2
    kl = rng.uniform(0.2, 0.95, n_inf) * omega
    mq[at] = mp[at] + np.sqrt(2.0 * kl) * sp[at] * rng.choice([-1.0, 1.0], n_inf)
    return mq, sq, mp, sp


def _eqvar(rng, D):
    mp = rng.normal(0.0, 1.0, D)
    sp = np.exp(rng.normal(0.0, 0.5, D))
    mq = mp + sp * rng.normal(0.0, 0.3, D)
    return mq, sp.copy(), mp, sp


def block(family, D, seed, omega=3.0, max_K=None):
    """One block of D dims, float32 (mq, sq, mp, sp).  `family` may not be 'mixed' (see mixed()).  max_K: 'sharp' keeps few enough
    informative dims (at most ~22 nats each) for K to stay below it."""
    rng = np.random.default_rng(_BASE[family] + 7919 * seed + D)
    if family == "benign":
        from oracle import oracle as O
        return O.synthetic_latent(int(rng.integers(1 << 20)), D)
    if family == "sharp":
        out = _sharp(rng, D, None if max_K is None else max(1, int(max_K * omega / 48)))
    elif family == "collapsed":
        out = _collapsed(rng, D, omega)
    elif family == "eqvar":
        out = _eqvar(rng, D)
    elif family == "tiny":
        out = _benign(rng, D, scale=1e-3)
    elif family == "wide":
        out = _benign(rng, D, scale=1e2)
    elif family == "offset":
        out = _benign(rng, D, loc=200.0)
    elif family == "subnormal_probe":
        out = _benign(rng, D, scale=1e-9)
    else:
        raise ValueError(family)
    mq, sq, mp, sp = _f32(*out)
    if family == "eqvar":
        sq = sp.copy()
    return mq, sq, mp, sp


def kl_boundary_block(D, seed, omega, extra_parts):
    """A benign-like block with one strongly shifted dim, whose float64 KL is an integer number of omegas (extra_parts more than
    the rest of the block holds) up to the float32 rounding of that dim's mean: K's boundary."""
    from f64_referee import kl64
    rng = np.random.default_rng(977 + 7919 * seed + D)
    mq, sq, mp, sp = _f32(*_benign(rng, D))
    j = D - 1
    rest = kl64(mq[:j], sq[:j], mp[:j], sp[:j]) if j else 0.0
    t = float(sq[j]) / float(sp[j])
    var_part = 0.5 * (t * t - 1.0) - np.log(t)
    need = (np.ceil((rest + var_part) / omega) + extra_parts) * omega - rest - var_part       # = 0.5 d^2 of dim j
    mq[j] = np.float32(float(mp[j]) + np.sqrt(2.0 * need) * float(sp[j]))
    return mq, sq, mp, sp


def mixed(D, seed, omega=3.0, max_K=None):
    """The blocks of one call: every other family (sharp twice, so K reaches ~70 at D = 1000) plus two K-boundary blocks."""
    out = [block(f, D, seed, omega, max_K) for f in ("benign", "sharp", "collapsed", "eqvar", "tiny", "wide", "offset")]
    out.append(block("sharp", D, seed + 1000, omega, max_K))
    out.append(kl_boundary_block(D, seed, omega, extra_parts=1))
    out.append(kl_boundary_block(D, seed + 1, omega, extra_parts=3))
    return out


def blocks(family, D, seed, omega=3.0, max_K=None):
    """List of blocks: one for a plain family, all of mixed()'s for 'mixed'."""
    return mixed(D, seed, omega, max_K) if family == "mixed" else [block(family, D, seed, omega, max_K)]


def stack(blocks_):
    """[n_blocks, D] float32 arrays (mq, sq, mp, sp) of blocks of equal D."""
    return tuple(np.ascontiguousarray(np.stack([b[j] for b in blocks_])) for j in range(4))
