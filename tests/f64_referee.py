"""An independent float64 statement of BeamSearchCoder.encode_block's scores, K and sample -- the referee of
tests/test_f64_referee.py.  Plain numpy; shares no arithmetic with oracle/irec_oracle.c.  It reads only what the reference
itself takes as given: the float32 quantile table (oracle.build_lut()), the uniform_int stream of
beam_search_coder.py:38-43 (oracle.uniform_int) and the float32 auxiliary-variance ratios (oracle.aux_ratio).

Every score is the full log-density ratio of beam_search_coder.py:84-86,
    sum_d  log N(x_d; m_d, sqrt(var_d)) - log N(x_d; 0, sqrt(v_d)),     x = beam + sqrt(a) z,
with the step constants of coder.py:147-154 and beam_search_coder.py:64-77 evaluated in float64:
    var_p = sp^2,  a = rho_i (var_p - c),  v = a + c,  m = (mq - mp) v / var_p,
    var   = sq^2 v^2 / var_p^2 + v (var_p - v) / var_p,                    c += a after every step.
The beams are rebuilt in float64 along the path a float32 coder chose (its selections), so what differs between the two is the
float32 arithmetic alone."""
import numpy as np

P = 10007
HALF_LOG_2PI = 0.9189385332046727


def kl64(mq, sq, mp, sp):
    """Closed-form KL(N(mq, sq) || N(mp, sp)) summed over the dims, float64."""
    mq, sq, mp, sp = (np.asarray(a, dtype=np.float64) for a in (mq, sq, mp, sp))
    t = sq / sp
    d = (mq - mp) / sp
    return float(np.sum(0.5 * d * d + 0.5 * (t * t - 1.0) - np.log(t)))


def K64(kl, omega):
    """(ceil(kl / omega), distance of kl / omega to the nearest integer).  K = 0 for kl <= 0 (beam_search_coder.py:59)."""
    x = float(kl) / float(omega)
    if not x > 0:
        return 0, float("inf")
    return int(np.ceil(x)), abs(x - np.round(x))


def _wrap32(x):
    """int32 wrap-around (TensorFlow's int32 arithmetic)."""
    return ((int(x) + (1 << 31)) % (1 << 32)) - (1 << 31)


def _hash(hsum):
    """simple_hash (beam_search_coder.py:33-35) from the int32 sum of idx[j] * (69 + j); floormod, so never negative."""
    return _wrap32(hsum) % (P - 1) + 1


def _lut64(lut):
    if lut is None:
        from oracle import oracle as O
        lut = O.build_lut()
    return np.asarray(lut, dtype=np.float32).astype(np.float64)


def _ratios(K, aux_ratio):
    if aux_ratio is None:
        from oracle import oracle as O
        aux_ratio = O.aux_ratio
    return [float(np.float32(aux_ratio(K - 1 - t))) for t in range(K)]


def _draw(seed, t, S, D, uniform_int):
    if uniform_int is None:
        from oracle import oracle as O
        uniform_int = O.uniform_int
    return np.asarray(uniform_int(seed + t, S * D), dtype=np.int64).reshape(S, D)


def rescore(mq, sq, mp, sp, seed, omega, S, B, sel, lut=None, aux_ratio=None, uniform_int=None, n_spread=128, _faults=()):
    """Walks the path of selections `sel` ([K][B][2] (s, b) per step, -1 padded: the oracle's trace["sel"]) and returns one dict
    per step: score [N] float64 in flat s * Bcur + b order; Bcur; paths (the index path of every beam the step starts from); at
    (flat indices of the candidates whose error is bounded: the 2B + 2 best and n_spread more); and
    mag_canonical / mag_literal [len(at)]: the first-order bound on a float32 coder's error in that score, in units of u = 2^-24, for the
    two summation orders of the oracle (see _error_units).  `_faults` (tests only) plants one of the mistakes the negative controls
    must catch."""
    mq, sq, mp, sp = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (mq, sq, mp, sp))
    D = mq.size
    sel = np.asarray(sel)
    K = len(sel)
    lut = _lut64(lut)
    if "lut_bit" in _faults:
        lut = lut.copy()
    rho = _ratios(K, aux_ratio)
    var_p = sp * sp
    var_q = sq * sq
    c = np.zeros(D)
    ec = np.zeros(D)               # error bound of the float32 c, units of u
    beams = np.zeros((1, D))
    eb = np.zeros((1, D))          # error bound of the float32 beams, units of u
    hsum = [0]
    paths = [()]
    out = []
    for t in range(K):
        r_t = rho[t] if "ratio_index" not in _faults else rho[K - 1 - t]     # rho_{K-1-t}, or (fault) rho_t
        a = r_t * (var_p - c)
        v = (a if "sa_for_sa2" not in _faults else np.sqrt(a)) + c      # v = sa^2 + c, or (fault) sa + c
        m = (mq - mp) * v / var_p
        var = var_q * v * v / (var_p * var_p)
        if "drop_var_term" not in _faults:
            var = var + v * (var_p - v) / var_p
        sa = np.sqrt(a)
        r = _draw(seed, t, S, D, uniform_int)
        Bcur = len(beams)
        k = (r[:, None, :] * np.array([_hash(h) for h in hsum], dtype=np.int64)[None, :, None]) % P   # [S, Bcur, D]
        if "lut_bit" in _faults and t == 0:
            # bit 20 of the entry candidate (0, 0) reads in the dim where its score is steepest in z
            x0 = sa * lut[k[0, 0]]
            d0 = int(np.argmax(np.abs((x0 / v - (x0 - m) / var) * sa)))
            k0 = int(k[0, 0, d0])
            lut[k0] = float(np.array([lut[k0]], dtype=np.float32).view(np.uint32).__xor__(np.uint32(1 << 20)).view(np.float32)[0])
        z = lut[k]
        y = sa * z
        x = beams[None, :, :] + y
        q1 = (x - m) ** 2 / (2.0 * var)
        q2 = x * x / (2.0 * v)
        n1 = 0.5 * np.log(var) + HALF_LOG_2PI
        n2 = 0.5 * np.log(v) + HALF_LOG_2PI
        score = (q2 - q1).sum(axis=2).reshape(-1) + float((n2 - n1).sum())
        # the error bounds are evaluated on a subset of the candidates (cost): the 2B + 2 best in float64, and n_spread
        # more spread evenly over the flat order
        N = S * Bcur
        rank = np.argsort(-score, kind="stable")
        at = np.unique(np.concatenate([rank[:2 * B + 2], np.linspace(0, N - 1, min(N, n_spread)).astype(np.int64)]))
        ss, bb = at // Bcur, at % Bcur
        z_, y_, x_, q1_, q2_ = z[ss, bb], y[ss, bb], x[ss, bb], q1[ss, bb], q2[ss, bb]
        # -- first-order error bounds (units of u) of the float32 step constants, one rounding per float32 op
        ea = r_t * (var_p + ec + np.abs(var_p - c)) + a                 # var_p = sp*sp, var_p - c, rho * (.)
        ev = ea + ec + v                                                # a + c
        esa = ea / (2.0 * np.sqrt(np.maximum(a, 1e-300))) + np.sqrt(np.maximum(a, 0.0))
        em = np.abs(m) * (4.0 + ev / v)                                 # (mq - mp) * v / var_p
        t1 = var_q * v * v / (var_p * var_p)
        t2 = v * (var_p - v) / var_p
        evar = (t1 * (7.0 + 2.0 * ev / v) + np.abs(t2) * 4.0 + np.abs(var_p - 2.0 * v) / var_p * ev
                + v / var_p * (var_p + np.abs(var_p - v)) + var)
        ey = np.abs(z_) * esa + np.abs(y_)
        ex = eb[bb] + ey + np.abs(x_)                                   # beam + y
        # the candidate-dependent part of the term's derivatives in x, m, var and v, plus the term's own roundings
        prop = (np.abs(x_ / v - (x_ - m) / var) * ex + np.abs(x_ - m) / var * em + q1_ / var * evar + q2_ / v * ev
                + 4.0 * (q1_ + q2_))
        lit_terms = q2_ - q1_ + (n2 - n1)
        out.append({"score": score, "Bcur": Bcur, "paths": list(paths), "at": at,
                    "mag_canonical": _error_units(prop, q1_ + q2_, None),
                    "mag_literal": _error_units(prop + 2.0 * (np.abs(n1) + np.abs(n2)), None, lit_terms)})
        # the float32 beams' error bounds along the chosen path (the chosen are among the 2B + 2 best or the step's
        # selection disagrees with float64 by more than the bound anyway: those rows fall back to the worst bound seen)
        ex_all = np.full((S, Bcur, D), np.nan)
        ex_all[ss, bb] = ex
        ex_worst = ex.max(axis=0)
        Bnew = min(B, S * Bcur)
        chosen = sel[t][:Bnew]
        beams = np.stack([x[s, b] for s, b in chosen])
        eb = np.stack([ex_all[s, b] if not np.isnan(ex_all[s, b, 0]) else ex_worst for s, b in chosen])
        paths = [paths[b] + (int(s),) for s, b in chosen]
        hsum = [_wrap32(hsum[b] + int(s) * (69 + t)) for s, b in chosen]
        ec = ec + ea + (c + a)
        c = c + a
    return out


def _error_units(prop, tree_terms, seq_terms):
    """Per candidate: the propagated errors summed over the dims, plus the rounding of the sum itself, in units of u.
      CANONICAL (tree_terms): a dim's term passes 4 fma of its lane, 6 levels of the 64-lane tree and at most ng - 1 group
        additions, so the sum adds at most (10 + ng) u sum_d |term_d|.
      LITERAL (seq_terms): a sequential float32 sum rounds every partial sum once: u sum_k |S_k|, S_k = sum_{d<=k} term_d."""
    base = prop.sum(axis=-1)
    if tree_terms is not None:
        ng = (prop.shape[-1] + 255) // 256
        return base + (10 + ng) * tree_terms.sum(axis=-1)
    return base + np.abs(np.cumsum(seq_terms, axis=-1)).sum(axis=-1)


def decode64(mp, sp, indices, seed, S, lut=None, aux_ratio=None, uniform_int=None):
    """The float64 sample beams[0] + mp of the path `indices` (beam_search_coder.py:124-148), and per dim the magnitude the
    decode bound needs: |mp| + sum_t (K + 1 - t) |y_t| + sum_t |z_t| (t + 2) var_p / (2 sqrt(a_t))  (see test_f64_referee)."""
    mp, sp = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (mp, sp))
    D = mp.size
    K = len(indices)
    lut = _lut64(lut)
    rho = _ratios(K, aux_ratio)
    var_p = sp * sp
    c = np.zeros(D)
    sample = np.zeros(D)
    mag = np.abs(mp).copy()
    hsum = 0
    for t in range(K):
        a = rho[t] * (var_p - c)
        sa = np.sqrt(a)
        r = _draw(seed, t, S, D, uniform_int)
        z = lut[(r[int(indices[t])] * _hash(hsum)) % P]
        y = sa * z
        sample = sample + y
        mag = mag + (K + 1 - t) * np.abs(y) + np.abs(z) * (t + 2) * var_p / (2.0 * np.maximum(sa, 1e-300))
        hsum = _wrap32(hsum + int(indices[t]) * (69 + t))
        c = c + a
    return sample + mp, mag
