"""numpy referee of the sequential importance coder at FINITE alpha: tests/gc_referee.py with the selection of
importance_sampling.py:67-72 in place of the arg-max --

    v[s]  = float32(alpha) * w[s] + g[s]      one float32 multiply, then one float32 add
    index = first s with the greatest v[s]; the accumulator starts at (0, -FLT_MAX) and moves on a strict ">"

The weights w are gc_referee.importance_step's (the same arithmetic as at alpha = inf); the perturbations are the caller's:
`gumbel(step_seed, S)` -> float32 [S], by default stateless_gumbel_sample([S], step_seed + 1) (rec/coding/utils.py:9-12).
Test infrastructure: shared by tests/test_gc_importance_alpha_host.py and tests/test_gc_importance_alpha_gpu.py.
"""
import numpy as np

import gc_referee as R

f32 = np.float32


def reference_gumbel(step_seed, S):
    from irec.coding.utils import stateless_gumbel_sample
    return stateless_gumbel_sample((S,), step_seed + 1)


def select(w, g, alpha):
    """-> index.  A NaN is never chosen, +inf can win, -inf never does (it is not greater than -FLT_MAX)."""
    with np.errstate(all="ignore"):
        v = (f32(alpha) * np.asarray(w, f32)).astype(f32) + np.asarray(g, f32)
    best, j = -R.FLT_MAX, 0
    for s, x in enumerate(v.astype(f32)):
        if x > best:
            best, j = x, s
    return j


def importance_step(t_loc, t_scale, p_loc, p_scale, S, seed, normal, alpha, gumbel):
    _, _, w = R.importance_step(t_loc, t_scale, p_loc, p_scale, S, seed, normal)
    j = select(w, gumbel(seed, S), alpha)
    x = np.asarray(normal(seed, S * t_loc.size), dtype=f32).reshape(S, t_loc.size)
    with np.errstate(all="ignore"):
        return j, (p_scale * x[j] + p_loc).astype(f32), w


def encode_block(mq, sq, mp, sp, seed, S, K, normal, alpha, gumbel=reference_gumbel, ratio=R.power_law):
    """gc_referee.encode_block with the perturbed selection -> (max(K, 1) indices, sample)."""
    ql, qs, pl, ps = (np.asarray(v, f32).reshape(-1).copy() for v in (mq, sq, mp, sp))
    idx = []
    with np.errstate(all="ignore"):
        for i in range(K - 1, 0, -1):
            cv, tv = ps * ps, qs * qs
            a = (f32(ratio(i)) * cv).astype(f32)
            ta_loc = ((ql - pl) * a / cv).astype(f32)
            ta_scale = np.sqrt((tv * (a * a) / (cv * cv) + a * (cv - a) / cv).astype(f32))
            j, A, _ = importance_step(ta_loc, ta_scale, np.zeros_like(pl), np.sqrt(a), S, seed, normal, alpha, gumbel)
            idx.append(int(j))
            seed += 1
            nql = (pl + (A * tv * cv + (ql - pl) * (cv - a) * cv) / (tv * a + cv * (cv - a))).astype(f32)
            nqs = np.sqrt((tv * cv * (cv - a) / (a * tv + cv * (cv - a))).astype(f32))
            ql, qs, pl, ps = nql, nqs, (pl + A).astype(f32), np.sqrt((cv - a).astype(f32))
        j, z, _ = importance_step(ql, qs, pl, ps, S, seed, normal, alpha, gumbel)
    idx.append(int(j))
    return idx, z


def encode_tensor(q_loc, q_scale, p_loc, p_scale, seed, S, omega, block_size, oracle, alpha, gumbel=reference_gumbel):
    """gc_referee.encode_tensor at finite alpha: split, every block with the same seed, merge."""
    shape = np.shape(q_loc)
    flat = [np.asarray(v, f32).reshape(-1) for v in (q_loc, q_scale, p_loc, p_scale)]
    n = flat[0].size
    bs = n if block_size is None else block_size
    perm = oracle.tf_shuffle_perm(seed, n) if block_size is not None else np.arange(n)
    out, sample = [], np.empty(n, f32)
    for start in range(0, n, bs):
        at = perm[start:start + bs]
        blk = [v[at] for v in flat]
        K = oracle.num_aux(oracle.block_kl(*blk), omega)
        idx, z = encode_block(*blk, seed, S, K, oracle.tf_random_normal, alpha, gumbel)
        out.append(idx)
        sample[at] = z
    return out, sample.reshape(shape)
