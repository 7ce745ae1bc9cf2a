"""numpy referee of the sequential importance coder's arithmetic contract: GaussianCoder.encode_block /
decode_block over an ImportanceSampler at alpha = inf (rec/coding/coder.py:493-584, importance_sampling.py:9-103).

All float32, one rounding per operation in the reference's operator order; the weight of a sample is the float64 sum of its
float32 terms in dim order (np.cumsum), rounded once; log(ts) is the deterministic float64 log of csrc/irec_device.h restated
with the same operations and rounded to float32.  The standard-normal stream is the caller's (`normal(seed, count)`, e.g.
oracle.tf_random_normal).  Test infrastructure: shared by tests/test_gc_importance_host.py and tests/test_gc_importance_gpu.py.
"""
import numpy as np

f32 = np.float32
AUX_RATIO_POWER_LAW = -0.7864636765648174   # coder.py:16
HL2PI = f32(0.5 * np.log(2 * np.pi))
FLT_MAX = np.finfo(f32).max


def power_law(i):
    return f32(np.power(i + 1., AUX_RATIO_POWER_LAW))


def det_log(x):
    """csrc/irec_device.h det_log, operation by operation (float64 in, float64 out)."""
    x = np.array(x, dtype=np.float64, copy=True).reshape(-1)
    bits = x.view(np.uint64)
    e = ((bits >> np.uint64(52)) & np.uint64(0x7FF)).astype(np.int64)
    sub = e == 0
    if sub.any():
        x = np.where(sub, x * 18014398509481984.0, x)
        bits = x.view(np.uint64)
        e = np.where(sub, ((bits >> np.uint64(52)) & np.uint64(0x7FF)).astype(np.int64) - 54, e)
    e = e - 1023
    m = ((bits & np.uint64(0x000FFFFFFFFFFFFF)) | np.uint64(0x3FF0000000000000)).view(np.float64)
    big = m > 1.4142135623730951
    m = np.where(big, m * 0.5, m)
    e = e + big
    s = (m - 1.0) / (m + 1.0)
    s2 = s * s
    q = np.full_like(s, 1.0 / 25.0)
    for k in (23, 21, 19, 17, 15, 13, 11, 9, 7, 5, 3):
        q = q * s2 + 1.0 / k
    return e.astype(np.float64) * 0.6931471805599453 + (2.0 * s + (2.0 * s) * (s2 * q))


def importance_step(t_loc, t_scale, p_loc, p_scale, S, seed, normal):
    """encode_gaussian_importance_sample -> (index, sample, weights)."""
    with np.errstate(all="ignore"):
        n = t_loc.size
        x = np.asarray(normal(seed, S * n), dtype=f32).reshape(S, n)
        tl = ((t_loc - p_loc) / p_scale).astype(f32)
        ts = (t_scale / p_scale).astype(f32)
        c = (HL2PI + det_log(ts.astype(np.float64)).astype(f32)).astype(f32)
        e = (x / ts - tl / ts).astype(f32)
        lt = (f32(-0.5) * (e * e) - c).astype(f32)
        lp = (f32(-0.5) * (x * x) - (HL2PI + f32(0))).astype(f32)
        term = (lt - lp).astype(f32)
        w = np.cumsum(term.astype(np.float64), axis=1)[:, -1].astype(f32)     # dim order, rounded once
        best, j = -FLT_MAX, 0
        for s, v in enumerate(w):           # accumulator starts at (0, -FLT_MAX), strict ">": a NaN is never chosen
            if v > best:
                best, j = v, s
        return j, (p_scale * x[j] + p_loc).astype(f32), w


def encode_block(mq, sq, mp, sp, seed, S, K, normal, ratio=power_law, weights=None):
    """-> (max(K, 1) indices, sample).  K = ceil(KL / Omega) is the caller's.  `weights`: a list that receives every step's w."""
    ql, qs, pl, ps = (np.asarray(v, f32).reshape(-1).copy() for v in (mq, sq, mp, sp))
    idx = []
    with np.errstate(all="ignore"):
        for i in range(K - 1, 0, -1):
            cv, tv = ps * ps, qs * qs
            a = (f32(ratio(i)) * cv).astype(f32)
            ta_loc = ((ql - pl) * a / cv).astype(f32)
            ta_scale = np.sqrt((tv * (a * a) / (cv * cv) + a * (cv - a) / cv).astype(f32))
            j, A, w = importance_step(ta_loc, ta_scale, np.zeros_like(pl), np.sqrt(a), S, seed, normal)
            idx.append(int(j))
            if weights is not None:
                weights.append(w)
            seed += 1
            nql = (pl + (A * tv * cv + (ql - pl) * (cv - a) * cv) / (tv * a + cv * (cv - a))).astype(f32)
            nqs = np.sqrt((tv * cv * (cv - a) / (a * tv + cv * (cv - a))).astype(f32))
            ql, qs, pl, ps = nql, nqs, (pl + A).astype(f32), np.sqrt((cv - a).astype(f32))
        j, z, w = importance_step(ql, qs, pl, ps, S, seed, normal)
    idx.append(int(j))
    if weights is not None:
        weights.append(w)
    return idx, z


def decode_block(mp, sp, indices, seed, S, normal, ratio=power_law):
    pl, ps = (np.asarray(v, f32).reshape(-1).copy() for v in (mp, sp))
    n, K = pl.size, len(indices)
    with np.errstate(all="ignore"):
        for t in range(K - 1):
            cv = ps * ps
            a = (f32(ratio(K - 1 - t)) * cv).astype(f32)
            x = np.asarray(normal(seed + t, S * n), dtype=f32).reshape(S, n)[indices[t]]
            A = (np.sqrt(a) * x + f32(0)).astype(f32)
            pl, ps = (pl + A).astype(f32), np.sqrt((cv - a).astype(f32))
        x = np.asarray(normal(seed + K - 1, S * n), dtype=f32).reshape(S, n)[indices[K - 1]]
        return (ps * x + pl).astype(f32)


def encode_tensor(q_loc, q_scale, p_loc, p_scale, seed, S, omega, block_size, oracle, ratio=power_law):
    """GaussianCoder.encode of one tensor (coder.py:412-457): split, every block with the same seed, merge.
    -> (indices per block, merged sample of the input's shape).  K from the oracle's canonical block KL."""
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
        idx, z = encode_block(*blk, seed, S, K, oracle.tf_random_normal, ratio)
        out.append(idx)
        sample[at] = z
    return out, sample.reshape(shape)
