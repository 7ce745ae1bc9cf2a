"""Independent referee of the auxiliary-variance ratio fit: GaussianCoder.update_block_auxiliary_variance_ratios
(rec/coding/coder.py:266-410) restated in PyTorch float64 on the CPU.  Test infrastructure, shared by tests/test_ratio_fit_host.py
and tests/test_ratio_fit_gpu.py; no test functions.

What it shares with the code under test: nothing but the input data (the statistics and the table of standard normals).
  * the reference's literal formulas: get_auxiliary_target / get_auxiliary_coder (coder.py:141-154), TFP 0.9's KL of two Normals
    (0.5 squared_difference(la / sb, lb / sb) + 0.5 expm1(2 (log sa - log sb)) - (log sa - log sb)) and the tf.where losses
    (coder.py:360-367) -- not the closed form of DESIGN.md §3;
  * the gradient comes from torch.autograd, the optimiser step is theta - learning_rate * gradient (tf.optimizers.SGD);
  * libm log / exp / sigmoid and torch's own reductions, float64 throughout.
The state the reference keeps in float32 stays float32, in its operator order: the two state arrays and their running average
(coder.py:385-389), and the statistics tensors with the conditional target / coder that replace them (coder.py:157-171, :390-408).
The auxiliary sample is x * scale + loc (tfd.Normal.sample) with x read from the caller's table of standard normals.

For every fit step the referee also reports the STOP MARGIN | |prev - L| - relative_tolerance | at the stopping iteration and at
the one before: a comparison is meaningful only where float64 rounding cannot move the stop (the tests assert > 1e-9).

`mistake` plants one deliberate error (tests/test_ratio_fit_host.py checks that each one fails the comparison):
  "grad_sign"     the remaining-KL term enters the gradient with the wrong sign
  "stop_early"    the step yields sigmoid(theta) AFTER its last update instead of the ratio its last iteration evaluated (what a
                  stop test moved in front of the update amounts to once the ratio is read back from the parameter; moving the
                  test alone is not observable: same evaluated ratio, same iteration count)
  "rho_last"      the conditional target / coder are built from the step's own ratio instead of the averaged one
  "ceil"          partition counts by ceil(KL / Omega) instead of 1 + floor(KL / Omega)
"""
import numpy as np
import torch

f32 = np.float32


def sigmoid_inverse(x):
    """coder.py:19-24 in float64."""
    x = min(max(float(x), 1e-10), 1. - 1e-10)
    return float(np.log(x) - np.log(1. - x))


def kl_normal(la, sa, lb, sb):
    """tfp.distributions.normal._kl_normal_normal (TFP 0.9)."""
    diff_log_scale = torch.log(sa) - torch.log(sb)
    return 0.5 * (la / sb - lb / sb) ** 2 + 0.5 * torch.expm1(2. * diff_log_scale) - diff_log_scale


def _t(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


def total_kl(mq, sq, mp, sp):
    return kl_normal(_t(mq), _t(sq), _t(mp), _t(sp)).sum(dim=1)


def partition_counts(mq, sq, mp, sp, omega, mistake=None):
    kl = total_kl(mq, sq, mp, sp).numpy().astype(f32)
    if mistake == "ceil":
        return kl, np.ceil(kl / f32(omega)).astype(np.int64)
    return kl, 1 + np.floor(kl / f32(omega)).astype(np.int64)       # coder.py:284, float32


def fit(mq, sq, mp, sp, omega, table, ratios=(1.,), counts=(1.,), relative_tolerance=1e-4, max_iters=10000, learning_rate=0.001,
        mistake=None):
    """-> dict(ratios, counts: float32 arrays; num: partition counts; iters, margin_stop, margin_prev: one entry per fit step).
    mq .. sp: float32 [rows, D].  table: float32 [steps, D, S_pad], entry [j, d, n] = the draw of row n, dim d at fit step j."""
    omega = f32(omega)
    tl, ts, cl, cs = (np.array(v, dtype=f32, copy=True) for v in (mq, sq, mp, sp))
    n_rows = tl.shape[0]
    kl0, num = partition_counts(tl, ts, cl, cs, omega, mistake)
    if not np.all(np.isfinite(kl0)):
        raise ValueError("infinite KL")
    M = int(num.max())
    ratios, counts = np.array(ratios, dtype=f32).reshape(-1), np.array(counts, dtype=f32).reshape(-1)
    if M > ratios.size:                                                                   # coder.py:289-302
        ratios = np.concatenate([ratios, np.zeros(M - ratios.size, f32)])
        counts = np.concatenate([counts, np.zeros(M - counts.size, f32)])
    iters, margin_stop, margin_prev = [], [], []
    om = float(omega)
    for ratio in range(M, 1, -1):
        j = M - ratio
        rows = np.nonzero(num >= ratio)[0]                                                 # coder.py:308
        n_el = rows.size
        t_loc, t_scale, c_loc, c_scale = (_t(v[rows]) for v in (tl, ts, cl, cs))
        total = kl_normal(t_loc, t_scale, c_loc, c_scale).sum(dim=1)                      # coder.py:321
        if ratios[ratio - 1] > 0.:                                                        # coder.py:324-329
            init = ratios[ratio - 1]
        elif ratio < M:
            init = ratios[ratio]
        else:
            init = f32(1. / ratio)
        theta = torch.tensor(sigmoid_inverse(init), dtype=torch.float64, requires_grad=True)
        prev, margins, rho_eval = float("inf"), [], None
        c_var, t_var = c_scale ** 2, t_scale ** 2
        rest = om * (ratio - 1)
        for it in range(int(max_iters)):
            rho = torch.sigmoid(theta)
            aux_var = rho * c_var
            at_loc = (t_loc - c_loc) * aux_var / c_var                                    # get_auxiliary_target, coder.py:147-154
            at_var = t_var * aux_var ** 2 / c_var ** 2 + aux_var * (c_var - aux_var) / c_var
            aux_kl = kl_normal(at_loc, torch.sqrt(at_var), torch.zeros_like(c_loc), torch.sqrt(aux_var)).sum(dim=1)
            aux_loss = torch.where(aux_kl > om, (aux_kl - om) ** 2, torch.zeros_like(aux_kl))
            rem_loss = torch.where(total - aux_kl > rest, ((total - aux_kl) - rest) ** 2, torch.zeros_like(aux_kl))
            loss = torch.mean(aux_loss + rem_loss)
            objective = torch.mean(aux_loss - rem_loss) if mistake == "grad_sign" else loss
            grad, = torch.autograd.grad(objective, theta)
            rho_eval = float(rho.detach())
            with torch.no_grad():
                theta -= learning_rate * grad
            L = float(loss.detach())
            margins.append(abs(abs(prev - L) - relative_tolerance))
            if abs(prev - L) < relative_tolerance:                                        # coder.py:373-376
                break
            prev = L
        iters.append(it + 1)
        stopped_by_test = it + 1 < int(max_iters) or abs(prev - L) < relative_tolerance
        margin_stop.append(margins[-1] if stopped_by_test else float("inf"))
        margin_prev.append(margins[-2] if len(margins) > 1 and stopped_by_test else float("inf"))
        r_last = f32(float(torch.sigmoid(theta))) if mistake == "stop_early" else f32(rho_eval)
        # coder.py:385-389, float32
        ratios[ratio - 1] = (ratios[ratio - 1] * counts[ratio - 1] + r_last * f32(n_el)) / (counts[ratio - 1] + f32(n_el))
        counts[ratio - 1] = counts[ratio - 1] + f32(n_el)
        # coder.py:390-408, float32: the sample of aux_target (built from the step's own ratio), then the conditionals
        q_l, q_s, p_l, p_s = tl[rows], ts[rows], cl[rows], cs[rows]
        with np.errstate(all="ignore"):
            cv, tv = p_s * p_s, q_s * q_s
            a_last = r_last * cv
            loc = (q_l - p_l) * a_last / cv
            scale = np.sqrt(tv * (a_last * a_last) / (cv * cv) + a_last * (cv - a_last) / cv)
            x = np.asarray(table[j], dtype=f32)[:, rows].T                               # [n_el, D]
            A = x * scale + loc
            a = (r_last if mistake == "rho_last" else ratios[ratio - 1]) * cv
            new_q_l = p_l + (A * tv * cv + (q_l - p_l) * (cv - a) * cv) / (tv * a + cv * (cv - a))
            new_q_s = np.sqrt(tv * cv * (cv - a) / (a * tv + cv * (cv - a)))
            tl[rows], ts[rows], cl[rows], cs[rows] = new_q_l, new_q_s, p_l + A, np.sqrt(cv - a)
    return {"ratios": ratios, "counts": counts, "num": num, "kl": kl0, "iters": iters, "margin_stop": margin_stop,
            "margin_prev": margin_prev}
