"""Reference for cv_expected_counts_model* (DESIGN.md "Emission counts"): a plain numpy f64
restatement -- the scaled forward-backward of counts_ref.np_counts under per-sequence weights, then
a scatter of the rows w_s gamma by observation -- the bound of include/cviterbi.h, and an
exhaustive enumeration of the state paths for tiny models, which shares nothing with the
recursions."""
import itertools

import numpy as np

U = 2.0 ** -53
SEQ_OK, SEQ_INFEASIBLE, SEQ_EMPTY, SEQ_BADOBS = 0, 1, 2, 3


def b_bound(T, N, L, b_abs, wmax=1.0):
    """|b_cnt - exact|: T the longest sequence of the call, L its elements, b_abs the statistic
    with |w_s|, wmax the largest |w_s|."""
    return (4 * T * (N + 8) + L + 1) * U * b_abs + 1e-290 * L * max(1.0, wmax)


def _tables(pi, a, b):
    with np.errstate(over="ignore"):
        return 10.0 ** np.asarray(pi, np.float64), 10.0 ** np.asarray(a, np.float64), 10.0 ** np.asarray(b, np.float64)


def _mask(forced, lo, T, N):
    mask = np.ones((T, N))
    if forced is not None:
        for t in np.nonzero(np.asarray(forced[lo:lo + T]) >= 0)[0]:
            mask[t] = 0.0
            mask[t, forced[lo + t]] = 1.0
    return mask


def np_model_counts(pi, a, b, off, obs, w=None, forced=None):
    """dict(pi, a, b: the weighted counts [N], [N, N], [N, V]; pi_abs, a_abs, b_abs: the same with
    |w_s|; g [L, N]: the rows w_s gamma (zeros for a sequence that is not OK); status [B]) over the
    sequences of positive likelihood.  Tables log10 (-inf = 0), forced -1 = free, w None = all 1."""
    P, A, Bm = _tables(pi, a, b)
    N, V, nseq = len(P), Bm.shape[1], len(off) - 1
    w = np.ones(nseq) if w is None else np.asarray(w, np.float64)
    obs = np.asarray(obs)
    pi_g, S, pi_abs, S_abs = np.zeros(N), np.zeros((N, N)), np.zeros(N), np.zeros((N, N))
    g, g_abs = np.zeros((len(obs), N)), np.zeros((len(obs), N))
    status = np.zeros(nseq, np.uint8)
    for s, (lo, hi) in enumerate(zip(off[:-1], off[1:])):
        o = obs[lo:hi]
        T = len(o)
        if T == 0:
            status[s] = SEQ_EMPTY
            continue
        if o.min() < 0 or o.max() >= V:
            status[s] = SEQ_BADOBS
            continue
        mask = _mask(forced, lo, T, N)
        alpha = np.zeros((T, N))
        for t in range(T):
            y = (P if t == 0 else alpha[t - 1] @ A) * Bm[:, o[t]] * mask[t]
            if not y.max() > 0:
                status[s] = SEQ_INFEASIBLE
                break
            alpha[t] = y / y.max()
        else:
            R, Us = np.zeros((T, N)), np.zeros((T, N))
            W = np.ones(N)
            for t in range(T - 1, -1, -1):
                rsum = alpha[t] @ W
                gamma = alpha[t] * W / rsum
                g[lo + t], g_abs[lo + t] = gamma * w[s], gamma * abs(w[s])
                if t == 0:
                    pi_g += gamma * w[s]
                    pi_abs += gamma * abs(w[s])
                if t < T - 1:
                    R[t] = alpha[t] / rsum
                if t > 0:
                    u = Bm[:, o[t]] * mask[t] * (W / W.max())
                    Us[t - 1] = u
                    W = A @ u
            X = R.T @ Us
            S += X * w[s]
            S_abs += X * abs(w[s])
    # the scatter by observation: rows of sequences that are not OK are zero and are left out
    b_g, b_abs = np.zeros((V, N)), np.zeros((V, N))
    ok_rows = np.repeat(status == SEQ_OK, np.diff(off))
    e0 = int(off[0])
    idx = np.nonzero(ok_rows)[0] + e0
    np.add.at(b_g, obs[idx], g[idx])
    np.add.at(b_abs, obs[idx], g_abs[idx])
    return dict(pi=pi_g, a=A * S, b=b_g.T.copy(), pi_abs=pi_abs, a_abs=A * S_abs, b_abs=b_abs.T.copy(), g=g,
                g_abs=g_abs, status=status)


def enumerate_model_counts(pi, a, b, off, obs, w=None, forced=None):
    """The same dict (without g_abs) and loglik [B] by summing over every state path: N^T terms
    per sequence, tiny models only."""
    P, A, Bm = _tables(pi, a, b)
    N, V, nseq = len(P), Bm.shape[1], len(off) - 1
    w = np.ones(nseq) if w is None else np.asarray(w, np.float64)
    obs = np.asarray(obs)
    out = dict(pi=np.zeros(N), a=np.zeros((N, N)), b=np.zeros((N, V)), pi_abs=np.zeros(N), a_abs=np.zeros((N, N)),
               b_abs=np.zeros((N, V)), g=np.zeros((len(obs), N)), status=np.zeros(nseq, np.uint8),
               loglik=np.full(nseq, -np.inf))
    for s, (lo, hi) in enumerate(zip(off[:-1], off[1:])):
        o = obs[lo:hi]
        T = len(o)
        if T == 0:
            out["status"][s] = SEQ_EMPTY
            continue
        if o.min() < 0 or o.max() >= V:
            out["status"][s] = SEQ_BADOBS
            continue
        mask = _mask(forced, lo, T, N)
        total = 0.0
        g0, xi, em, gm = np.zeros(N), np.zeros((N, N)), np.zeros((N, V)), np.zeros((T, N))
        for path in itertools.product(range(N), repeat=T):
            p = P[path[0]]
            for t in range(T):
                p *= Bm[path[t], o[t]] * mask[t, path[t]]
                if t > 0:
                    p *= A[path[t - 1], path[t]]
            if p == 0.0:
                continue
            total += p
            g0[path[0]] += p
            for t in range(T):
                em[path[t], o[t]] += p
                gm[t, path[t]] += p
                if t > 0:
                    xi[path[t - 1], path[t]] += p
        if not total > 0:
            out["status"][s] = SEQ_INFEASIBLE
            continue
        out["loglik"][s] = np.log10(total)
        for key, x in (("pi", g0), ("a", xi), ("b", em)):
            out[key] += x / total * w[s]
            out[key + "_abs"] += x / total * abs(w[s])
        out["g"][lo:hi] = gm / total * w[s]
    return out


def within(got, ref, bound):
    """Largest |got - ref| / bound (asserted <= 1 by the callers)."""
    return float(np.max(np.abs(got - ref) / bound)) if np.size(got) else 0.0
