"""Reference for cv_expected_counts*: a plain numpy f64 restatement of the algorithm (scaled
forward rows, R^T U over all elements, then the product with A) and the derived bounds of
include/cviterbi.h (DESIGN.md "Expected counts").  Beyond the 60-digit fixtures
(tools/make_counts_golden.py) the GPU tests compare against this at twice the bounds."""
import numpy as np

U = 2.0 ** -53


def a_bound(T, N, L, ref):
    """|a_cnt - exact| for a call whose longest sequence has T elements, L elements in all."""
    return (4 * T * (N + 8) + L + 8) * U * ref + 1e-290 * L


def pi_bound(T, N, B, ref):
    return (4 * T * (N + 8) + B) * U * ref + 1e-290 * B


def np_counts(pi, a, b, off, obs, forced=None):
    """(pi_cnt [N], a_cnt [N, N]) over the sequences of positive likelihood; tables log10
    (-inf = 0), forced -1 = free.  A sequence holding an observation outside b counts nothing."""
    with np.errstate(over="ignore"):
        P, A, B = 10.0 ** np.asarray(pi), 10.0 ** np.asarray(a), 10.0 ** np.asarray(b)
    N = len(P)
    pi_cnt, S = np.zeros(N), np.zeros((N, N))
    for lo, hi in zip(off[:-1], off[1:]):
        o = np.asarray(obs[lo:hi])
        T = len(o)
        if T == 0 or o.min() < 0 or o.max() >= B.shape[1]:
            continue
        mask = np.ones((T, N))
        if forced is not None:
            for t in np.nonzero(np.asarray(forced[lo:hi]) >= 0)[0]:
                mask[t] = 0.0
                mask[t, forced[lo + t]] = 1.0
        alpha = np.zeros((T, N))
        for t in range(T):
            y = (P if t == 0 else alpha[t - 1] @ A) * B[:, o[t]] * mask[t]
            if not y.max() > 0:
                break
            alpha[t] = y / y.max()
        else:
            R, Us = np.zeros((T, N)), np.zeros((T, N))
            W = np.ones(N)
            for t in range(T - 1, -1, -1):
                rsum = alpha[t] @ W
                if t == 0:
                    pi_cnt += alpha[0] * W / rsum
                if t < T - 1:
                    R[t] = alpha[t] / rsum
                if t > 0:
                    u = B[:, o[t]] * mask[t] * (W / W.max())
                    Us[t - 1] = u
                    W = A @ u
            S += R.T @ Us
    return pi_cnt, A * S


def within(got, ref, bound):
    """Largest |got - ref| / bound (asserted <= 1 by the callers)."""
    return float(np.max(np.abs(got - ref) / bound))
