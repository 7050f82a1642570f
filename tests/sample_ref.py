"""The posterior path sampler's specification in numpy (include/cviterbi.h, cv_sample_batch):
scaled forward rows as tests/test_posterior.np_forward_backward builds them, the pick rule, the
accuracy bound, and the interval check of a set of paths against a conditional CDF.  No GPU; a
plain helper of tests/test_sample.py and tests/test_gpu_sample.py, nothing here is collected."""
import numpy as np

import cviterbi as cv

U = 2.0 ** -53


def eps(T, N):
    """The accuracy contract: the picked i satisfies F_(i-1) - eps <= u <= F_i + eps."""
    return 4 * (T + 1) * (N + 8) * U


def prob_tables(pi, a, b, dtype=np.float64):
    """10^x of the log10 tables in f64 (-inf -> 0), then widened to dtype."""
    with np.errstate(over="ignore"):
        return tuple((10.0 ** np.asarray(x, np.float64)).astype(dtype) for x in (pi, a, b))


def forward_rows(P, A, B, obs, forced=None):
    """alpha^[T, N], each row scaled to sum 1, in the dtype of the tables; None: likelihood 0."""
    T, N = len(obs), len(P)
    alpha = np.zeros((T, N), P.dtype)
    for t in range(T):
        y = (P if t == 0 else alpha[t - 1] @ A) * B[:, obs[t]]
        if forced is not None and forced[t] >= 0:
            keep = y[forced[t]]
            y = np.zeros_like(y)
            y[forced[t]] = keep
        c = y.sum()
        if c == 0:
            return None
        alpha[t] = y / c
    return alpha


def pick(w, u):
    """The smallest i with w_i > 0 and c_i > u W (c = the sequential prefix sums); the largest i
    with w_i > 0 when rounding leaves none."""
    c = np.cumsum(w)
    ok = np.nonzero((w > 0) & (c > u * c[-1]))[0]
    return int(ok[0]) if len(ok) else int(np.nonzero(w > 0)[0][-1])


def sample_path(alpha, A, u, order=None):
    """One FFBS path from the rows alpha under the uniforms u[T].  order: a permutation in which
    the weights are summed (a deliberately different association); the pick is still by state."""
    T = len(alpha)
    path = np.zeros(T, np.int32)
    for t in range(T - 1, -1, -1):
        w = alpha[t] if t == T - 1 else alpha[t] * A[:, path[t + 1]]
        if order is None:
            path[t] = pick(w, u[t])
        else:  # prefix sums built from blocks summed in another order: same values up to rounding
            blocks = np.array_split(np.arange(len(w)), max(1, len(w) // 7))
            c = np.zeros(len(w))
            base = 0.0
            for blk in blocks:
                c[blk] = base + np.cumsum(w[blk])
                base = base + w[blk][::-1].sum()
            ok = np.nonzero((w > 0) & (c > u[t] * base))[0]
            path[t] = int(ok[0]) if len(ok) else int(np.nonzero(w > 0)[0][-1])
    return path


def uniforms(seed, S, r, T):
    return cv.sample.uniform(seed, S, r, np.arange(T, dtype=np.uint64))


def interval_ratio(alpha, A, paths, us):
    """paths[R, T] drawn under us[R, T]: every pick has a positive weight, and the largest
    distance of u outside [F_(i-1), F_i] over all picks, F the CDF of alpha / A (their dtype)
    conditioned on the path's own next state.  Returns that distance (0: every u inside)."""
    R, T = paths.shape
    rows = np.arange(R)
    worst = 0.0
    for t in range(T - 1, -1, -1):
        i = paths[:, t]
        assert np.all((i >= 0) & (i < alpha.shape[1])), (t, i)
        w = np.broadcast_to(alpha[t], (R, alpha.shape[1])) if t == T - 1 else alpha[t][None, :] * A[:, paths[:, t + 1]].T
        assert np.all(w[rows, i] > 0), ("a state of weight 0 was picked", t, i[w[rows, i] <= 0])
        c = np.cumsum(w, axis=1)
        F = c / c[:, -1:]
        hi = F[rows, i]
        lo = np.where(i > 0, F[rows, np.maximum(i - 1, 0)], 0.0)
        u = us[:, t]
        worst = max(worst, float(np.max(np.maximum(lo - u, u - hi))))
    return max(worst, 0.0)


def model_sequences(pi, a, b, lengths, seed):
    """Observations drawn from the model itself (so every sequence is feasible), concatenated."""
    P, A, B = prob_tables(pi, a, b)
    rng = np.random.default_rng(seed)
    out = []
    for T in lengths:
        o = np.zeros(T, np.int32)
        s = 0
        for t in range(T):
            p = P if t == 0 else A[s]
            s = rng.choice(len(P), p=p / p.sum())
            o[t] = rng.choice(B.shape[1], p=B[s] / B[s].sum())
        out.append(o)
    return np.concatenate(out) if out else np.zeros(0, np.int32)
