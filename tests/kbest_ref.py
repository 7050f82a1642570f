"""The K-best (list) Viterbi specification in numpy f64 (include/cviterbi.h, cv_kbest_batch),
implemented literally, plus the fold of a path and an exhaustive enumeration for tiny models.
No GPU; helpers of tests/test_kbest.py and tests/test_gpu_kbest.py."""
import itertools

import numpy as np

NINF = -np.inf


def fold_score(pi, a, b, obs, path):
    """The reference's fold along a path: d = pi + b, then d = (d + a) + b (f64)."""
    d = np.float64(pi[path[0]]) + np.float64(b[path[0], obs[0]])
    for t in range(1, len(obs)):
        d = (d + np.float64(a[path[t - 1], path[t]])) + np.float64(b[path[t], obs[t]])
    return d


def kbest_ref(pi, a, b, obs, K, forced=None):
    """(paths int32[K, T] (-1 unused), scores f64[K] (-inf unused), count) of one sequence.
    Per (t, j): one stable descending sort of the candidates at index i * K + r, the first K
    finite ones kept, then the emission added."""
    pi, a, b = np.asarray(pi, np.float64), np.asarray(a, np.float64), np.asarray(b, np.float64)
    T, N = len(obs), len(pi)
    paths = np.full((K, T), -1, np.int32)
    scores = np.full(K, NINF)
    if T == 0:
        return paths, scores, 0
    if forced is None:
        forced = np.full(T, -1)
    lists = np.full((N, K), NINF)  # L_t(j)[r], -inf = no entry
    back = np.zeros((T, N, K), np.int64)  # flattened i * K + r
    with np.errstate(invalid="ignore"):
        for j in range(N):
            if forced[0] < 0 or forced[0] == j:
                lists[j, 0] = pi[j] + b[j, obs[0]]
        for t in range(1, T):
            new = np.full((N, K), NINF)
            flat = lists.reshape(-1)
            for j in range(N):
                if forced[t] >= 0 and forced[t] != j:
                    continue
                x = flat + np.repeat(a[:, j], K)
                order = np.argsort(-x, kind="stable")
                order = order[np.isfinite(x[order])][:K]
                new[j, :len(order)] = x[order] + b[j, obs[t]]
                back[t, j, :len(order)] = order
            lists = new
    flat = lists.reshape(-1)
    order = np.argsort(-flat, kind="stable")
    order = order[np.isfinite(flat[order])][:K]
    for rank, idx in enumerate(order):
        scores[rank] = flat[idx]
        for t in range(T - 1, -1, -1):
            paths[rank, t] = idx // K
            idx = back[t, idx // K, idx % K]
    return paths, scores, len(order)


def brute_force(pi, a, b, obs, forced=None):
    """Every path of finite score, by enumeration (N^T <= 4,096): (scores descending, paths)."""
    T, N = len(obs), len(pi)
    assert N ** T <= 4096
    out = []
    for path in itertools.product(range(N), repeat=T):
        if forced is not None and any(f >= 0 and f != s for f, s in zip(forced, path)):
            continue
        d = fold_score(pi, a, b, obs, path)
        if np.isfinite(d):
            out.append((d, path))
    out.sort(key=lambda e: -e[0])
    return np.array([e[0] for e in out], np.float64), [e[1] for e in out]


def quantised_model(n, v, seed, inf_arcs=False):
    """Log-probability-like tables quantised to multiples of 1/4 (abundant exact ties: sums of
    such values are exact in f64); inf_arcs: ~30% -inf arcs and ~20% -inf emissions too."""
    rng = np.random.default_rng(seed)
    pi = -rng.integers(0, 8, size=n) / 4.0
    a = -rng.integers(0, 8, size=(n, n)) / 4.0
    b = -rng.integers(0, 8, size=(n, v)) / 4.0
    if inf_arcs:
        a[rng.random((n, n)) < 0.3] = NINF
        b[rng.random((n, v)) < 0.2] = NINF
    return pi, a, b


def random_logprobs(n, v, seed):
    """log10 of random row-stochastic tables (generic: no ties)."""
    rng = np.random.default_rng(seed)

    def rows(r, c):
        p = rng.gamma(1.0, 1.0, size=(r, c))
        return np.log10(p / p.sum(axis=1, keepdims=True))

    return rows(1, n)[0], rows(n, n), rows(n, v)
