#!/usr/bin/env python3
"""Writes tests/golden/posterior_*.npz: reference log-likelihoods and posterior marginals of
small HMMs in 60-digit arithmetic (mpmath), for tests/test_posterior.py and
tests/test_gpu_posterior.py (which only load the files; they do not need mpmath).

Each fixture holds the model (pi, a, b: log10 f64, -inf = 0; the reference takes p = 10^x of
exactly these doubles), the sequences (offsets, obs), forced tags (forced: -1 = free) and, for
the free run and for the run with the tags (suffix _f):
  loglik[B]          log10 sum_s P(o, s)            (-inf if the likelihood is 0)
  gamma[sum T, N]    P(s_t = j | o)                  rounded to f64
  S[B]               sum_t |log10 c_t|, c_t the per-step normalisers (loglik = sum_t log10 c_t)

    python tools/make_posterior_golden.py [fixture names ...]
"""
from __future__ import annotations

import os
import sys

import numpy as np
from mpmath import mp, mpf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
mp.dps = 60


def random_model(rng, n, v, zero_frac=0.1):
    """log10 of row-stochastic tables with ~zero_frac zeros (every row keeps a positive entry)."""
    def rows(r, c):
        p = rng.gamma(1.0, 1.0, size=(r, c))
        z = rng.random((r, c)) < zero_frac
        z[np.arange(r), rng.integers(0, c, size=r)] = False
        p[z] = 0.0
        return p / p.sum(axis=1, keepdims=True)

    with np.errstate(divide="ignore"):
        return np.log10(rows(1, n)[0]), np.log10(rows(n, n)), np.log10(rows(n, v))


def viterbi_path(pi, a, b, obs):
    d = pi + b[:, obs[0]]
    back = []
    for o in obs[1:]:
        m = d[:, None] + a
        back.append(m.argmax(axis=0))
        d = m.max(axis=0) + b[:, o]
    path = [int(d.argmax())]
    for bk in reversed(back):
        path.append(int(bk[path[-1]]))
    return path[::-1], float(d.max())


def mp_tables(pi, a, b):
    p10 = lambda x: mpf(0) if x == -np.inf else mp.power(10, mpf(float(x)))
    n, v = b.shape
    return ([p10(x) for x in pi], [[p10(a[i, j]) for j in range(n)] for i in range(n)],
            [[p10(b[i, o]) for o in range(v)] for i in range(n)])


def mp_forward_backward(P, A, B, obs, forced):
    """Exact (60-digit) normalised forward-backward: (loglik, gamma[T][N], S)."""
    n, T = len(P), len(obs)
    ok = lambda t, j: forced[t] < 0 or forced[t] == j
    alphas, cs = [], []
    prev = None
    for t in range(T):
        o = obs[t]
        if t == 0:
            y = [P[j] * B[j][o] if ok(t, j) else mpf(0) for j in range(n)]
        else:
            y = [sum(prev[i] * A[i][j] for i in range(n)) * B[j][o] if ok(t, j) else mpf(0) for j in range(n)]
        c = sum(y)
        if c == 0:
            return -np.inf, np.zeros((T, n)), np.inf
        prev = [x / c for x in y]
        alphas.append(prev)
        cs.append(c)
    beta = [mpf(1)] * n
    gamma = np.zeros((T, n))
    for t in range(T - 1, -1, -1):
        g = [alphas[t][j] * beta[j] for j in range(n)]
        s = sum(g)
        gamma[t] = [float(x / s) for x in g]
        if t > 0:
            u = [B[j][obs[t]] * beta[j] if ok(t, j) else mpf(0) for j in range(n)]
            w = [sum(A[i][j] * u[j] for j in range(n)) for i in range(n)]
            m = max(w)
            beta = [x / m for x in w]
    logs = [mp.log10(c) for c in cs]
    return float(sum(logs)), gamma, float(sum(abs(x) for x in logs))


def make(name, n, v, lengths, seed, tag_frac=0.3, zero_frac=0.1):
    rng = np.random.default_rng(seed)
    pi, a, b = random_model(rng, n, v, zero_frac)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    obs = np.zeros(int(offsets[-1]), np.int32)
    forced = np.full(int(offsets[-1]), -1, np.int32)
    for k, T in enumerate(lengths):  # observations with a feasible path; tags taken from it
        lo = int(offsets[k])
        while True:
            o = rng.integers(0, v, size=T)
            path, score = viterbi_path(pi, a, b, o)
            if score > -np.inf:
                break
        obs[lo:lo + T] = o
        tagged = rng.random(T) < tag_frac
        forced[lo:lo + T][tagged] = np.asarray(path, np.int32)[tagged]
    P, A, B = mp_tables(pi, a, b)
    out = dict(pi=pi, a=a, b=b, offsets=offsets, obs=obs, forced=forced)
    for suffix, frc in (("", np.full_like(forced, -1)), ("_f", forced)):
        ll, gm, S = [], [], []
        for k, T in enumerate(lengths):
            lo = int(offsets[k])
            l1, g1, s1 = mp_forward_backward(P, A, B, obs[lo:lo + T].tolist(), frc[lo:lo + T].tolist())
            ll.append(l1)
            gm.append(g1)
            S.append(s1)
        out["loglik" + suffix] = np.asarray(ll)
        out["gamma" + suffix] = np.concatenate(gm, axis=0)
        out["S" + suffix] = np.asarray(S)
    path = os.path.join(GOLDEN, name)
    np.savez_compressed(path, **out)
    print(f"{name}: N={n} V={v} lengths={list(lengths)} loglik={out['loglik']} ({os.path.getsize(path)} bytes)")


FIXTURES = {
    "posterior_n3.npz": dict(n=3, v=4, lengths=[12, 1, 2, 5], seed=301),
    "posterior_n17.npz": dict(n=17, v=5, lengths=[33, 1, 7], seed=317),
    "posterior_n64.npz": dict(n=64, v=6, lengths=[33, 2], seed=364),
    "posterior_n4_long.npz": dict(n=4, v=8, lengths=[2048], seed=304),
    "posterior_n4_t4096.npz": dict(n=4, v=8, lengths=[4096], seed=309),
    # beyond one column tile of the matrix-core kernels (NP = 192: 3 tiles, NP = 256: 4) and on the
    # plain kernels (N > 256); the two sparse models double as a zero-heavy case.  The seeds are
    # chosen so that the tags reach the later tiles (tests/test_posterior.py asserts it).
    "posterior_n130.npz": dict(n=130, v=5, lengths=[9, 1, 4], seed=3130, zero_frac=0.1),
    "posterior_n250.npz": dict(n=250, v=5, lengths=[8, 1, 3], seed=3250, zero_frac=0.75),
    "posterior_n300.npz": dict(n=300, v=4, lengths=[6, 1, 3], seed=3300, zero_frac=0.8),
}


def main(argv):
    """No argument: every fixture; else only the named ones (the others stay byte-identical)."""
    names = argv or list(FIXTURES)
    for name in names:
        if name not in FIXTURES:
            print(f"unknown fixture {name}; known: {' '.join(FIXTURES)}", file=sys.stderr)
            return 2
    for name in names:
        make(name, **FIXTURES[name])
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
