#!/usr/bin/env python3
"""Writes tests/golden/counts_*.npz: the expected initial and transition counts of the posterior
fixtures in 60-digit arithmetic (mpmath), for tests/test_counts.py and tests/test_gpu_counts.py
(which only load the files; they do not need mpmath).

Reads tests/golden/posterior_*.npz and posterior_emis_n{3,17,64}.npz (model, sequences, tags; it
does not rewrite them) and writes counts_<the same name>.npz with, for the free run and for the
run with the tags (suffix _f), over all sequences of the fixture:
  pi_cnt[N]      sum_s P(s_0 = i | o)
  a_cnt[N, N]    sum_s sum_t P(s_t = i, s_t+1 = j | o)         rounded to f64

    python tools/make_counts_golden.py [posterior fixture names ...]
"""
from __future__ import annotations

import os
import sys

import numpy as np
from mpmath import mp, mpf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
mp.dps = 60

FIXTURES = ["posterior_n3.npz", "posterior_n17.npz", "posterior_n64.npz", "posterior_n4_long.npz",
            "posterior_n4_t4096.npz", "posterior_n130.npz", "posterior_n250.npz", "posterior_n300.npz",
            "posterior_emis_n3.npz", "posterior_emis_n17.npz", "posterior_emis_n64.npz"]


def p10(x):
    return mpf(0) if x == -np.inf else mp.power(10, mpf(float(x)))


def mp_counts(P, A, em, forced, pi_cnt, S):
    """Adds one sequence's gamma_0 to pi_cnt and sum_t xi_t / A to S (lists of mpf; S only where
    A is not 0).  em[t][j]: the emission probability of element t in state j."""
    n, T = len(P), len(em)
    ok = lambda t, j: forced[t] < 0 or forced[t] == j
    nz = [[j for j in range(n) if A[i][j] != 0] for i in range(n)]
    alphas, prev = [], None
    for t in range(T):
        if t == 0:
            y = [P[j] * em[t][j] if ok(t, j) else mpf(0) for j in range(n)]
        else:
            y = [mpf(0)] * n
            for i in range(n):
                if prev[i] != 0:
                    for j in nz[i]:
                        y[j] += prev[i] * A[i][j]
            y = [y[j] * em[t][j] if ok(t, j) else mpf(0) for j in range(n)]
        c = sum(y)
        assert c != 0, "the fixtures hold feasible sequences only"
        prev = [x / c for x in y]
        alphas.append(prev)
    beta = [mpf(1)] * n
    for t in range(T - 1, -1, -1):
        if t == 0:
            g = [alphas[0][j] * beta[j] for j in range(n)]
            s = sum(g)
            for j in range(n):
                pi_cnt[j] += g[j] / s
            break
        u = [em[t][j] * beta[j] if ok(t, j) else mpf(0) for j in range(n)]
        w = [sum(A[i][j] * u[j] for j in nz[i]) for i in range(n)]
        al = alphas[t - 1]
        d = sum(al[i] * w[i] for i in range(n))
        for i in range(n):
            if al[i] != 0:
                r = al[i] / d
                row = S[i]
                for j in nz[i]:
                    row[j] += r * u[j]
        m = max(w)
        beta = [x / m for x in w]


def make(name):
    z = np.load(os.path.join(GOLDEN, name))
    pi, a, off = z["pi"], z["a"], z["offsets"]
    n = len(pi)
    P = [p10(x) for x in pi]
    A = [[p10(a[i, j]) for j in range(n)] for i in range(n)]
    if "E" in z.files:  # dense emissions: row e of E is element e's scores
        em_of = lambda e: [p10(x) for x in z["E"][e, :n]]
    else:
        cols = {}
        b, obs = z["b"], z["obs"]

        def em_of(e):
            o = int(obs[e])
            if o not in cols:
                cols[o] = [p10(b[j, o]) for j in range(n)]
            return cols[o]
    out = {}
    for suffix, frc in (("", np.full_like(z["forced"], -1)), ("_f", z["forced"])):
        pi_cnt = [mpf(0)] * n
        S = [[mpf(0)] * n for _ in range(n)]
        for k in range(len(off) - 1):
            lo, hi = int(off[k]), int(off[k + 1])
            mp_counts(P, A, [em_of(e) for e in range(lo, hi)], frc[lo:hi].tolist(), pi_cnt, S)
        out["pi_cnt" + suffix] = np.array([float(x) for x in pi_cnt])
        out["a_cnt" + suffix] = np.array([[float(A[i][j] * S[i][j]) for j in range(n)] for i in range(n)])
    path = os.path.join(GOLDEN, "counts_" + name)
    np.savez_compressed(path, **out)
    print(f"counts_{name}: N={n} sum a_cnt={out['a_cnt'].sum():.12g} sum pi_cnt={out['pi_cnt'].sum():.12g} "
          f"({os.path.getsize(path)} bytes)")


def main(argv):
    """No argument: every fixture; else only the named ones (the others stay byte-identical)."""
    names = argv or FIXTURES
    for name in names:
        if name not in FIXTURES:
            print(f"unknown fixture {name}; known: {' '.join(FIXTURES)}", file=sys.stderr)
            return 2
    for name in names:
        make(name)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
