#!/usr/bin/env python3
"""Writes tests/golden/posterior_emis_*.npz: reference log-likelihoods and posterior marginals
under caller-supplied emission scores (cv_posterior_emissions*) in 60-digit arithmetic (mpmath),
for tests/test_posterior_emissions.py and tests/test_gpu_posterior_emissions.py (which only load
the files).  The reference is the substitution that defines the feature: the discrete model
b[j][e] = E[e][j] with obs[e] = e, through tools/make_posterior_golden.py's forward-backward.

Each fixture holds pi, a (log10 f64, -inf = 0), E [sum T, N] (log10 scores), offsets, forced
(-1 = free) and, for the free run and the run with the tags (suffix _f), loglik[B], S[B] and
gamma.  gamma_rows lists the elements whose gamma rows are stored (all of them except in the
long fixture, which keeps every 16th row to stay small).

    python tools/make_posterior_emissions_golden.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
from mpmath import mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_posterior_golden import GOLDEN, mp_forward_backward, mp_tables, random_model, viterbi_path  # noqa: E402

mp.dps = 60


def make(name, n, lengths, seed, draw, tag_frac=0.3, gamma_every=1, zero_frac=0.1):
    """draw(rng, T) -> E [T, n] of one sequence; redrawn until the sequence has a feasible path."""
    rng = np.random.default_rng(seed)
    pi, a, _ = random_model(rng, n, 2, zero_frac)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    total = int(offsets[-1])
    E = np.zeros((total, n))
    forced = np.full(total, -1, np.int32)
    for k, T in enumerate(lengths):
        lo = int(offsets[k])
        while True:
            e = draw(rng, T)
            path, score = viterbi_path(pi, a, e.T.copy(), np.arange(T))
            if score > -np.inf:
                break
        E[lo:lo + T] = e
        tagged = rng.random(T) < tag_frac
        forced[lo:lo + T][tagged] = np.asarray(path, np.int32)[tagged]
    rows = np.arange(0, total, gamma_every, dtype=np.int64)
    out = dict(pi=pi, a=a, E=E, offsets=offsets, forced=forced, gamma_rows=rows)
    for suffix, frc in (("", np.full_like(forced, -1)), ("_f", forced)):
        ll, gm, S = [], [], []
        for k, T in enumerate(lengths):
            lo = int(offsets[k])
            P, A, B = mp_tables(pi, a, E[lo:lo + T].T.copy())
            l1, g1, s1 = mp_forward_backward(P, A, B, list(range(T)), frc[lo:lo + T].tolist())
            ll.append(l1)
            gm.append(g1)
            S.append(s1)
        out["loglik" + suffix] = np.asarray(ll)
        out["gamma" + suffix] = np.concatenate(gm, axis=0)[rows]
        out["S" + suffix] = np.asarray(S)
    path = os.path.join(GOLDEN, name)
    np.savez_compressed(path, **out)
    print(f"{name}: N={n} lengths={list(lengths)} loglik={out['loglik']} ({os.path.getsize(path)} bytes)")


def main():
    # benign: probabilities between 10^-3 and 1
    make("posterior_emis_n3.npz", 3, [12, 1, 2, 5], 401, lambda rng, T: rng.uniform(-3.0, 0.0, size=(T, 3)))

    def mixed(rng, T):  # -inf entries, and a third of the rows densities up to 10^+40
        e = rng.normal(0.0, 3.0, size=(T, 17))
        up = rng.random(T) < 0.34
        e[up] += rng.uniform(20.0, 37.0, size=(int(up.sum()), 1))
        e = np.minimum(e, 40.0)
        e[rng.random(e.shape) < 0.15] = -np.inf
        return e

    make("posterior_emis_n17.npz", 17, [33, 1, 7], 417, mixed)
    # half of A zero and scores in multiples of 2^-10: the file stays below posterior_n64.npz
    make("posterior_emis_n64.npz", 64, [31, 2], 464,
         lambda rng, T: np.round(rng.normal(-2.0, 2.0, size=(T, 64)) * 1024.0) / 1024.0, zero_frac=0.5)
    # far outside what 10^x can represent: multiples of 1/8 in [-5200, -4800].  A row spans at
    # most 250 decades: an entry more than 300 decades below the largest of its own row is outside
    # the accuracy contract (it is staged as a subnormal or as 0, and where the transitions leave
    # such a state as the only way on, gamma of the exact model is not what any f64 row can give)
    def deep(rng, T):
        centre = rng.integers(-5075 * 8, -4925 * 8 + 1, size=(T, 1))
        return (centre + rng.integers(-125 * 8, 125 * 8 + 1, size=(T, 4))) / 8.0

    make("posterior_emis_n4_t4096.npz", 4, [4096], 409, deep, gamma_every=16)
    return 0


if __name__ == "__main__":
    sys.exit(main())
