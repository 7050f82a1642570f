"""Generates tests/golden/fit_*.npz: one and two iterations of the reference's tag-clamped
Baum-Welch (HMM::train, hmm/hmm.rs:69-190) in 60-digit arithmetic (mpmath), for
tests/test_fit.py (which only loads the files and does not need mpmath).

Written from hmm.rs and the docstring of oracle/fit_oracle.py, not from the oracle's code,
so the fixtures pin the oracle's semantics and measure its accuracy independently:

  alpha_0 = e_tag, else normalize(pi o b(o_0))                        hmm.rs:81-88
  alpha_t = e_tag, else normalize((alpha_{t-1} o b(o_t)) A)            hmm.rs:89-98 (as written:
                                                                       the emission BEFORE the arc)
  beta_{T-1} = e_tag, else ones                                        hmm.rs:106-109
  beta_t  = e_tag, else normalize(A (beta_{t+1} o b(o_{t+1})))         hmm.rs:110-120
  gamma_t = normalize(alpha_t o beta_t)                                hmm.rs:124-131
  xi_t    = normalize(A o (alpha_t (x) (b(o_{t+1}) o beta_{t+1})))     hmm.rs:134-142, over all N^2
  pi' = sum_seq gamma_0 / R;  A' = sum xi / sum_{t<T-1} gamma;  B'[., o] = sum_{o_t=o} gamma / sum gamma
                                                                       hmm.rs:144-172
  normalize(v) = v / sum(v), or the constant 1 / len(v) when the sum is EXACTLY 0
                                                                       hmm.rs:274-282, 306-317
  log: 0 -> -inf, else log10                                           hmm.rs:192-205

The inputs are f64 values taken exactly; a sum of non-negative terms is 0 at 60 digits only
when every term is 0, the same condition as in f64 (no product of the fixtures underflows:
every vector is renormalised each step and T <= 25).  x / 0 follows IEEE as the reference's
f64 does: 0 / 0 = NaN, x / 0 = +inf.

Each file holds the inputs (pi, a, b, offsets, obs, tags), the log10 results after 1 and 2
iterations rounded to f64 (pi1, a1, b1, pi2, a2, b2) and oracle_err[2]: the numpy oracle's
largest absolute error against them after 1 and 2 iterations, on the generating machine.

Run from the repository root:  python tests/golden/make_fit_golden.py
"""
import os
import sys

import numpy as np
from mpmath import mp, mpf

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fit_cases as FC  # noqa: E402
import fit_oracle as FO  # noqa: E402

mp.dps = 60
ZERO = mpf(0)
NAN, INF = mpf("nan"), mpf("inf")


def normalize(v):
    s = sum(v, ZERO)
    if s != 0:
        return [x / s for x in v]
    return [mpf(1) / len(v)] * len(v)


def div(x, d):
    if d != 0:
        return x / d
    return NAN if x == 0 else INF


def train_step(pi, a, b, offsets, obs, tags):
    """pi[N], a[N][N], b[N][V] lists of mpf -> the next (pi, a, b)."""
    n, nv = len(pi), len(b[0])
    rng = range(n)
    arcs = [[j for j in rng if a[i][j] != 0] for i in rng]   # the nonzero arcs out of i
    into = [[i for i in rng if a[i][j] != 0] for j in rng]   # ... and into j (zero terms left out)
    pi_num = [ZERO] * n
    a_den = [ZERO] * n
    b_den = [ZERO] * n
    xi_sum = [[ZERO] * n for _ in rng]
    b_num = [[ZERO] * nv for _ in rng]
    nseq = len(offsets) - 1
    for s in range(nseq):
        ob = [int(x) for x in obs[offsets[s]:offsets[s + 1]]]
        tg = [int(x) for x in tags[offsets[s]:offsets[s + 1]]]
        T = len(ob)

        def onehot(k):
            return [mpf(1) if i == k else ZERO for i in rng]

        al = [None] * T
        al[0] = onehot(tg[0]) if tg[0] >= 0 else normalize([pi[i] * b[i][ob[0]] for i in rng])
        for t in range(1, T):
            if tg[t] >= 0:
                al[t] = onehot(tg[t])
            else:
                x = [al[t - 1][i] * b[i][ob[t]] for i in rng]
                al[t] = normalize([sum((x[i] * a[i][j] for i in into[j]), ZERO) for j in rng])
        be = [None] * T
        be[T - 1] = onehot(tg[T - 1]) if tg[T - 1] >= 0 else [mpf(1)] * n
        for t in range(T - 2, -1, -1):
            if tg[t] >= 0:
                be[t] = onehot(tg[t])
            else:
                u = [be[t + 1][j] * b[j][ob[t + 1]] for j in rng]
                be[t] = normalize([sum((a[i][j] * u[j] for j in arcs[i]), ZERO) for i in rng])
        for t in range(T):
            g = normalize([al[t][i] * be[t][i] for i in rng])
            for i in rng:
                if t == 0:
                    pi_num[i] += g[i]
                if t < T - 1:
                    a_den[i] += g[i]
                b_den[i] += g[i]
                b_num[i][ob[t]] += g[i]
        for t in range(T - 1):
            u = [b[j][ob[t + 1]] * be[t + 1][j] for j in rng]
            m = {(i, j): u[j] * al[t][i] * a[i][j] for i in rng if al[t][i] != 0 for j in arcs[i] if u[j] != 0}
            tot = sum(m.values(), ZERO)
            if tot != 0:
                for (i, j), x in m.items():
                    xi_sum[i][j] += x / tot
            else:  # every one of the N^2 entries, zero arcs included (hmm.rs:311-312)
                for i in rng:
                    for j in rng:
                        xi_sum[i][j] += mpf(1) / (n * n)
    new_pi = [x / nseq for x in pi_num]
    new_a = [[div(xi_sum[i][j], a_den[i]) for j in rng] for i in rng]
    new_b = [[div(b_num[i][o], b_den[i]) for o in range(nv)] for i in rng]
    return new_pi, new_a, new_b


def log10_f64(x):
    def one(v):
        if mp.isnan(v):
            return np.nan
        if mp.isinf(v):
            return np.inf
        return -np.inf if v == 0 else float(mp.log10(v))
    return np.array([[one(v) for v in row] for row in x] if isinstance(x[0], list) else [one(v) for v in x])


def make(name, inputs):
    pi0, a0, b0, off, obs, tags = inputs
    pi = [mpf(float(x)) for x in pi0]
    a = [[mpf(float(x)) for x in row] for row in a0]
    b = [[mpf(float(x)) for x in row] for row in b0]
    out = {"pi": pi0, "a": a0, "b": b0, "offsets": np.asarray(off, np.int64), "obs": obs, "tags": tags}
    errs = []
    for it in (1, 2):
        pi, a, b = train_step(pi, a, b, [int(x) for x in off], obs, tags)
        gold = (log10_f64(pi), log10_f64(a), log10_f64(b))
        ref = FO.train(pi0, a0, b0, off, obs, tags, it, 0.0)[:3]
        FC.assert_params_match(ref, gold, atol=1e-9)
        errs.append(max(float(np.abs(r[np.isfinite(g)] - g[np.isfinite(g)]).max()) for r, g in zip(ref, gold)))
        for k, g in zip(("pi", "a", "b"), gold):
            out[f"{k}{it}"] = g
    out["oracle_err"] = np.array(errs)
    np.savez_compressed(os.path.join(HERE, name), **out)
    print(name, "steps", int(off[-1]), "fallbacks", FO.fallback_counts(*inputs), "oracle_err", errs)


if __name__ == "__main__":
    make("fit_dense_n5.npz", FC.dense(5, 4, 12, 20, seed=4105))
    make("fit_s1_n17.npz", FC.s1(17, 5, 20, 25, seed=4117))
    make("fit_s1_n70.npz", FC.s1(70, 6, 30, 25, seed=4170))
