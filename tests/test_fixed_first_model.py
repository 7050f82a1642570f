"""CPU: the numpy model of the certified fixed-point first pass (tools/probe_fixed_first.py,
DESIGN.md "Certified fixed-point first pass") against exact rational arithmetic.

On small random models (N <= 8, T <= 12, with and without -inf arcs) and at a coarse step q, so
that certificates do fail:
  * the error bound the certificate rests on holds in exact arithmetic (`fractions`): along a
    certified path |v_t[p_t] q + shift_t - d64_t[p_t]| <= E_t, and every other entry of every row
    is no lower than its f64 value minus E_t;
  * a certified path is the f64 oracle's path;
  * forced exact ties never certify;
  * the extreme tables (every entry at the floor, or at 0) stay inside int32;
  * the tables round-trip: |x~ q - x| <= q/2 above the floor.
"""
import importlib.util
import os
from fractions import Fraction

import numpy as np
import pytest

import np_oracle as NO

_spec = importlib.util.spec_from_file_location(
    "probe_fixed_first", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools",
                                      "probe_fixed_first.py"))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)


def _model(n, v, seed, inf_frac):
    rng = np.random.default_rng(seed)
    pi = np.log10(rng.dirichlet(np.ones(n)))
    a = np.log10(rng.dirichlet(np.ones(n), size=n))
    b = np.log10(rng.dirichlet(np.ones(v), size=n))
    if inf_frac:
        a[rng.random((n, n)) < inf_frac] = -np.inf
        b[rng.random((n, v)) < inf_frac] = -np.inf
        pi[rng.random(n) < inf_frac] = -np.inf
    return pi, a, b


def _f64_rows(pi, a, b, obs):
    T = len(obs)
    d = np.empty((T, len(pi)))
    d[0] = pi + b[:, obs[0]]
    for t in range(1, T):
        d[t] = (d[t - 1][:, None] + a).max(axis=0) + b[:, obs[t]]
    return d


def _frac(x):
    return None if x == -np.inf else Fraction(float(x))


def _check_bounds(pi, a, b, obs, qlog2, floor, path, cert, rows):
    """The induction of DESIGN.md in exact arithmetic for one sequence (rows [T, N] int)."""
    T, N = rows.shape
    q = Fraction(2) ** qlog2
    d64 = _f64_rows(pi, a, b, obs)
    g = M.rounding_gain(pi, a, b, qlog2)
    shift = Fraction(0)  # sum of the subtracted row maxima, in real units
    for t in range(T):
        if t >= 1:
            shift += int(rows[t - 1].max()) * q
        # E_t / q <= (t + 1) + g (t + 1)^2: quantisation of t + 1 table pairs plus the f64 rounding
        E = (Fraction(t + 1) + Fraction(g) * (t + 1) ** 2) * q
        for j in range(N):
            x = _frac(d64[t, j])
            if x is None:
                continue
            assert int(rows[t, j]) * q + shift >= x - E, (t, j)  # never an under-estimate
        if cert:
            x = _frac(d64[t, path[t]])
            assert x is not None and rows[t, path[t]] > floor
            assert abs(int(rows[t, path[t]]) * q + shift - x) <= E, (t, "two-sided on the path")


@pytest.mark.parametrize("inf_frac", [0.0, 0.25])
@pytest.mark.parametrize("qlog2", [-6, -10, -26])
def test_certificate_against_exact_arithmetic(inf_frac, qlog2):
    floor = -(1 << 30)
    ncert = nfail = 0
    for seed in range(40):
        n, v, T = 2 + seed % 7, 3 + seed % 3, 1 + seed % 12
        pi, a, b = _model(n, v, 1000 * -qlog2 + seed, inf_frac)
        rng = np.random.default_rng(seed)
        obs = rng.integers(0, v, size=(6, T))
        path, cert, rows = M.decode(pi, a, b, obs, qlog2, floor)
        for s in range(obs.shape[0]):
            rp, _, rst = NO.decode(pi, a, b, obs[s].astype(np.int32))
            _check_bounds(pi, a, b, obs[s], qlog2, floor, path[s], bool(cert[s]), rows[:, s, :])
            if cert[s]:
                ncert += 1
                assert rst == NO.SEQ_OK and np.array_equal(rp, path[s]), (seed, s)
            else:
                nfail += 1
    assert ncert > 0
    if qlog2 == -6:
        assert nfail > 0  # the coarse step does leave sequences uncertified


@pytest.mark.parametrize("qlog2", [-6, -26])
def test_exact_ties_never_certify(qlog2):
    for seed in range(12):
        n, v, T = 3 + seed % 5, 3, 2 + seed % 9
        pi, a, b = _model(n, v, 77 + seed, 0.0)
        # states 0 and 1 identical: every path through one has an exact twin through the other
        a[1, :] = a[0, :]
        a[:, 1] = a[:, 0]
        b[1, :] = b[0, :]
        pi[1] = pi[0]
        # ... and they dominate, so the best path runs through them
        a[:, :2] = np.log10(0.45)
        b[:2, :] = np.log10(0.9)
        rng = np.random.default_rng(seed)
        obs = rng.integers(0, v, size=(4, T))
        _, cert, _ = M.decode(pi, a, b, obs, qlog2)
        assert not cert.any(), seed


def test_extreme_tables_stay_inside_int32():
    n, v, T = 8, 3, 12
    obs = np.zeros((2, T), np.int64)
    for fill in (-np.inf, -1e300, -16.0, 0.0):
        pi, a, b = np.full(n, fill), np.full((n, n), fill), np.full((n, v), fill)
        path, cert, rows = M.decode(pi, a, b, obs)  # forward() and backtrack() assert the int32 range
        assert rows.min() >= M.FLOOR and rows.max() <= 0
        assert not cert.any()  # all at the floor, or all tied
    # mixed: one column at 0, the rest at the floor
    a = np.full((n, n), -np.inf)
    a[:, 3] = 0.0
    pi, b = np.zeros(n), np.zeros((n, v))
    path, cert, rows = M.decode(pi, a, b, obs)
    assert rows.min() >= M.FLOOR and rows.max() <= 0


def test_tables_round_trip():
    rng = np.random.default_rng(5)
    x = np.concatenate([-rng.random(1000) * 15.9, -10.0 ** rng.uniform(-12, 1.2, 1000), [0.0, -np.inf, -16.0, -17.0, -1e9]])
    xq = M.quantise(x)
    q = 2.0 ** M.QLOG2
    assert xq.min() >= M.FLOOR and xq.max() <= 0
    above = xq > M.FLOOR
    assert above.sum() > 1900 and not above[-4:].any()
    err = [abs(Fraction(int(k)) * Fraction(q) - Fraction(float(v))) for k, v in zip(xq[above], x[above])]
    assert max(err) <= Fraction(q) / 2
    # at the floor the image is an upper bound
    assert all(v <= M.FLOOR * q for v in x[~above])
