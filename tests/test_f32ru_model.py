"""CPU: the numpy model of the certified f32 round-up first pass (tools/probe_f32ru.py, DESIGN.md
"Certified f32 round-up first pass") against exact rational arithmetic.

  * the round-up add emulation is the exact RU of the real sum (`fractions`), on random and
    adversarial operand pairs: large exponent gaps, results that cross a binade, -inf, overflow;
  * the shifted tables are the exact RU of a - ca_j, b + ca_j - cb_o, pi - ca_j;
  * on small dense and sparse models (N = 3 .. 8, T <= 12, -inf entries, an infeasible sequence)
    the invariant v_t[j] + C_t + R_t >= d_t[j] holds for every entry, C_t summed exactly;
  * every certified path is the f64 first-argmax path and its fold is the f64 score bit for bit;
  * an exact tie (two identical states) never certifies.
"""
import importlib.util
import os
from fractions import Fraction

import numpy as np
import pytest

import np_oracle as NO

_spec = importlib.util.spec_from_file_location(
    "probe_f32ru", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "probe_f32ru.py"))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)

F32 = np.float32
NINF = F32(-np.inf)


def _model(n, v, seed, inf_frac, scale=1.0):
    rng = np.random.default_rng(seed)
    pi = np.log10(rng.dirichlet(np.ones(n))) * scale
    a = np.log10(rng.dirichlet(np.ones(n), size=n)) * scale
    b = np.log10(rng.dirichlet(np.ones(v), size=n)) * scale
    if inf_frac:
        a[rng.random((n, n)) < inf_frac] = -np.inf
        b[rng.random((n, v)) < inf_frac] = -np.inf
        pi[rng.random(n) < inf_frac] = -np.inf
    return pi, a, b


def _is_exact_ru(f, exact):
    """f (f32) is the smallest f32 >= exact (a Fraction); None stands for -inf."""
    if exact is None:
        return f == NINF
    if not np.isfinite(f) or Fraction(float(f)) < exact:
        return False
    with np.errstate(over="ignore"):
        below = np.nextafter(F32(f), NINF)
    return below == NINF or Fraction(float(below)) < exact


def _fr(x):
    return None if x == -np.inf else Fraction(float(x))


def _operand_pairs():
    rng = np.random.default_rng(2)
    n = 3000
    x = (rng.standard_normal(n) * 10.0 ** rng.uniform(-30, 30, n)).astype(F32)
    y = (rng.standard_normal(n) * 10.0 ** rng.uniform(-30, 30, n)).astype(F32)
    # near cancellation and binade crossings: y = -x (1 + k ulp), and sums just around powers of two
    k = rng.integers(-3, 4, n)
    xc = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)).astype(F32)
    yc = -xc
    for _ in range(3):
        yc = np.where(k > 0, np.nextafter(yc, F32(np.inf)), np.where(k < 0, np.nextafter(yc, NINF), yc))
    p2 = (2.0 ** rng.integers(-20, 20, n)).astype(F32)
    xb = np.nextafter(p2, NINF)
    yb = (p2 * F32(2.0) ** rng.integers(-60, -1, n).astype(F32)).astype(F32) * rng.choice([-1, 1], n).astype(F32)
    # huge gaps: one ulp-sized operand beside a large one, either sign (f64 cannot hold the sum)
    xg = (rng.standard_normal(n) * 1e20).astype(F32)
    yg = (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-44, -10, n)).astype(F32)
    edge = np.array([0.0, -0.0, 1.0, -1.0, -np.inf, M.FLT_MAX, -M.FLT_MAX, 1e-45, -1e-45, 2.0 ** -126, 1.0 + 2.0 ** -23],
                    F32)
    ex, ey = np.meshgrid(edge, edge)
    keep = ~((ex.ravel() == np.inf) | (ey.ravel() == np.inf))
    return (np.concatenate([x, xc, xb, xg, ex.ravel()[keep]]), np.concatenate([y, yc, yb, yg, ey.ravel()[keep]]))


def test_round_up_add_against_fractions():
    x, y = _operand_pairs()
    assert len(x) > 12000
    with np.errstate(over="ignore"):
        got = M.ru_add(x, y)
    assert got.dtype == F32
    inexact64 = 0
    for xi, yi, gi in zip(x, y, got):
        if xi == NINF or yi == NINF:
            assert gi == NINF
            continue
        exact = Fraction(float(xi)) + Fraction(float(yi))
        if exact > Fraction(float(M.FLT_MAX)):
            assert gi == np.inf
            continue
        assert _is_exact_ru(gi, exact), (xi, yi, gi)
        inexact64 += Fraction(float(xi) + float(yi)) != exact
    assert inexact64 > 500  # the two-sum branch is exercised


def test_round_up_differs_from_nearest():
    x, y = _operand_pairs()
    fin = np.isfinite(x) & np.isfinite(y)
    with np.errstate(over="ignore"):
        up, rn = M.ru_add(x[fin], y[fin]), M.rn_add(x[fin], y[fin])
    assert (up >= rn).all() and (up > rn).sum() > 1000


@pytest.mark.parametrize("inf_frac", [0.0, 0.3])
def test_table_shifts_against_fractions(inf_frac):
    for seed in range(6):
        n, v = 3 + seed, 3 + seed % 3
        pi, a, b = _model(n, v, 50 + seed, inf_frac, scale=(1.0, 1e-3, 40.0)[seed % 3])
        tb = M.tables(pi, a, b)
        ca, cb = tb["ca"], tb["cb"]
        assert np.array_equal(ca * 65536.0, np.rint(ca * 65536.0)) and np.array_equal(cb * 65536.0, np.rint(cb * 65536.0))
        for j in range(n):
            assert _is_exact_ru(tb["p1"][j], None if pi[j] == -np.inf else _fr(pi[j]) - _fr(ca[j])), (seed, j)
            for i in range(n):
                assert _is_exact_ru(tb["a1"][i, j], None if a[i, j] == -np.inf else _fr(a[i, j]) - _fr(ca[j])), (seed, i, j)
            for o in range(v):
                want = None if b[j, o] == -np.inf else _fr(b[j, o]) + _fr(ca[j]) - _fr(cb[o])
                assert _is_exact_ru(tb["b2"][j, o], want), (seed, j, o)


def _f64_rows(pi, a, b, obs):
    T = len(obs)
    d = np.empty((T, len(pi)))
    d[0] = pi + b[:, obs[0]]
    for t in range(1, T):
        d[t] = (d[t - 1][:, None] + a).max(axis=0) + b[:, obs[t]]
    return d


def _check_invariant(pi, a, b, obs, tb, rows, mu):
    """v_t[j] + C_t + R_t >= d_t[j] for every entry, in exact arithmetic; rows [T, N]."""
    T, N = rows.shape
    d64 = _f64_rows(pi, a, b, obs)
    w = sum(float(np.abs(m[np.isfinite(m)]).max()) if np.isfinite(m).any() else 0.0 for m in (pi, a, b))
    C = _fr(tb["cb"][obs[0]])
    for t in range(T):
        if t >= 1:
            C += _fr(tb["cb"][obs[t]]) + _fr(mu[t])
        R = Fraction(2.02) * Fraction(2) ** -53 * Fraction(w) * (t + 1) ** 2
        for j in range(N):
            x = _fr(d64[t, j])
            if x is None:
                continue
            assert rows[t, j] > NINF and _fr(rows[t, j]) + C + R >= x, (t, j)


@pytest.mark.parametrize("inf_frac", [0.0, 0.3])
@pytest.mark.parametrize("scale", [1.0, 1e-5])
def test_certificate_against_exact_arithmetic(inf_frac, scale):
    ncert = nfail = ninfeasible = 0
    for seed in range(36):
        n, v, T = 3 + seed % 6, 3 + seed % 3, 1 + seed % 12
        pi, a, b = _model(n, v, 1000 + seed, inf_frac, scale)
        b[:, v - 1] = -np.inf  # the last observation is impossible: sequence 5 ends in it
        rng = np.random.default_rng(seed)
        obs = rng.integers(0, v - 1, size=(6, T))
        obs[5, T - 1] = v - 1
        path, cert, score, parts = M.decode(pi, a, b, obs)
        for s in range(obs.shape[0]):
            rp, rs, rst = NO.decode(pi, a, b, obs[s].astype(np.int32))
            _check_invariant(pi, a, b, obs[s], parts["tb"], parts["rows"][:, s, :], parts["mu"][s])
            if rst != NO.SEQ_OK:
                ninfeasible += 1
                assert not cert[s], (seed, s)
            if cert[s]:
                ncert += 1
                assert rst == NO.SEQ_OK and np.array_equal(rp, path[s]), (seed, s)
                assert np.float64(score[s]).view(np.uint64) == np.float64(rs).view(np.uint64), (seed, s)
            else:
                nfail += 1
    assert ncert > 0 and ninfeasible >= 36
    if scale < 1.0:
        assert nfail > ninfeasible  # margins of 1e-5 decades and less do leave sequences uncertified


def test_exact_ties_never_certify():
    for seed in range(12):
        n, v, T = 3 + seed % 6, 3, 2 + seed % 11
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
        _, cert, _, _ = M.decode(pi, a, b, obs)
        assert not cert.any(), seed


def test_all_impossible_rows_stay_free_of_nan():
    """A row of -inf alone shifts by -FLT_MAX: later rows stay -inf, nothing certifies."""
    n, v, T = 5, 3, 6
    pi, a, b = _model(n, v, 9, 0.0)
    b[:, 2] = -np.inf
    obs = np.array([[0, 2, 1, 0, 1, 0], [2, 0, 0, 1, 1, 0]])
    path, cert, score, parts = M.decode(pi, a, b, obs)
    assert not np.isnan(parts["rows"]).any() and not np.isnan(parts["mu"]).any()
    assert (parts["rows"][-1] == NINF).all() and not cert.any()
