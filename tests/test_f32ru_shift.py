"""CPU: the predicted, decimated row shift of the certified f32 round-up first pass
(tools/probe_f32ru.py forward(every=K), DESIGN.md "Certified f32 round-up first pass").

The shift of row t is a per-sequence prediction dhat of the drift per step; the row maximum is
taken at the steps t with (t - 1) % K == 0 only, where it corrects the row and the prediction, and
the shift is folded into the emission term: v_t = RU(m + RU(b'' - mu_t)).  Any shift is valid, so
test_f32ru_model.py's exact-rational check of the invariant v_t[j] + C_t + R_t >= d_t[j] applies
unchanged; here it runs for K = 1, 4, 8 at the lengths round a block of K steps, on models with
-inf entries, on sequences whose prefix is infeasible (a measured step then reads a row of -inf
alone), and on exact f64 ties.
"""
import importlib.util
import os

import numpy as np
import pytest

import np_oracle as NO
import test_f32ru_model as TM

M = TM.M
F32 = np.float32
NINF = F32(-np.inf)

_spec = importlib.util.spec_from_file_location(
    "probe_fixed_first",
    os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "probe_fixed_first.py"))
FX = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(FX)

KS = [1, 4, 8]


def _lengths(K):
    return sorted({1, 2, 3, K, K + 1, K + 2, 2 * K + 1})


def test_default_is_an_instantiated_k():
    assert M.EVERY in KS


@pytest.mark.parametrize("inf_frac", [0.0, 0.3])
@pytest.mark.parametrize("K", KS)
def test_invariant_and_certified_results(K, inf_frac):
    ncert = ninfeasible = 0
    for T in _lengths(K):
        for seed in range(3):
            n, v = 3 + (seed + T) % 6, 3 + seed % 3
            pi, a, b = TM._model(n, v, 3000 + 37 * T + seed, inf_frac, (1.0, 1e-5, 1.0)[seed])
            b[:, v - 1] = -np.inf  # the last observation is impossible: sequence 5 ends in it
            rng = np.random.default_rng(seed + 10 * T)
            obs = rng.integers(0, v - 1, size=(6, T))
            obs[5, T - 1] = v - 1
            path, cert, score, parts = M.decode(pi, a, b, obs, every=K)
            assert not np.isnan(parts["rows"]).any() and not np.isnan(parts["mu"]).any()
            assert not (parts["rows"] == np.inf).any() and np.isfinite(parts["mu"]).all()
            assert (np.abs(parts["dhat"]) < 64).all()
            # the steps between two measured ones shift by the prediction alone
            for t in range(1, T):
                if (t - 1) % K:
                    assert np.array_equal(parts["mu"][:, t], parts["dhat"][:, t]), (K, T, t)
            with np.errstate(invalid="ignore"):  # its margin is NaN beside -inf entries; the path is not
                p64 = FX.decode64(pi, a, b, obs)[0]
            for s in range(obs.shape[0]):
                rp, rs, rst = NO.decode(pi, a, b, obs[s].astype(np.int32))
                TM._check_invariant(pi, a, b, obs[s], parts["tb"], parts["rows"][:, s, :], parts["mu"][s])
                if rst != NO.SEQ_OK:
                    ninfeasible += 1
                    assert not cert[s], (K, T, seed, s)
                if cert[s]:
                    ncert += 1
                    assert rst == NO.SEQ_OK and np.array_equal(rp, path[s]), (K, T, seed, s)
                    assert np.float64(score[s]).view(np.uint64) == np.float64(rs).view(np.uint64), (K, T, seed, s)
                    assert np.array_equal(p64[s], path[s]), (K, T, seed, s)
    assert ncert > 0 and ninfeasible >= 3 * len(_lengths(K))


@pytest.mark.parametrize("K", KS)
def test_every_values_agree_on_what_certifies_and_differ_in_rows(K):
    """The shift cancels in the bookkeeping: another K gives other rows and shifts, and the paths
    of the sequences both certify are the f64 decode's in both."""
    pi, a, b = TM._model(8, 4, 5, 0.0)
    obs = np.random.default_rng(5).integers(0, 4, size=(6, 2 * 8 + 1))
    p1, c1, s1, q1 = M.decode(pi, a, b, obs, every=K)
    p2, c2, s2, q2 = M.decode(pi, a, b, obs, every=2 if K == 1 else K // 2)
    both = c1 & c2
    assert both.any() and np.array_equal(p1[both], p2[both]) and np.array_equal(s1[both], s2[both])
    assert not np.array_equal(q1["mu"], q2["mu"])


@pytest.mark.parametrize("K", KS)
def test_infeasible_prefix_across_a_measured_step(K):
    """Rows of -inf alone from step 0 on, from step K on (the row a measured step reads, after the
    prediction has a value) and from step K + 1 on: no NaN or +inf in rows, mu or dhat, the
    prediction returns to 0, and the sequence does not certify."""
    n, v, T = 5, 3, 2 * K + 3
    pi, a, b = TM._model(n, v, 9, 0.0)
    b[:, 2] = -np.inf
    rng = np.random.default_rng(K)
    obs = rng.integers(0, 2, size=(4, T))
    obs[0, 0] = 2
    obs[1, K] = 2
    obs[2, K + 1] = 2
    path, cert, score, parts = M.decode(pi, a, b, obs, every=K)
    for x in (parts["rows"], parts["mu"], parts["dhat"]):
        assert not np.isnan(x).any() and not (x == np.inf).any()
    assert np.isfinite(parts["mu"]).all() and (np.abs(parts["dhat"]) < 64).all()
    assert (parts["rows"][:, 0] == NINF).all()
    assert (parts["rows"][K:, 1] == NINF).all() and (parts["rows"][K + 1:, 2] == NINF).all()
    assert np.isfinite(parts["rows"][:, 3]).all()
    # the measured steps that read a row of -inf alone: the clamp is the shift, the prediction is 0
    for s, t in ((0, 1), (0, K + 1), (1, K + 1), (2, 2 * K + 1)):
        assert parts["mu"][s, t] == M.MRAW_MIN and parts["dhat"][s, t] == 0, (s, t)
    assert not cert[:3].any()
    for s in range(3):
        TM._check_invariant(pi, a, b, obs[s], parts["tb"], parts["rows"][:, s, :], parts["mu"][s])


def test_predictor_update_guards():
    """shift_update: exact scaling, a tiny maximum counts 0, and the result is 0 wherever it would
    leave (-64, 64) or is not finite."""
    for K in KS:
        d = np.array([0.0, 0.5, -0.5, 63.0, -63.0, 1.0, 0.25, 0.0, 0.0], F32)
        m = np.array([1.0, -0.25, 0.75, 8.0 * K, -8.0 * K, 2.0 ** -65, -(2.0 ** -64), float(M.MRAW_MIN), -0.0], F32)
        got = M.shift_update(d, m, K)
        want = [1.0 / K, 0.5 - 0.25 / K, -0.5 + 0.75 / K, 0.0, 0.0, 1.0, None, 0.0, 0.0]
        for g, w, di, mi in zip(got, want, d, m):
            if w is None:  # 0.25 - 2^-64 / K, rounded up: 0.25
                assert g == F32(0.25), (K, di, mi, g)
            else:
                assert g == F32(w), (K, di, mi, g)
        assert got.dtype == F32 and not np.isnan(got).any()
    assert M.shift_update(np.array([np.nan, np.inf, -np.inf], F32), np.zeros(3, F32), 4).tolist() == [0.0, 0.0, 0.0]


@pytest.mark.parametrize("K", KS)
def test_exact_ties_never_certify(K):
    for seed in range(8):
        n, v, T = 3 + seed % 6, 3, (2, 3, K, K + 1, K + 2, 2 * K + 1, 2 * K + 2, 3 * K)[seed]
        pi, a, b = TM._model(n, v, 77 + seed, 0.0)
        a[1, :] = a[0, :]
        a[:, 1] = a[:, 0]
        b[1, :] = b[0, :]
        pi[1] = pi[0]
        a[:, :2] = np.log10(0.45)
        b[:2, :] = np.log10(0.9)
        obs = np.random.default_rng(seed).integers(0, v, size=(4, max(T, 2)))
        _, cert, _, _ = M.decode(pi, a, b, obs, every=K)
        assert not cert.any(), (K, seed)
