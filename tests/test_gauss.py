"""Gaussian emissions without a device: the exports and argument errors of cv_gauss_emissions* and
cv_expected_counts_gauss* (checked before any device work), the tuning key, reestimate_gauss, and
the references of tests/gauss_ref.py against 60-digit arithmetic and against path enumeration."""
import ctypes

import numpy as np
import pytest

import cviterbi as cv
import gauss_ref as G
from cviterbi import _lib as L

NEW = ["cv_gauss_emissions", "cv_gauss_emissions_device", "cv_expected_counts_gauss", "cv_expected_counts_gauss_device"]


def _model(n=3, d=2, seed=0):
    rng = np.random.default_rng(seed)
    pi = np.log10(rng.dirichlet(np.ones(n)))
    a = np.log10(rng.dirichlet(np.ones(n), size=n))
    mean = rng.normal(size=(n, d))
    var = rng.uniform(0.5, 2.0, size=(n, d))
    return pi, a, mean, var


def test_exports_and_python_names():
    lib = L.lib()
    for name in NEW:
        assert name in cv.EXPORTS and hasattr(lib, name), name
    for name in ("gauss_hmm", "gauss_emissions", "gauss_emissions_device", "expected_counts_gauss",
                 "expected_counts_gauss_device", "reestimate_gauss", "fit_gauss"):
        assert callable(getattr(cv, name)), name
    h = cv.gauss_hmm(*_model()[:2])
    assert h.nstates() == 3 and h.nobs() == 1


def test_gm_part_rows_is_a_tuning_key():
    assert "gm_part_rows" in cv.tuning_keys()
    h = cv.gauss_hmm(*_model()[:2])
    assert h.tuning("gm_part_rows") == 0
    h.set_tuning(gm_part_rows=7)
    assert h.tuning("gm_part_rows") == 7


def _p(x):
    return None if x is None else x.ctypes.data_as(ctypes.c_void_p)


def _call_emis(h, x, ldx, D, mean, var, out, ld, nrows=4):
    return L.lib().cv_gauss_emissions(h.handle, nrows, _p(x), ldx, D, _p(mean), _p(var), _p(out), ld)


def _call_emis_dev(h, x, ldx, D, mean, var, out, ld, nrows=4):
    # host addresses stand in for the device pointers: the argument errors come before any device work
    return L.lib().cv_gauss_emissions_device(h.handle, nrows, _p(x), ldx, D, _p(mean), _p(var), None, _p(out), ld)


def _call_counts(h, x, ldx, D, mean, var, outs=None, device=False):
    n = h.nstates()
    off = np.array([0, 4], np.int64)
    o = dict(ll=np.zeros(1), pi=np.zeros(n), a=np.zeros((n, n)), g=np.zeros(n), m1=np.zeros((n, max(D, 1))),
             m2=np.zeros((n, max(D, 1))), st=np.zeros(1, np.uint8))
    o.update(outs or {})
    lib = L.lib()
    if device:
        return lib.cv_expected_counts_gauss_device(h.handle, 1, _p(off), _p(off), _p(x), ldx, D, _p(mean), _p(var), None,
                                                   None, None, _p(o["ll"]), _p(o["pi"]), _p(o["a"]), _p(o["g"]),
                                                   _p(o["m1"]), _p(o["m2"]), None, _p(o["st"]))
    return lib.cv_expected_counts_gauss(h.handle, 1, _p(off), _p(x), ldx, D, _p(mean), _p(var), None, None, None,
                                        _p(o["ll"]), _p(o["pi"]), _p(o["a"]), _p(o["g"]), _p(o["m1"]), _p(o["m2"]), None,
                                        _p(o["st"]))


def _bad_params(mean, var):
    """(name, mean, var) for every parameter value the header rejects."""
    out = []
    for name, v in (("mean nan", np.nan), ("mean +inf", np.inf), ("mean -inf", -np.inf)):
        m = mean.copy()
        m[1, 0] = v
        out.append((name, m, var))
    for name, v in (("var nan", np.nan), ("var 0", 0.0), ("var negative", -1.0), ("var below 1e-300", 9e-301),
                    ("var above 1e300", 1.1e300), ("var inf", np.inf)):
        s = var.copy()
        s[2, 1] = v
        out.append((name, mean, s))
    return out


@pytest.mark.parametrize("call", [_call_emis, _call_emis_dev], ids=["host", "device"])
def test_gauss_emissions_argument_errors(call):
    pi, a, mean, var = _model()
    h = cv.gauss_hmm(pi, a)
    x, out = np.zeros((4, 2)), np.zeros((4, 3))
    EINVAL, ELIMIT = L.CV_EINVAL, L.CV_ELIMIT
    assert call(h, None, 2, 2, mean, var, out, 3) == EINVAL
    assert call(h, x, 2, 2, None, var, out, 3) == EINVAL
    assert call(h, x, 2, 2, mean, None, out, 3) == EINVAL
    assert call(h, x, 2, 2, mean, var, None, 3) == EINVAL
    assert call(h, x, 1, 2, mean, var, out, 3) == EINVAL  # ldx < D
    assert call(h, x, 2, 2, mean, var, out, 2) == EINVAL  # ld < N
    assert call(h, x, 2, 0, mean, var, out, 3) == EINVAL  # D < 1
    assert call(h, x, 2, -3, mean, var, out, 3) == EINVAL
    big_m, big_v = np.zeros((3, 1025)), np.ones((3, 1025))
    assert call(h, np.zeros((4, 1025)), 1025, 1025, big_m, big_v, out, 3) == ELIMIT  # D > 1024
    for name, m, s in _bad_params(mean, var):
        assert call(h, x, 2, 2, m, s, out, 3) == EINVAL, name
    # the two ends of the variance range are inside it (no device here: the call gets past its checks)
    s = var.copy()
    s[0, 0], s[0, 1] = 1e-300, 1e300
    assert call(h, x, 2, 2, mean, s, out, 3, nrows=0) == L.CV_OK


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_expected_counts_gauss_argument_errors(device):
    pi, a, mean, var = _model()
    h = cv.gauss_hmm(pi, a)
    x = np.zeros((4, 2))
    EINVAL, ELIMIT = L.CV_EINVAL, L.CV_ELIMIT
    call = lambda *args, **kw: _call_counts(h, *args, device=device, **kw)  # noqa: E731
    assert call(None, 2, 2, mean, var) == EINVAL
    assert call(x, 2, 2, None, var) == EINVAL
    assert call(x, 2, 2, mean, None) == EINVAL
    assert call(x, 1, 2, mean, var) == EINVAL
    assert call(x, 2, 0, mean, var) == EINVAL
    assert call(np.zeros((4, 1025)), 1025, 1025, np.zeros((3, 1025)), np.ones((3, 1025))) == ELIMIT
    for name, m, s in _bad_params(mean, var):
        assert call(x, 2, 2, m, s) == EINVAL, name

    class Null:  # an output the call must have
        ctypes = type("c", (), {"data_as": staticmethod(lambda t: None)})

    for key in ("pi", "a", "g", "m1", "m2"):
        assert call(x, 2, 2, mean, var, outs={key: Null}) == EINVAL, key


def test_reestimate_gauss_rules():
    g = np.array([2.0, 0.0, 4.0, -1.0])
    m1 = np.array([[2.0, 4.0], [1.0, 1.0], [4.0, 0.0], [1.0, 1.0]])
    m2 = np.array([[10.0, 8.0], [1.0, 1.0], [4.0, 8.0], [1.0, 1.0]])
    mean_prev, var_prev = np.full((4, 2), 7.0), np.full((4, 2), 3.0)
    center = np.array([100.0, -100.0])
    mean, var = cv.reestimate_gauss(g, m1, m2, center, mean_prev, var_prev, var_floor=0.5)
    np.testing.assert_array_equal(mean[0], [101.0, -98.0])  # center + m1 / g
    np.testing.assert_array_equal(var[0], [4.0, 0.5])  # 10 / 2 - 1 = 4; 8 / 2 - 4 = 0 -> the floor
    np.testing.assert_array_equal(mean[2], [101.0, -100.0])
    np.testing.assert_array_equal(var[2], [0.5, 2.0])  # 4 / 4 - 1 = 0 -> the floor; 8 / 4 - 0 = 2
    for dead in (1, 3):  # g <= 0: the previous row
        np.testing.assert_array_equal(mean[dead], mean_prev[dead])
        np.testing.assert_array_equal(var[dead], var_prev[dead])
    mean0, _ = cv.reestimate_gauss(g, m1, m2, None, mean_prev, var_prev)
    np.testing.assert_array_equal(mean0[0], [1.0, 2.0])  # no center: 0
    with pytest.raises(ValueError):
        cv.reestimate_gauss(g[:3], m1, m2, None, mean_prev, var_prev)


def _density_case(D, n, rows, offset, sigma, seed):
    rng = np.random.default_rng(seed)
    mean = offset + sigma * rng.normal(size=(n, D))
    var = (sigma * rng.uniform(0.5, 2.0, size=(n, D))) ** 2
    x = offset + sigma * 2.0 * rng.normal(size=(rows, D))
    return x, mean, var


@pytest.mark.parametrize("D,offset,sigma", [(1, 0.0, 1.0), (3, 0.0, 1.0), (17, 0.0, 1.0), (64, 0.0, 1.0),
                                            (3, 1e8, 1e3), (17, 1e8, 1e3), (3, 0.0, 1e-150), (17, 0.0, 1e-150)])
def test_reference_density_against_mpmath(D, offset, sigma):
    """The numpy restatement of the kernel's operation order is within the header's bound of
    60-digit arithmetic: plain shapes, an offset of 1e8 with sigma = 1e3 (where the expanded form
    x^2 - 2 x mean + mean^2 would lose every digit), and sigma = 1e-150."""
    x, mean, var = _density_case(D, 3, 4, offset, sigma, seed=D)
    E = G.np_density(x, mean, var)
    exact = G.mp_density(x, mean, var)
    ratio = G.within(E, exact, G.density_bound(x, mean, var, exact))
    print(f"D={D} offset={offset} sigma={sigma}: error / bound = {ratio:.3f}")
    assert ratio <= 1.0


def test_reference_density_rows():
    x, mean, var = _density_case(3, 4, 5, 0.0, 1.0, seed=1)
    x[1, 2], x[3, 0] = np.nan, np.inf
    E = G.np_density(x, mean, var)
    assert np.isnan(E[[1, 3]]).all() and np.isfinite(E[[0, 2, 4]]).all()
    x[4, 1] = 1e200  # q overflows: -inf, a legal score
    assert (G.np_density(x, mean, var)[4] == -np.inf).all()


@pytest.mark.parametrize("n,lens", [(2, (5, 1, 3)), (3, (4, 0, 2, 3))])
def test_reference_statistics_against_enumeration(n, lens):
    """np_gauss_counts against the sum over every state path: signed weights, a forced tag, a
    center; the tolerance is the header's bound."""
    pi, a, mean, var = _model(n, 2, seed=n)
    rng = np.random.default_rng(10 + n)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    x = rng.normal(size=(int(off[-1]), 2)) * 1.5 + 3.0
    w = rng.normal(size=len(lens))
    forced = np.full(int(off[-1]), -1, np.int32)
    forced[1] = 1
    center = x.mean(axis=0)
    E = G.np_density(x, mean, var)
    ref = G.np_gauss_counts(pi, a, E, off, x, w=w, forced=forced, center=center)
    enum = G.enumerate_gauss_counts(pi, a, E, off, x, w=w, forced=forced, center=center)
    np.testing.assert_array_equal(ref["status"], enum["status"])
    bg, b1, b2 = G.moment_bounds(off, n, ref, w)
    assert G.within(ref["g"], enum["g"], bg) <= 1.0
    assert G.within(ref["m1"], enum["m1"], b1) <= 1.0
    assert G.within(ref["m2"], enum["m2"], b2) <= 1.0
    # the tag is honoured and the moments are what the definition says
    assert np.all(enum["gamma"][1, [j for j in range(n) if j != 1]] == 0.0)
    y = x - center
    np.testing.assert_allclose(enum["m1"], enum["gamma"].T @ y, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(enum["g"], enum["gamma"].sum(axis=0), rtol=1e-12, atol=1e-14)
