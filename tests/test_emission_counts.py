"""CPU: cv_expected_counts_model* -- the ABI surface, the numpy reference of tests/bcnt_ref.py
against an exhaustive enumeration of the state paths, the M-step reestimate_model and the argument
checks of cviterbi.autograd.discrete_loglik.  No GPU: the kernels are tested in
test_gpu_emission_counts.py."""
import ctypes

import numpy as np
import pytest

import cviterbi as cv
from cviterbi import _lib as L
from bcnt_ref import SEQ_INFEASIBLE, SEQ_OK, enumerate_model_counts, np_model_counts

NINF = -np.inf


def test_symbols_resolve_and_reject_a_null_handle():
    lib = L.lib()
    for name in ("cv_expected_counts_model", "cv_expected_counts_model_device"):
        assert name in L.EXPORTS
        assert getattr(lib, name) is not None
    nulls = [None] * 10
    assert lib.cv_expected_counts_model(None, 0, *nulls) == L.CV_EINVAL
    assert b"null handle" in lib.cv_last_error()
    assert lib.cv_expected_counts_model_device(None, 0, *nulls, None) == L.CV_EINVAL
    assert b"null handle" in lib.cv_last_error()
    assert "bcnt_part_rows" in cv.tuning_keys()
    for name in ("expected_counts_model", "expected_counts_model_device", "reestimate_model"):
        assert callable(getattr(cv, name))
    assert callable(cv.autograd.discrete_loglik)


EVAL_ENTRIES = ("cv_posterior_batch", "cv_sample_batch", "cv_posterior_emissions", "cv_expected_counts",
                "cv_expected_counts_emissions", "cv_loglik_grad_emissions", "cv_expected_counts_model")


@pytest.mark.parametrize("name", [e + twin for e in EVAL_ENTRIES for twin in ("", "_device")])
def test_every_evaluation_entry_rejects_a_null_handle(name):
    lib = L.lib()
    f = getattr(lib, name)
    lib.cv_hmm_set_tuning(None, None, 0)  # another message, so the entry's own is seen
    assert b"null handle" not in lib.cv_last_error()
    assert f(None, *[None if t is ctypes.c_void_p else 0 for t in f.argtypes[1:]]) == L.CV_EINVAL
    assert lib.cv_last_error() == b"null handle"


def tiny_model():
    """N = 3, V = 3 with a -inf entry in each of pi, A and b."""
    with np.errstate(divide="ignore"):
        pi = np.log10(np.array([0.5, 0.0, 0.5]))
        a = np.log10(np.array([[0.2, 0.3, 0.5], [0.0, 0.6, 0.4], [0.3, 0.3, 0.4]]))
        b = np.log10(np.array([[0.1, 0.9, 0.0], [0.3, 0.3, 0.4], [0.6, 0.2, 0.2]]))
    return pi, a, b


@pytest.mark.parametrize("weighted", [False, True])
def test_numpy_reference_equals_path_enumeration(weighted):
    pi, a, b = tiny_model()
    assert np.isinf(pi).any() and np.isinf(a).any() and np.isinf(b).any()
    lengths = [1, 2, 5, 5, 2, 0, 5]
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    rng = np.random.default_rng(12)
    obs = rng.integers(0, 3, size=int(off[-1])).astype(np.int32)
    obs[off[4]:off[5]] = (2, 2)   # state 0 cannot emit 2 and pi[1] = 0: still feasible through state 2
    obs[off[6]] = 2
    forced = np.full(len(obs), -1, np.int32)
    forced[off[2] + 3] = 1        # one tag inside a sequence of T = 5
    forced[off[6]] = 0            # b[0][2] = 0 under the tag: likelihood 0
    w = np.array([1.5, -2.0, 0.75, -0.5, 3.0, 9.0, -7.0]) if weighted else None
    ref = np_model_counts(pi, a, b, off, obs, w, forced)
    exact = enumerate_model_counts(pi, a, b, off, obs, w, forced)
    assert np.array_equal(ref["status"], exact["status"])
    assert list(ref["status"][:5]) == [SEQ_OK] * 5 and ref["status"][6] == SEQ_INFEASIBLE
    for key in ("pi", "a", "b", "g"):
        scale = np.abs(exact[key + "_abs"]) if key != "g" else np.abs(exact["g"])
        assert np.all(np.abs(ref[key] - exact[key]) <= 1e-12 * scale), key
        assert np.all(ref[key][scale == 0] == 0), key
    assert np.all(ref["b"][np.isinf(b)] == 0) and np.all(ref["a"][np.isinf(a)] == 0) and ref["pi"][1] == 0
    # the tag's element counts for its state alone
    e = off[2] + 3
    assert ref["g"][e, 1] != 0 and ref["g"][e, 0] == 0 and ref["g"][e, 2] == 0
    # mass: every element of an OK sequence adds its weight
    lens = np.diff(off)
    ww = np.ones(len(lens)) if w is None else w
    mass = float(np.sum((ww * lens)[ref["status"] == SEQ_OK]))
    assert abs(ref["b"].sum() - mass) <= 1e-12 * float(np.sum((np.abs(ww) * lens)))


def test_reestimate_model():
    rng = np.random.default_rng(3)
    N, V = 4, 6
    pi_cnt, a_cnt, b_cnt = rng.random(N), rng.random((N, N)), rng.random((N, V))
    b_cnt[1] = 0.0       # a state never visited
    b_cnt[2, 3] = 0.0    # a value never emitted by state 2
    a_cnt[3] = 0.0
    pi_prev, a_prev, b_prev = (np.log10(x / x.sum(axis=-1, keepdims=True))
                               for x in (rng.random(N), rng.random((N, N)), rng.random((N, V))))
    pi, a, b = cv.reestimate_model(pi_cnt, a_cnt, b_cnt, pi_prev, a_prev, b_prev)
    pi2, a2 = cv.reestimate(pi_cnt, a_cnt, pi_prev, a_prev)
    assert np.array_equal(pi, pi2) and np.array_equal(a, a2)
    assert b.shape == (N, V)
    assert np.allclose((10.0 ** b).sum(axis=1), 1.0, rtol=0, atol=1e-14)
    assert np.array_equal(b[1], b_prev[1]) and np.array_equal(a[3], a_prev[3])
    assert b[2, 3] == NINF and np.isfinite(np.delete(b[2], 3)).all()
    assert np.allclose(10.0 ** b[0], b_cnt[0] / b_cnt[0].sum(), rtol=1e-14, atol=0)
    for bad in (dict(b_cnt=b_cnt[:3]), dict(b_cnt=b_cnt.ravel()), dict(b_prev=b_prev[:, :5]), dict(a_cnt=a_cnt[:, :3]),
                dict(pi_prev=pi_prev[:3])):
        kw = dict(pi_cnt=pi_cnt, a_cnt=a_cnt, b_cnt=b_cnt, pi_prev=pi_prev, a_prev=a_prev, b_prev=b_prev)
        kw.update(bad)
        with pytest.raises(ValueError):
            cv.reestimate_model(**kw)


def test_discrete_loglik_rejects_bad_arguments_before_any_launch():
    torch = pytest.importorskip("torch")
    N, V = 3, 4
    obs = torch.zeros(5, dtype=torch.int32)
    off = [0, 2, 5]
    lp, la, lb = (torch.zeros(N, dtype=torch.float64), torch.zeros((N, N), dtype=torch.float64),
                  torch.zeros((N, V), dtype=torch.float64))
    f = cv.autograd.discrete_loglik
    cases = [
        (obs.to(torch.int64), off, lp, la, lb),            # obs dtype
        (obs.numpy(), off, lp, la, lb),                    # not a tensor
        (obs, off, lp.float(), la, lb),                    # f32 parameters
        (obs, off, lp, la, lb.float()),
        (obs, off, lp, la[:, :2], lb),                     # shapes
        (obs, off, lp, la, lb[:2]),
        (obs, off, lp, la, lb.reshape(-1)),
        (obs, off, lp, la, lb),                            # obs on the CPU
    ]
    for args in cases:
        with pytest.raises(ValueError):
            f(*args)
