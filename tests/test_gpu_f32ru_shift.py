"""GPU: the predicted, decimated row shift of the certified f32 round-up first pass (tuning key
t64_f32ru_mu_every, DESIGN.md "Certified f32 round-up first pass").

trellis_fwd2_f32ru<256, K> takes the row maximum at every K-th step only and shifts every row by a
per-sequence prediction of the drift.  For every K that has an instantiation (1, 4, 8):

  * rows, shifts, path, r_t and E from cv_f32ru_trace equal the numpy model with the same `every`
    (tools/probe_f32ru.py) bit for bit at the lengths round a block of K steps and at T = 37, at
    N = 256 and N = 240, for equal lengths, for a ragged batch whose pairs have different lengths
    (T < K included) and for a banded -inf model with infeasible prefixes;
  * a decode returns the f64 kernels' paths, score bits and statuses, the same under every value of
    the key, and last_first_pass_kind says the round-up pass ran;
  * a bad observation is reported in its own slot;
  * a value that has no instantiation behaves as the nearest one.
"""
import importlib.util
import os

import numpy as np
import pytest

import cviterbi as cv
from cviterbi import _lib as L
from cviterbi import synth

pytestmark = pytest.mark.gpu


def _tool(name):
    spec = importlib.util.spec_from_file_location(
        name, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


M = _tool("probe_f32ru")

V = 16
KS = [1, 4, 8]  # the instantiated K
NS = [256, 240]


def _lengths(K):
    return sorted({1, 2, 3, K, K + 1, K + 2, 2 * K + 1, 37})


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _same(got, ref, what):
    for x, y, name in zip(got, ref, ("path", "score", "status")):
        x, y = np.asarray(x), np.asarray(y)
        if name == "score":
            x, y = x.view(np.uint64), y.view(np.uint64)
        bad = np.nonzero(x != y)[0]
        assert bad.size == 0, f"{what}: {name} differs at {bad[:8]}"


@pytest.fixture(scope="module")
def models():
    return {n: synth.random_hmm(n, V, seed=100 + n) for n in NS}


@pytest.fixture(scope="module")
def modelled(models):
    """Per (n, T, K): the model's run on 4 sequences of length T, computed once."""
    cache = {}

    def get(n, T, K, S=4):
        if (n, T, K) not in cache:
            pi, a, b = models[n]
            obs = synth.iid_obs(V, S * T, seed=7 * n + T).reshape(S, T)
            tb = M.tables(pi, a, b)
            rows, mu = M.forward(tb, obs.astype(np.int64), every=K)
            path, r, E = M.backtrack(tb, rows)
            cache[(n, T, K)] = dict(obs=obs, rows=rows, mu=mu, path=path, r=r, E=E)
        return cache[(n, T, K)]

    return get


def _check_trace(got, c, what, S=None):
    S = S or c["obs"].shape[0]
    assert np.array_equal(_bits(got["rows"][:, :S]), _bits(c["rows"][:, :S])), what + ": rows"
    assert np.array_equal(_bits(got["mu"][:S, 1:]), _bits(c["mu"][:S, 1:])), what + ": mu"
    assert np.array_equal(got["path"][:S], c["path"][:S]), what + ": path"
    assert np.array_equal(_bits(got["r"][:S, 1:]), _bits(c["r"][:S, 1:])), what + ": r"
    assert np.array_equal(_bits(got["E"][:S]), _bits(c["E"][:S])), what + ": E"


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("K", KS)
def test_stored_values_equal_the_model_bit_for_bit(gpu, models, modelled, K, n):
    h = cv.HMM(*models[n])
    h.set_tuning(t64_f32ru_mu_every=K)
    for T in _lengths(K):
        c = modelled(n, T, K)
        for S in (2, 4):
            _check_trace(cv.f32ru_trace(h, c["obs"][:S]), c, f"K={K} N={n} T={T} S={S}", S)


def test_the_key_changes_rows_and_shifts(gpu, models, modelled):
    """K = 1, 4 and 8 are three kernels: from the second block on their shifts differ."""
    h = cv.HMM(*models[256])
    mus = []
    for K in KS:
        h.set_tuning(t64_f32ru_mu_every=K)
        mus.append(_bits(cv.f32ru_trace(h, modelled(256, 37, K)["obs"])["mu"]))
    assert not np.array_equal(mus[0], mus[1]) and not np.array_equal(mus[1], mus[2])


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("K", KS)
def test_ragged_pairs_equal_the_model(gpu, models, K, n):
    """One launch, 16 sequences: pairs of lengths 37, 2K + 1, K + 2, K + 1, K, 3, 2, 1 in a mixed
    order (lengths below K included for K > 1), each pair against the model at its own length."""
    pi, a, b = models[n]
    lens = [K + 1, 37, 1, K, 2 * K + 1, 2, K + 2, 3]
    lengths = np.repeat(lens, 2)
    off = synth.offsets_from_lengths(lengths)
    obs = synth.iid_obs(V, int(off[-1]), seed=31 * K + n)
    h = cv.HMM(pi, a, b)
    h.set_tuning(t64_f32ru_mu_every=K)
    got = cv.f32ru_trace_ragged(h, off, obs)
    tb = M.tables(pi, a, b)
    for p, T in enumerate(lens):
        s0, e0, e1 = 2 * p, int(off[2 * p]), int(off[2 * p + 2])
        o = obs[e0:e1].reshape(2, T).astype(np.int64)
        rows, mu = M.forward(tb, o, every=K)
        path, r, E = M.backtrack(tb, rows)
        what = f"K={K} N={n} pair {p} T={T}"
        assert np.array_equal(_bits(got["rows"][e0:e1].reshape(2, T, n)), _bits(rows.transpose(1, 0, 2))), what + ": rows"
        assert np.array_equal(_bits(got["mu"][e0:e1].reshape(2, T)[:, 1:]), _bits(mu[:, 1:])), what + ": mu"
        assert np.array_equal(got["path"][e0:e1].reshape(2, T), path), what + ": path"
        assert np.array_equal(_bits(got["r"][e0:e1].reshape(2, T)[:, 1:]), _bits(r[:, 1:])), what + ": r"
        assert np.array_equal(_bits(got["E"][s0:s0 + 2]), _bits(E)), what + ": E"


def _banded():
    n = 256
    pi, a, b = synth.random_hmm(n, 8, seed=13)
    i, j = np.indices((n, n))
    a[(j - i) % n > 3] = -np.inf
    rng = np.random.default_rng(13)
    b[rng.random((n, 8)) < 0.5] = -np.inf
    pi[::2] = -np.inf
    b[:, 7] = -np.inf
    return pi, a, b


@pytest.mark.parametrize("K", KS)
def test_banded_inf_model_with_infeasible_prefixes(gpu, K):
    """-inf transitions, emissions and initial states, and the impossible observation at step 0,
    at step K (the row a measured step reads) and at step K + 1: rows of -inf alone cross measured
    steps.  Everything stored equals the model; nothing is NaN or +inf."""
    pi, a, b = _banded()
    S, T = 8, 2 * K + 3
    rng = np.random.default_rng(K)
    obs = rng.integers(0, 7, size=(S, T)).astype(np.int32)
    obs[0, 0] = obs[3, K] = obs[4, K + 1] = obs[7, T - 1] = 7
    tb = M.tables(pi, a, b)
    rows, mu = M.forward(tb, obs.astype(np.int64), every=K)
    path, r, E = M.backtrack(tb, rows)
    assert (rows[:, 0] == -np.inf).all() and (rows[K:, 3] == -np.inf).all() and (rows[K + 1:, 4] == -np.inf).all()
    assert np.isfinite(rows[:, 1]).any(axis=1).all()
    h = cv.HMM(pi, a, b)
    h.set_tuning(t64_f32ru_mu_every=K)
    got = cv.f32ru_trace(h, obs)
    for x in (got["rows"], got["mu"], got["r"], got["E"]):
        assert not np.isnan(x).any() and not (x == np.inf).any()
    _check_trace(got, dict(obs=obs, rows=rows, mu=mu, path=path, r=r, E=E), f"banded K={K}")
    # and the decode of these sequences is the f64 kernels'
    off = np.arange(S + 1, dtype=np.int64) * T
    h.set_tuning(t64_f32ru_first=1, t64_fixed_first=0)
    on = cv.decode_batch(h, off, obs.ravel(), dtype="f64", rescore_f64=False)
    assert cv.last_first_pass_kind(h) == "f32ru"
    h.set_tuning(t64_f32ru_first=0, t64_fixed_first=0)
    _same(on, cv.decode_batch(h, off, obs.ravel(), dtype="f64", rescore_f64=False), f"banded K={K}")
    assert (on[2][[0, 3, 4, 7]] == L.SEQ_INFEASIBLE).all() and (on[2] == L.SEQ_OK).any()


@pytest.mark.parametrize("n", NS)
def test_decode_is_the_f64_kernels_under_every_value(gpu, models, n):
    """16 sequences in pairs of six lengths: paths, score bits and statuses equal the f64 kernels'
    (both first-pass keys 0) and each other under every value of the key; the counters too."""
    pi, a, b = models[n]
    lengths = np.repeat([37, 9, 5, 4, 37, 3, 1, 17], 2)
    off = synth.offsets_from_lengths(lengths)
    obs = synth.iid_obs(V, int(off[-1]), seed=n)
    h = cv.HMM(pi, a, b)
    h.set_tuning(t64_f32ru_first=0, t64_fixed_first=0)
    ref = cv.decode_batch(h, off, obs, dtype="f64", rescore_f64=False)
    assert cv.last_first_pass_kind(h) == "none"
    for K in KS + [2, 100]:
        h.set_tuning(t64_f32ru_first=1, t64_fixed_first=0, t64_f32ru_mu_every=K)
        got = cv.decode_batch(h, off, obs, dtype="f64", rescore_f64=False)
        st = cv.last_fixed_first_stats(h)
        assert cv.last_first_pass_kind(h) == "f32ru", K
        assert st["engaged"] == 1 and st["certified"] + st["fallback"] == len(lengths) and st["certified"] > 0, (K, st)
        _same(got, ref, f"N={n} K={K} vs the f64 kernels")


@pytest.mark.parametrize("K", KS)
def test_bad_observation_in_its_own_slot(gpu, models, K):
    import torch

    pi, a, b = models[256]
    B, T = 12, 2 * K + 4
    off = np.arange(B + 1, dtype=np.int64) * T
    obs = synth.iid_obs(V, B * T, seed=21 + K)
    obs[off[5] + K + 1] = V + 3  # in a step between two measured ones (K > 1)
    obs[off[8]] = V + 5

    def run(h):
        dev = torch.device("cuda", 0)
        off_d, obs_d = torch.from_numpy(off).to(dev), torch.from_numpy(obs).to(dev)
        p_d = torch.full((len(obs),), -9, dtype=torch.int32, device=dev)
        s_d = torch.full((B,), np.nan, dtype=torch.float64, device=dev)
        st_d = torch.full((B,), 77, dtype=torch.uint8, device=dev)
        cv.decode_batch_device(h, off_d, obs_d, p_d, s_d, st_d, offsets_host=off, dtype="f64")
        torch.cuda.synchronize(dev)
        return p_d.cpu().numpy(), s_d.cpu().numpy(), st_d.cpu().numpy()

    h = cv.HMM(pi, a, b)
    h.set_tuning(t64_f32ru_first=1, t64_fixed_first=0, t64_f32ru_mu_every=K)
    got = run(h)
    assert cv.last_first_pass_kind(h) == "f32ru"
    st = cv.last_fixed_first_stats(h)
    assert st["engaged"] == 1 and st["fallback"] >= 2 and st["certified"] + st["fallback"] == B, st
    assert got[2][5] == L.SEQ_BADOBS and got[2][8] == L.SEQ_BADOBS and (np.delete(got[2], [5, 8]) == L.SEQ_OK).all()
    h.set_tuning(t64_f32ru_first=0, t64_fixed_first=0)
    _same(got, run(h), f"bad observation, K={K}")


def test_unlisted_values_take_the_nearest_instantiation(gpu, models, modelled):
    """0 and negative values are the default, 2 runs as 1, 3, 5 and 6 as 4, 7 and 100 as 8."""
    h = cv.HMM(*models[256])
    assert h.tuning("t64_f32ru_mu_every") == M.EVERY  # the model's default is the library's
    obs = modelled(256, 37, 1)["obs"]
    ref = {}
    for K in KS:
        h.set_tuning(t64_f32ru_mu_every=K)
        ref[K] = cv.f32ru_trace(h, obs)
    for value, K in ((0, M.EVERY), (-3, M.EVERY), (2, 1), (3, 4), (5, 4), (6, 4), (7, 8), (100, 8)):
        h.set_tuning(t64_f32ru_mu_every=value)
        got = cv.f32ru_trace(h, obs)
        for name in ("rows", "mu", "r", "E"):
            assert np.array_equal(_bits(got[name]), _bits(ref[K][name])), (value, K, name)
        assert np.array_equal(got["path"], ref[K]["path"]), (value, K)
