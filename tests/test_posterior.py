"""CPU: the posterior (forward-backward) feature's host-side checks -- the symbols and Python
wrappers exist, the numpy f64 oracle used by tests/test_gpu_posterior.py agrees with the
60-digit golden fixtures (tools/make_posterior_golden.py) inside the derived error bounds, and
hipcc builds the new kernel file for gfx950 without spilling in the hot (scoring) kernel."""
import os
import re
import subprocess

import numpy as np
import pytest

import cviterbi as cv
from conftest import ROOT, has_gpu, load_golden
from cviterbi import _lib as L

U = 2.0 ** -53
FIXTURES = ["posterior_n3.npz", "posterior_n17.npz", "posterior_n64.npz", "posterior_n4_long.npz",
            "posterior_n4_t4096.npz", "posterior_n130.npz", "posterior_n250.npz", "posterior_n300.npz"]
# the fixtures whose tags are partial (the two long ones carry tags on ~30% of 2048 / 4096 elements too)
TAGGED = FIXTURES[:3] + FIXTURES[5:]


# ---- the derived bounds (include/cviterbi.h; DESIGN.md "Posterior") ------------------------------
def loglik_bound(T, N, S):
    return 2 * T * (N + 8) * U / np.log(10) + 4 * T * U * max(1.0, S)


def gamma_bound(T, N, ref):
    return 4 * T * (N + 8) * U * ref + 1e-290


def rowsum_bound(N):
    return 4 * (N + 8) * U


# ---- plain numpy f64 scaled forward-backward (the oracle beyond the fixtures) ------------------------
def np_forward_backward(pi, a, b, obs, forced=None):
    """(loglik, gamma[T, N], S) of one sequence; tables log10 (-inf = 0), forced -1 = free."""
    with np.errstate(over="ignore"):
        P, A, B = 10.0 ** np.asarray(pi), 10.0 ** np.asarray(a), 10.0 ** np.asarray(b)
    T, N = len(obs), len(P)
    if forced is None:
        forced = np.full(T, -1)
    mask = np.ones((T, N))
    for t in range(T):
        if forced[t] >= 0:
            mask[t] = 0.0
            mask[t, forced[t]] = 1.0
    alpha = np.zeros((T, N))
    logc = np.zeros(T)
    for t in range(T):
        y = (P if t == 0 else alpha[t - 1] @ A) * B[:, obs[t]] * mask[t]
        c = y.sum()
        if c == 0:
            return -np.inf, np.zeros((T, N)), np.inf
        alpha[t] = y / c
        logc[t] = np.log10(c)
    gamma = np.zeros((T, N))
    beta = np.ones(N)
    for t in range(T - 1, -1, -1):
        g = alpha[t] * beta
        gamma[t] = g / g.sum()
        if t > 0:
            w = A @ (B[:, obs[t]] * mask[t] * beta)
            beta = w / w.max()
    return float(logc.sum()), gamma, float(np.abs(logc).sum())


def random_model(n, v, seed, zero_frac=0.1):
    """log10 of row-stochastic tables with ~10% zeros (every row keeps a positive entry)."""
    rng = np.random.default_rng(seed)

    def rows(r, c):
        p = rng.gamma(1.0, 1.0, size=(r, c))
        z = rng.random((r, c)) < zero_frac
        z[np.arange(r), rng.integers(0, c, size=r)] = False
        p[z] = 0.0
        return p / p.sum(axis=1, keepdims=True)

    with np.errstate(divide="ignore"):
        return np.log10(rows(1, n)[0]), np.log10(rows(n, n)), np.log10(rows(n, v))


def fixture_sequences(z):
    off = z["offsets"]
    for k in range(len(off) - 1):
        yield k, int(off[k]), int(off[k + 1])


# ---- tests -----------------------------------------------------------------------------------------
def test_symbols_and_wrappers_exist():
    lib = L.lib()
    for name in ("cv_posterior_batch", "cv_posterior_batch_device"):
        assert name in L.EXPORTS
        assert getattr(lib, name) is not None
    assert callable(cv.score_batch) and callable(cv.posterior_batch) and callable(cv.posterior_batch_device)


@pytest.mark.parametrize("name", FIXTURES)
def test_numpy_oracle_matches_golden(name):
    z = load_golden(name)
    N = len(z["pi"])
    worst = 0.0
    for suffix, forced in (("", None), ("_f", z["forced"])):
        for k, lo, hi in fixture_sequences(z):
            T = hi - lo
            ll, gm, S = np_forward_backward(z["pi"], z["a"], z["b"], z["obs"][lo:hi],
                                            None if forced is None else forced[lo:hi])
            ref_ll, ref_g, ref_S = z["loglik" + suffix][k], z["gamma" + suffix][lo:hi], z["S" + suffix][k]
            assert np.isfinite(ref_ll)
            assert abs(S - ref_S) <= 1e-9 * max(1.0, ref_S)
            r1 = abs(ll - ref_ll) / loglik_bound(T, N, ref_S)
            r2 = float(np.max(np.abs(gm - ref_g) / gamma_bound(T, N, ref_g)))
            worst = max(worst, r1, r2)
            assert r1 <= 1.0, (name, suffix, k, ll, ref_ll)
            assert r2 <= 1.0, (name, suffix, k)
            assert np.all(np.abs(gm.sum(axis=1) - 1.0) <= rowsum_bound(N))
            assert np.all(gm[ref_g == 0.0] == 0.0)
    print(f"{name}: numpy oracle at {worst:.4f} of the bounds")


def test_golden_forced_tags_are_partial():
    for name in TAGGED:
        f = load_golden(name)["forced"]
        assert (f >= 0).any() and (f < 0).any()


def test_golden_forced_tags_reach_the_later_tiles():
    """The matrix-core kernels own the states in column tiles of 64 (NP / 64 of them), the plain
    kernels give thread j the states j, j + 256, ...: the wide fixtures must tag a state beyond the
    first tile / the first stride, or a regenerated file silently stops testing the mask there."""
    tags = {}
    for name in FIXTURES[5:]:
        z = load_golden(name)
        f = z["forced"]
        tags[len(z["pi"])] = f[f >= 0]
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name)) <= 195 * 1024, name
    assert sorted(tags) == [130, 250, 300]
    assert (tags[130] >= 64).any() and (tags[130] < 64).any(), tags[130]
    assert (tags[250] >= 192).any(), tags[250]
    assert (tags[300] >= 256).any(), tags[300]


def test_unscaled_forward_underflows_on_the_long_fixture():
    z = load_golden("posterior_n4_t4096.npz")
    assert z["loglik"][0] < -3000 and np.isfinite(z["loglik"][0])
    P, A, B = 10.0 ** z["pi"], 10.0 ** z["a"], 10.0 ** z["b"]
    x = P * B[:, z["obs"][0]]
    for o in z["obs"][1:]:
        x = (x @ A) * B[:, o]
    with np.errstate(divide="ignore"):
        assert np.log10(x.sum()) == -np.inf


@pytest.mark.skipif(has_gpu(), reason="checks the no-device error path")
def test_posterior_without_device_fails_loudly():
    pi, a, b = random_model(4, 3, seed=1)
    h = cv.HMM(pi, a, b)
    with pytest.raises(cv.CVError) as e:
        cv.score_batch(h, [0, 3], np.array([1, 2, 0], np.int32))
    assert e.value.status == L.CV_EDEVICE


def test_null_arguments_are_einval():
    pi, a, b = random_model(4, 3, seed=1)
    h = cv.HMM(pi, a, b)
    off = np.array([0, 2], np.int64)
    obs = np.array([0, 1], np.int32)
    st8 = np.zeros(1, np.uint8)
    p = lambda x: x.ctypes.data
    lib = L.lib()
    assert lib.cv_posterior_batch(h.handle, 1, p(off), p(obs), None, None, None, None, p(st8)) == L.CV_EINVAL
    assert lib.cv_posterior_batch(None, 1, p(off), p(obs), None, None, None, None, p(st8)) == L.CV_EINVAL
    assert lib.cv_posterior_batch_device(h.handle, 1, None, p(off), p(obs), None, None, None, None, p(st8)) == L.CV_EINVAL


def test_hipcc_builds_posterior_for_gfx950(tmp_path):
    """The new kernel file compiles for gfx950; the compiler's resource remarks show no scratch
    spill in the matrix-core kernels (the scoring-mode forward is the hot path)."""
    src = os.path.join(ROOT, "consistent-viterbi_amd", "csrc", "kernels", "posterior.hip")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950", "--cuda-device-only",
                        "-c", src, "-o", str(tmp_path / "posterior.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert os.path.getsize(tmp_path / "posterior.o") > 0
    blocks = re.split(r"Function Name: ", r.stderr)[1:]
    seen = 0
    for blk in blocks:
        name = blk.split()[0]
        if "post_fwd_mm" in name or "post_bwd_mm" in name:
            seen += 1
            assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blk).group(1)) == 0, name
            assert int(re.search(r"VGPRs Spill: (\d+)", blk).group(1)) == 0, name
    assert seen == 16, [b.split()[0] for b in blocks]  # NP 64 / 128 / 192 / 256 x store / gamma
