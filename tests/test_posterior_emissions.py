"""CPU: the host-side checks of cv_posterior_emissions* (evaluation under caller-supplied emission
scores) -- the symbols and wrappers exist, the argument checks that need no device, the fixtures
of tools/make_posterior_emissions_golden.py against the numpy oracle on the substituted model,
hipcc builds emis.hip and posterior.hip for gfx950 without scratch, and the proof of the staging
arithmetic's error bound: the host build of exp10_scaled (csrc/kernels/exp10_scaled.h, the one
source of the host and the device code) against 60-digit arithmetic."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import cviterbi as cv
from conftest import ROOT, has_gpu, load_golden
from cviterbi import _lib as L
from emis_ref import model
from test_posterior import gamma_bound, loglik_bound, np_forward_backward, rowsum_bound

KERNELS = os.path.join(ROOT, "consistent-viterbi_amd", "csrc", "kernels")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
C = 2.0  # kExp10ScaledC: the stated worst case of one staged entry, in u = 2^-53 relative
FIXTURES = ["posterior_emis_n3.npz", "posterior_emis_n17.npz", "posterior_emis_n64.npz",
            "posterior_emis_n4_t4096.npz"]
BENIGN = FIXTURES[:3]  # 10^x of every score is a normal double: the numpy oracle applies


def test_symbols_and_wrappers_exist():
    lib = L.lib()
    for name in ("cv_posterior_emissions", "cv_posterior_emissions_device"):
        assert name in L.EXPORTS
        assert getattr(lib, name) is not None
    assert callable(cv.posterior_emissions) and callable(cv.score_emissions)
    assert callable(cv.posterior_emissions_device)


def test_stated_c_is_the_headers():
    txt = open(os.path.join(KERNELS, "exp10_scaled.h")).read()
    assert float(re.search(r"kExp10ScaledC = ([0-9.]+);", txt).group(1)) == C
    assert C <= 2.0  # the discrete entry's bounds (N + 8 = N + 6 + c) stand unchanged


def _call_args(N=4):
    pi, a, b0 = model(N)
    h = cv.HMM(pi, a, b0)
    off = np.array([0, 2], np.int64)
    E = np.zeros((2, N))
    ll, path, gm, st8 = np.zeros(1), np.zeros(2, np.int32), np.zeros((2, N)), np.zeros(1, np.uint8)
    p = lambda x: x.ctypes.data
    keep = (off, E, ll, path, gm, st8)
    host = [h.handle, 1, p(off), p(E), N, None, p(ll), p(path), p(gm), p(st8)]
    dev = [h.handle, 1, None, p(off), p(E), N, None, p(ll), p(path), p(gm), p(st8)]
    return h, keep, host, dev


def test_null_arguments_and_short_rows_are_einval():
    h, keep, host, dev = _call_args()
    lib = L.lib()
    for hole in (0, 2, 3, 6, 9):
        args = list(host)
        args[hole] = None
        assert lib.cv_posterior_emissions(*args) == L.CV_EINVAL, hole
    for hole in (0, 3, 4, 7, 10):
        args = list(dev)
        args[hole] = None
        assert lib.cv_posterior_emissions_device(*args) == L.CV_EINVAL, hole
    for ld in (3, 0, -1):  # ld < N = 4
        args = list(host)
        args[4] = ld
        assert lib.cv_posterior_emissions(*args) == L.CV_EINVAL, ld
        args = list(dev)
        args[5] = ld
        assert lib.cv_posterior_emissions_device(*args) == L.CV_EINVAL, ld


def test_option_errors_follow_posterior_batch():
    h, keep, host, dev = _call_args()
    lib = L.lib()
    cases = [(L.opts(L.DTYPE_F32, L.ASSOC_VITERBI, L.KERNEL_AUTO), L.CV_EUNSUPPORTED),
             (L.opts(L.DTYPE_F64, L.ASSOC_CP, L.KERNEL_AUTO), L.CV_EINVAL),
             (L.opts(L.DTYPE_F64, L.ASSOC_DECODE, L.KERNEL_AUTO), L.CV_EINVAL),
             (L.opts(L.DTYPE_F64, L.ASSOC_VITERBI, L.KERNEL_TRELLIS_F64), L.CV_EINVAL)]
    for o, code in cases:
        args = list(host)
        args[5] = ctypes.byref(o)
        assert lib.cv_posterior_emissions(*args) == code
        args = list(dev)
        args[6] = ctypes.byref(o)
        assert lib.cv_posterior_emissions_device(*args) == code


@pytest.mark.skipif(has_gpu(), reason="checks the no-device error path")
def test_without_device_fails_loudly():
    h, keep, host, dev = _call_args()
    with pytest.raises(cv.CVError) as e:
        cv.score_emissions(h, keep[0], keep[1])
    assert e.value.status == L.CV_EDEVICE
    with pytest.raises(cv.CVError) as e:
        cv.posterior_emissions(h, keep[0], keep[1], gamma=True)
    assert e.value.status == L.CV_EDEVICE
    assert L.lib().cv_posterior_emissions_device(*dev) == L.CV_EDEVICE


def test_wrapper_array_handling():
    """A row-strided array passes as it is (ld = stride), any other layout is copied; the device
    wrapper rejects a wrong dtype, device or column stride with ValueError."""
    import torch
    from cviterbi import emissions

    seen = {}
    real = L.lib

    class FakeLib:
        def cv_posterior_emissions(self, handle, nseq, off, emis, ld, *rest):
            seen["ld"], seen["ptr"] = ld, emis.value
            return L.CV_OK

        def __getattr__(self, name):
            return getattr(real(), name)

    pi, a, b0 = model(4)
    h = cv.HMM(pi, a, b0)
    wide = np.zeros((6, 7))
    L.lib = lambda: FakeLib()
    try:
        emissions.posterior_emissions(h, [0, 6], wide[:, 1:5])
        assert seen == {"ld": 7, "ptr": wide.ctypes.data + 8}
        emissions.score_emissions(h, [0, 6], wide[:, ::2])  # column stride: copied
        assert seen["ld"] == 4 and seen["ptr"] != wide.ctypes.data
        with pytest.raises(ValueError):
            emissions.posterior_emissions(h, [0, 7], wide)
        with pytest.raises(ValueError):
            emissions.posterior_emissions(h, [0, 6], wide[:, :3])
    finally:
        L.lib = real
    t = torch.zeros(6, 8, dtype=torch.float64)
    for bad in (t.float(), t, t[:, ::2], t[:, :3], t[0]):  # dtype, device (cpu), stride(1), columns, 1-D
        with pytest.raises(ValueError):
            cv.posterior_emissions_device(h, None, bad, None, None, offsets_host=[0, 6])


# ---- the fixtures ------------------------------------------------------------------------------
def fixture_runs(z):
    """(suffix, forced or None) x (k, lo, hi) of a fixture."""
    off = z["offsets"]
    for suffix, forced in (("", None), ("_f", z["forced"])):
        for k in range(len(off) - 1):
            yield suffix, forced, k, int(off[k]), int(off[k + 1])


@pytest.mark.parametrize("name", BENIGN)
def test_numpy_oracle_matches_golden(name):
    z = load_golden(name)
    N = len(z["pi"])
    assert np.array_equal(z["gamma_rows"], np.arange(len(z["E"])))
    b = z["E"].T.copy()
    worst = 0.0
    for suffix, forced, k, lo, hi in fixture_runs(z):
        T = hi - lo
        ll, gm, S = np_forward_backward(z["pi"], z["a"], b, np.arange(lo, hi), None if forced is None else forced[lo:hi])
        ref_ll, ref_g, ref_S = z["loglik" + suffix][k], z["gamma" + suffix][lo:hi], z["S" + suffix][k]
        assert np.isfinite(ref_ll)
        assert abs(S - ref_S) <= 1e-9 * max(1.0, ref_S)
        r1 = abs(ll - ref_ll) / loglik_bound(T, N, ref_S)
        r2 = float(np.max(np.abs(gm - ref_g) / gamma_bound(T, N, ref_g)))
        worst = max(worst, r1, r2)
        assert r1 <= 1.0 and r2 <= 1.0, (name, suffix, k, r1, r2)
        assert np.all(np.abs(gm.sum(axis=1) - 1.0) <= rowsum_bound(N))
    print(f"{name}: numpy oracle at {worst:.4f} of the bounds")


def test_fixtures_are_what_the_issue_asks_for():
    z = load_golden("posterior_emis_n17.npz")
    assert np.isneginf(z["E"]).any() and z["E"].max() > 30 and z["E"].max() <= 40
    z = load_golden("posterior_emis_n64.npz")
    assert len(z["pi"]) == 64 and np.diff(z["offsets"]).max() <= 33
    z = load_golden("posterior_emis_n4_t4096.npz")
    assert z["E"].shape == (4096, 4) and z["E"].min() >= -5200 and z["E"].max() <= -4800
    assert np.all(10.0 ** z["E"] == 0.0)  # the discrete tables cannot hold this model
    spread = z["E"].max(axis=1) - z["E"].min(axis=1)
    assert 200 < spread.max() <= 300  # inside the contract: within 300 decades of the row's maximum
    assert np.isfinite(z["loglik"][0]) and z["loglik"][0] < -1.9e7
    assert len(z["gamma_rows"]) == 256 and z["gamma"].shape == (256, 4)
    limit = os.path.getsize(os.path.join(ROOT, "tests", "golden", "posterior_n64.npz"))
    for name in FIXTURES:
        f = load_golden(name)["forced"]
        assert (f >= 0).any() and (f < 0).any()
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name)) <= limit


# ---- hipcc builds the kernels ------------------------------------------------------------------
def _remarks(src, tmp_path):
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950",
                        "--cuda-device-only", "-c", os.path.join(KERNELS, src), "-o", str(tmp_path / (src + ".o")),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = {}
    for blk in re.split(r"Function Name: ", r.stderr)[1:]:
        out[blk.split()[0]] = {key: int(re.search(pat + r": (\d+)", blk).group(1))
                               for key, pat in (("vgprs", r" VGPRs"), ("scratch", r"ScratchSize \[bytes/lane\]"),
                                                ("spill", r"VGPRs Spill"), ("occupancy", r"Occupancy \[waves/SIMD\]"))}
    return out


def test_hipcc_builds_the_staging_kernel_without_scratch(tmp_path):
    res = {k: v for k, v in _remarks("emis.hip", tmp_path).items() if "emis_prepare_lin_f64" in k}
    assert len(res) == 1, res
    for name, r in res.items():
        print(name, r)
        assert r["scratch"] == 0 and r["spill"] == 0, (name, r)


def test_posterior_kernels_keep_their_resources(tmp_path):
    res = _remarks("posterior.hip", tmp_path)
    assert len(res) == 18, sorted(res)
    for name, r in res.items():
        assert r["scratch"] == 0 and r["spill"] == 0, (name, r)
    big = {k: v for k, v in res.items() if "post_fwd_mmILi256E" in k}
    assert len(big) == 2
    for name, r in big.items():  # two waves per SIMD: at most 256 VGPRs
        print(name, r)
        assert r["vgprs"] <= 256 and r["occupancy"] >= 2, (name, r)


# ---- the proof of c: the host build of exp10_scaled against 60-digit arithmetic -------------------
DRIVER = r"""
#include <cstdio>
#include <cstdint>
#include "exp10_scaled.h"
// stdin: records (f64 x, i64 k); stdout: records (f64 exp10_scaled(x, k), i64 row shift of x,
// f64 exp10_scaled(x, row shift of x))
int main() {
  struct In { double x; int64_t k; } in;
  struct Out { double v; int64_t kr; double vr; } out;
  while (fread(&in, sizeof in, 1, stdin) == 1) {
    out.v = cvx::exp10_scaled(in.x, in.k);
    out.kr = cvx::exp10_row_shift(cvx::exp10_parts(in.x));
    out.vr = cvx::exp10_scaled(in.x, out.kr);
    fwrite(&out, sizeof out, 1, stdout);
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def exp10_driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("exp10")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = d / "driver"
    r = subprocess.run([HIPCC, "-x", "c++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", KERNELS, str(src),
                        "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]

    def run(xs, ks):
        data = b"".join(struct.pack("<dq", float(x), int(k)) for x, k in zip(xs, ks))
        out = subprocess.run([str(exe)], input=data, capture_output=True, check=True).stdout
        assert len(out) == 24 * len(xs)
        return [struct.unpack_from("<dqd", out, 24 * i) for i in range(len(xs))]

    return run


def test_exp10_scaled_is_within_c_ulp_of_60_digit_arithmetic(exp10_driver):
    from mpmath import mp, mpf

    mp.dps = 60
    ln10, ln2 = mp.log(10), mp.log(2)
    log2_10 = ln10 / ln2
    u = mpf(2) ** -53
    tiny = mpf(2) ** -1074
    exact = lambda x, k: mp.exp(mpf(x) * ln10 - k * ln2)
    floor_y = lambda x: int(mp.floor(mpf(x) * log2_10))

    rng = np.random.default_rng(20240611)
    xs, ks = [], []

    def add(x, k):
        xs.append(float(x))
        ks.append(int(k))

    # >= 10^5 seeded pairs: the scores models produce, k within a few binades of the value ...
    for lo, hi, n in ((-400.0, 60.0, 40000), (-1.0, 1.0, 10000), (-5200.0, -4800.0, 15000),
                      (-2.0 ** 40, 2.0 ** 40, 15000), (-1e6, 1e6, 10000)):
        for x in rng.uniform(lo, hi, n):
            add(x, floor_y(x) + int(rng.integers(-3, 3)))
    # ... and entries far below their row's maximum (down to 300 decades)
    for x in rng.uniform(-100.0, 100.0, 10000):
        add(x, floor_y(x + rng.uniform(0.0, 300.0)))
    assert len(xs) >= 100000
    # edges: the value (a row maximum) a power of two or next to one
    i_zero = len(xs)
    add(0.0, 0), add(-0.0, 0), add(0.0, 1), add(0.0, -1)
    for j in list(range(-40, 41)) + [-3000, 3000, 10 ** 9, -10 ** 9, 2 ** 38]:
        x0 = float(mpf(j) / log2_10)
        for x in (x0, np.nextafter(x0, np.inf), np.nextafter(x0, -np.inf)):
            add(x, j), add(x, j - 1)
    # an entry 300 decades below its row's maximum, small and large maxima
    for xmax in (0.0, 37.5, -4999.25, 1e9):
        for d in (299.0, 299.999, 300.0):
            add(xmax - d, floor_y(xmax))
    # |x| next to 2^40
    for x in (np.nextafter(2.0 ** 40, 0), -np.nextafter(2.0 ** 40, 0), 2.0 ** 40 - 1.0, -(2.0 ** 40) + 0.5):
        add(x, floor_y(x)), add(x, floor_y(x) - 1)
    # subnormal results, and below them
    for d in (1021.5, 1023.0, 1040.25, 1073.0, 1074.0, 1075.5, 1100.0, 5000.0):
        x = -d / float(log2_10)
        add(x, 0), add(x + 1234.5, floor_y(1234.5))
    n_inf = len(xs)
    add(-np.inf, 0), add(-np.inf, -12345), add(-np.inf, 2 ** 41)

    got = exp10_driver(xs, ks)
    worst, worst_at = mpf(0), None
    for i, (x, k, (v, kr, vr)) in enumerate(zip(xs, ks, got)):
        if i >= n_inf:
            assert v == 0.0 and np.signbit(v) == False and kr == 0 and vr == 0.0, (x, k, v, kr, vr)  # noqa: E712
            continue
        ex = exact(x, k)
        err = abs(mpf(v) - ex)
        if ex >= mpf(2) ** -1022:  # a normal result: the stated bound
            r = err / (u * ex)
            if r > worst:
                worst, worst_at = r, (x, k)
            assert r <= C, (x, k, v, float(r))
        else:  # outside the accuracy contract: gradual underflow, one more rounding
            assert err <= C * u * ex + tiny / 2, (x, k, v)
        # the row scale puts the value itself into [1, 2)
        assert 1.0 <= vr < 2.0 and abs(kr - floor_y(x)) <= 1, (x, kr, vr)
    assert got[i_zero][0] == 1.0 and got[i_zero + 2][0] == 0.5 and got[i_zero + 3][0] == 2.0
    assert struct.pack("<d", got[i_zero + 1][0]) == struct.pack("<d", got[i_zero][0])  # -0.0 reads as +0.0
    print(f"exp10_scaled: largest error {float(worst):.4f} u at (x, k) = {worst_at}, stated c = {C}")
    assert worst > 0.5  # the measurement is in units of u (a correctly rounded result reaches 1)
