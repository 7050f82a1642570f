"""CPU: the expected-counts feature's host-side checks (cv_expected_counts*) -- the symbols and
Python wrappers exist, null arguments are CV_EINVAL, the numpy oracle of tests/counts_ref.py agrees
with the 60-digit fixtures (tools/make_counts_golden.py) inside the derived bounds, reestimate's
row rules, and hipcc builds the count kernels for gfx950 without scratch and without atomics."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import cviterbi as cv
from conftest import ROOT, has_gpu, load_golden
from counts_ref import a_bound, np_counts, pi_bound, within
from cviterbi import _lib as L
from emis_ref import as_discrete
from test_posterior import FIXTURES, random_model

EMIS_FIXTURES = ["posterior_emis_n3.npz", "posterior_emis_n17.npz", "posterior_emis_n64.npz"]
U_SUM = 2.0 ** -53  # one rounding per term of the test's own sum over the entries
ENTRIES = ("cv_expected_counts", "cv_expected_counts_device", "cv_expected_counts_emissions",
           "cv_expected_counts_emissions_device")


def fixture_model(z):
    """(pi, a, b, obs) of a posterior fixture; a dense-emission one as its discrete equivalent."""
    if "E" in z:
        b, obs = as_discrete(z["E"], len(z["pi"]))
        return z["pi"], z["a"], b, obs
    return z["pi"], z["a"], z["b"], z["obs"]


def check_counts(got_pi, got_a, z, c, suffix, a_log, factor=1.0):
    """Counts against the fixture's 60-digit values at `factor` times the bounds; exact zeros
    wherever A is 0.  Returns the largest error / bound."""
    lens = np.diff(z["offsets"])
    T, Lel, B, N = int(lens.max()), int(lens.sum()), len(lens), len(z["pi"])
    ref_pi, ref_a = c["pi_cnt" + suffix], c["a_cnt" + suffix]
    ra = within(got_a, ref_a, factor * a_bound(T, N, Lel, ref_a))
    rp = within(got_pi, ref_pi, factor * pi_bound(T, N, B, ref_pi))
    assert ra <= 1.0 and rp <= 1.0, (ra, rp)
    assert np.all(got_a[a_log == -np.inf] == 0.0)
    assert np.all(got_a[ref_a == 0.0] == 0.0) and np.all(got_pi[ref_pi == 0.0] == 0.0)
    return max(ra, rp)


def test_symbols_and_wrappers_exist():
    lib = L.lib()
    for name in ENTRIES:
        assert name in L.EXPORTS
        assert getattr(lib, name) is not None
    for f in (cv.expected_counts, cv.expected_counts_device, cv.expected_counts_emissions,
              cv.expected_counts_emissions_device, cv.reestimate):
        assert callable(f)
    assert "xi_part_rows" in cv.tuning_keys()


def test_header_and_integration_name_the_entries():
    header = open(os.path.join(ROOT, "include", "cviterbi.h")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRIES:
        assert re.search(r"CV_API cv_status %s\(" % name, header), name
        assert re.search(r"fn %s\(" % name, integ), name
    assert "xi_part_rows" in header


@pytest.mark.parametrize("name", FIXTURES + EMIS_FIXTURES)
def test_numpy_oracle_matches_golden(name):
    z, c = load_golden(name), load_golden("counts_" + name)
    pi, a, b, obs = fixture_model(z)
    lens = np.diff(z["offsets"])
    T, Lel, B, N = int(lens.max()), int(lens.sum()), len(lens), len(pi)
    worst = 0.0
    for suffix, forced in (("", None), ("_f", z["forced"])):
        got_pi, got_a = np_counts(pi, a, b, z["offsets"], obs, forced)
        worst = max(worst, check_counts(got_pi, got_a, z, c, suffix, a))
        # every fixture sequence is feasible: each counts once in pi and T - 1 times in A
        ref_pi, ref_a = c["pi_cnt" + suffix], c["a_cnt" + suffix]
        assert abs(ref_a.sum() - (Lel - B)) <= a_bound(T, N, Lel, Lel - B) + N * N * U_SUM * (Lel - B)
        assert abs(ref_pi.sum() - B) <= pi_bound(T, N, B, B) + N * U_SUM * B
        assert abs(got_a.sum() - (Lel - B)) <= a_bound(T, N, Lel, Lel - B) + N * N * U_SUM * (Lel - B)
        assert abs(got_pi.sum() - B) <= pi_bound(T, N, B, B) + N * U_SUM * B
    print(f"{name}: numpy oracle at {worst:.4f} of the bounds")


def test_golden_files_are_small():
    for name in FIXTURES + EMIS_FIXTURES:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "counts_" + name)) <= 300 * 1024, name


def test_reestimate():
    pi_cnt = np.array([1.0, 3.0, 0.0])
    a_cnt = np.array([[2.0, 2.0, 0.0], [0.0, 0.0, 0.0], [1.0, 0.0, 3.0]])
    with np.errstate(divide="ignore"):
        pi_prev = np.log10(np.array([0.2, 0.3, 0.5]))
        a_prev = np.log10(np.array([[0.1, 0.2, 0.7], [0.25, 0.5, 0.25], [1.0, 0.0, 0.0]]))
    pi, a = cv.reestimate(pi_cnt, a_cnt, pi_prev, a_prev)
    assert np.allclose(10.0 ** pi, [0.25, 0.75, 0.0], rtol=1e-15, atol=0) and pi[2] == -np.inf
    assert np.allclose(10.0 ** a[0], [0.5, 0.5, 0.0], rtol=1e-15, atol=0) and a[0, 2] == -np.inf
    assert np.array_equal(a[1], a_prev[1])  # a state never left keeps its row
    assert np.allclose(10.0 ** a[2], [0.25, 0.0, 0.75], rtol=1e-15, atol=0)
    assert a_prev[1, 1] == np.log10(0.5)  # inputs untouched
    pi0, _ = cv.reestimate(np.zeros(3), a_cnt, pi_prev, a_prev)
    assert np.array_equal(pi0, pi_prev)
    with pytest.raises(ValueError):
        cv.reestimate(pi_cnt, a_cnt[:2], pi_prev, a_prev)


@pytest.mark.skipif(has_gpu(), reason="checks the no-device error path")
def test_counts_without_device_fail_loudly():
    pi, a, b = random_model(4, 3, seed=1)
    h = cv.HMM(pi, a, b)
    with pytest.raises(cv.CVError) as e:
        cv.expected_counts(h, [0, 3], np.array([1, 2, 0], np.int32))
    assert e.value.status == L.CV_EDEVICE
    with pytest.raises(cv.CVError) as e:
        cv.expected_counts_emissions(h, [0, 3], np.zeros((3, 4)))
    assert e.value.status == L.CV_EDEVICE


def test_null_and_bad_arguments_are_einval():
    pi, a, b = random_model(4, 3, seed=1)
    h = cv.HMM(pi, a, b)
    off = np.array([0, 2], np.int64)
    obs = np.array([0, 1], np.int32)
    E = np.zeros((2, 4))
    ll, pc, ac, st8 = np.zeros(1), np.zeros(4), np.zeros(16), np.zeros(1, np.uint8)
    p = lambda x: x.ctypes.data
    lib = L.lib()
    assert lib.cv_expected_counts(None, 1, p(off), p(obs), None, p(ll), p(pc), p(ac), None, p(st8)) == L.CV_EINVAL
    assert lib.cv_expected_counts(h.handle, 1, p(off), p(obs), None, p(ll), None, p(ac), None, p(st8)) == L.CV_EINVAL
    assert lib.cv_expected_counts(h.handle, 1, p(off), p(obs), None, p(ll), p(pc), None, None, p(st8)) == L.CV_EINVAL
    assert lib.cv_expected_counts(h.handle, 1, p(off), None, None, p(ll), p(pc), p(ac), None, p(st8)) == L.CV_EINVAL
    assert lib.cv_expected_counts(h.handle, -1, p(off), p(obs), None, p(ll), p(pc), p(ac), None, p(st8)) == L.CV_EINVAL
    assert lib.cv_expected_counts_device(h.handle, 1, None, p(off), p(obs), None, None, p(pc), p(ac), None,
                                         p(st8)) == L.CV_EINVAL
    assert lib.cv_expected_counts_emissions(h.handle, 1, p(off), None, 4, None, p(ll), p(pc), p(ac), None,
                                            p(st8)) == L.CV_EINVAL
    assert lib.cv_expected_counts_emissions(h.handle, 1, p(off), p(E), 3, None, p(ll), p(pc), p(ac), None,
                                            p(st8)) == L.CV_EINVAL  # ld < N
    assert lib.cv_expected_counts_emissions_device(h.handle, 1, None, p(off), p(E), 4, None, p(ll), p(pc), None, None,
                                                   p(st8)) == L.CV_EINVAL
    for kw in (dict(dtype=L.DTYPE_F32), dict(assoc=L.ASSOC_CP), dict(kernel=L.KERNEL_TRELLIS)):
        o = L.opts(**{**dict(dtype=L.DTYPE_F64), **kw})
        rc = lib.cv_expected_counts_emissions(h.handle, 1, p(off), p(E), 4, ctypes.byref(o), p(ll), p(pc), p(ac), None,
                                              p(st8))
        assert rc == (L.CV_EUNSUPPORTED if "dtype" in kw else L.CV_EINVAL), kw


KERNELS = os.path.join(ROOT, "consistent-viterbi_amd", "csrc", "kernels")


def test_hipcc_builds_the_count_kernels_for_gfx950(tmp_path):
    """counts.hip (the count kernels and the backward pass with its counts arm: the body of
    post_bwd.h that posterior.hip instantiates without it) compiles for gfx950; the resource
    remarks show no scratch in post_xi_gemm, in the matrix-core kernels or anywhere else."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950", "--cuda-device-only",
                        "-c", os.path.join(KERNELS, "counts.hip"), "-o", str(tmp_path / "counts.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert os.path.getsize(tmp_path / "counts.o") > 0
    seen = {}
    for blk in re.split(r"Function Name: ", r.stderr)[1:]:
        name = blk.split()[0]
        key = next(k for k in ("post_xi_gemm", "post_xi_fold", "post_cnt_bwd_mm", "post_cnt_bwd_gen", "post_cnt_a",
                               "post_cnt_pi") if k in name)
        seen[key] = seen.get(key, 0) + 1
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blk).group(1)) == 0, name
        assert int(re.search(r"VGPRs Spill: (\d+)", blk).group(1)) == 0, name
        if key in ("post_xi_gemm", "post_cnt_bwd_mm"):  # two waves per SIMD: at most 256 VGPRs
            assert int(re.search(r" VGPRs: (\d+)", blk).group(1)) <= 256, name
            assert int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", blk).group(1)) >= 2, name
    # the matrix-core backward pass at NP 64 / 128 / 192 / 256, with gamma and without
    assert seen == dict(post_xi_gemm=1, post_xi_fold=1, post_cnt_bwd_mm=8, post_cnt_bwd_gen=1, post_cnt_a=1,
                        post_cnt_pi=1), seen


def test_count_kernels_use_no_atomics():
    """The sums are plain stores of whole tiles folded in a fixed order: nothing in the kernel
    file adds atomically (that is what makes two calls bit-identical)."""
    code = ""
    for name in ("counts.hip", "post_bwd.h", "posterior.h"):
        code += re.sub(r"//[^\n]*", "", open(os.path.join(KERNELS, name)).read())
    assert "atomic" not in code.lower()
    for kernel in ("post_xi_gemm", "post_xi_fold", "post_cnt_a", "post_cnt_pi", "post_cnt_bwd_mm", "post_cnt_bwd_gen"):
        assert re.search(r"void %s\(" % kernel, code), kernel
