"""CPU: the posterior path sampler's host-side checks -- the symbols and wrappers exist, the
generator's known answers, the numpy reference sampler of tests/sample_ref.py inside the accuracy
contract against long-double CDFs, argument errors before any device is touched, and hipcc builds
the kernel file for gfx950 without scratch in the one-wave kernels."""
import os
import re
import subprocess

import numpy as np
import pytest

import cviterbi as cv
import sample_ref as sr
from conftest import ROOT, has_gpu
from cviterbi import _lib as L
from test_posterior import random_model


def test_symbols_and_wrappers_exist():
    lib = L.lib()
    for name in ("cv_sample_batch", "cv_sample_batch_device"):
        assert name in L.EXPORTS
        assert getattr(lib, name) is not None
    assert callable(cv.sample_batch) and callable(cv.sample_batch_device) and callable(cv.uniform)
    assert cv.sample.uniform is cv.uniform


@pytest.mark.parametrize("key,expect", [((0, 0, 0, 0), "0x1.da202e598192dp-1"),
                                        ((1, 2, 3, 4), "0x1.cfd7060f11400p-6"),
                                        ((2 ** 63 + 5, 70000, 63, 4095), "0x1.ffe09939fc547p-1"),
                                        ((3019, 0, 1, 0), "0x1.a3084221483d6p-1")])
def test_generator_known_answers(key, expect):
    u = cv.sample.uniform(*key)
    assert float(u) == float.fromhex(expect), (key, float(u).hex())
    assert 0.0 <= float(u) < 1.0


def test_kernel_header_generator_known_answers(tmp_path):
    """The generator the kernels include (csrc/kernels/sample_rng.h, one host / device definition)
    compiled into a host program: the same four answers and 64 more against cv.sample.uniform."""
    inc = os.path.join(ROOT, "consistent-viterbi_amd", "csrc", "kernels")
    src = tmp_path / "rng_check.cpp"
    src.write_text('#include <cstdio>\n#include "sample_rng.h"\n'
                   "int main() {\n"
                   '  std::printf("%a\\n%a\\n%a\\n%a\\n", cvs::uniform(0, 0, 0, 0), cvs::uniform(1, 2, 3, 4),\n'
                   "              cvs::uniform((1ull << 63) + 5, 70000, 63, 4095), cvs::uniform(3019, 0, 1, 0));\n"
                   '  for (unsigned t = 0; t < 64; ++t) std::printf("%a\\n", cvs::uniform(77, 1ull << 40, t % 7, 61 * t));\n'
                   "  return 0;\n}\n")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = tmp_path / "rng_check"
    r = subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-O1", "-I", inc, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    got = [float.fromhex(x) for x in out]
    expect = [float.fromhex(x) for x in ("0x1.da202e598192dp-1", "0x1.cfd7060f11400p-6", "0x1.ffe09939fc547p-1",
                                         "0x1.a3084221483d6p-1")]
    expect += [float(cv.sample.uniform(77, 1 << 40, t % 7, 61 * t)) for t in range(64)]
    assert got == expect


def test_generator_broadcasts_and_is_keyed():
    t = np.arange(300, dtype=np.uint64)
    u = cv.sample.uniform(7, 5, 2, t)
    assert u.shape == (300,) and u.dtype == np.float64 and np.all((u >= 0) & (u < 1))
    assert all(u[k] == cv.sample.uniform(7, 5, 2, int(k)) for k in (0, 1, 63, 64, 299))
    for other in (cv.sample.uniform(8, 5, 2, t), cv.sample.uniform(7, 6, 2, t), cv.sample.uniform(7, 5, 3, t)):
        assert not np.any(other == u)
    assert abs(u.mean() - 0.5) < 0.1


@pytest.mark.parametrize("N,T", [(17, 64), (256, 128)])
def test_reference_sampler_meets_the_contract(N, T):
    """The numpy sampler (f64 rows, two different summation orders) against the long-double
    conditional CDFs at 1 x eps: the bound is not an artefact of comparing like with like."""
    pi, a, b = random_model(N, 6, seed=900 + N)
    obs = sr.model_sequences(pi, a, b, [T], seed=N)
    P, A, B = sr.prob_tables(pi, a, b)
    alpha = sr.forward_rows(P, A, B, obs)
    assert alpha is not None
    Pl, Al, Bl = sr.prob_tables(pi, a, b, np.longdouble)
    alpha_l = sr.forward_rows(Pl, Al, Bl, obs)
    R = 16
    us = np.stack([sr.uniforms(11, 3, r, T) for r in range(R)])
    worst = 0.0
    for order in (None, "blocks"):
        paths = np.stack([sr.sample_path(alpha, A, us[r], order) for r in range(R)])
        d = sr.interval_ratio(alpha_l, Al, paths, us.astype(np.longdouble)) / sr.eps(T, N)
        assert d <= 1.0, (N, T, order, d)
        worst = max(worst, d)
        assert len({p.tobytes() for p in paths}) > 1  # the draws differ
    print(f"N={N} T={T}: numpy sampler at {worst:.4f} of eps")


def test_reference_sampler_never_picks_a_zero_weight():
    w = np.array([0.0, 0.0, 0.25, 0.0, 0.75, 0.0])
    assert sr.pick(w, 0.0) == 2 and sr.pick(w, 0.2499) == 2 and sr.pick(w, 0.25) == 4
    assert sr.pick(w, 1.0 - 2.0 ** -53) == 4
    assert sr.pick(w, 1.0) == 4  # rounding left no prefix above u W: the largest positive state


def _small():
    pi, a, b = random_model(4, 3, seed=1)
    return cv.HMM(pi, a, b), np.array([0, 2], np.int64), np.array([0, 1], np.int32)


def test_null_arguments_and_draw_limits_are_einval():
    h, off, obs = _small()
    path, st8 = np.zeros((64, 2), np.int32), np.zeros(1, np.uint8)
    p = lambda x: x.ctypes.data
    lib = L.lib()
    assert lib.cv_sample_batch(None, 1, p(off), p(obs), 1, 0, 0, None, p(path), None, None, p(st8)) == L.CV_EINVAL
    assert lib.cv_sample_batch(h.handle, 1, p(off), p(obs), 1, 0, 0, None, None, None, None, p(st8)) == L.CV_EINVAL
    assert lib.cv_sample_batch(h.handle, 1, p(off), p(obs), 1, 0, 0, None, p(path), None, None, None) == L.CV_EINVAL
    assert lib.cv_sample_batch(h.handle, 1, None, p(obs), 1, 0, 0, None, p(path), None, None, p(st8)) == L.CV_EINVAL
    assert lib.cv_sample_batch_device(h.handle, 1, None, p(off), p(obs), 1, 0, 0, None, None, None, None,
                                      p(st8)) == L.CV_EINVAL
    assert lib.cv_sample_batch_device(None, 1, None, p(off), p(obs), 1, 0, 0, None, p(path), None, None,
                                      p(st8)) == L.CV_EINVAL
    for draws in (0, 65, -1):
        assert lib.cv_sample_batch(h.handle, 1, p(off), p(obs), draws, 0, 0, None, p(path), None, None,
                                   p(st8)) == L.CV_EINVAL
        assert lib.cv_sample_batch_device(h.handle, 1, None, p(off), p(obs), draws, 0, 0, None, p(path), None, None,
                                          p(st8)) == L.CV_EINVAL
        with pytest.raises(cv.CVError) as e:
            cv.sample_batch(h, off, obs, draws)
        assert e.value.status == L.CV_EINVAL


@pytest.mark.skipif(has_gpu(), reason="checks the no-device error path")
def test_sampling_without_device_fails_loudly():
    h, off, obs = _small()
    with pytest.raises(cv.CVError) as e:
        cv.sample_batch(h, off, obs, 4)
    assert e.value.status == L.CV_EDEVICE


def test_hipcc_builds_sample_for_gfx950(tmp_path):
    """The kernel file compiles for gfx950; the resource remarks show no scratch and no VGPR spill
    in any one-wave (N <= 256) instantiation: NP 64 / 128 / 192 / 256 x 1 / 2 / 4 / 8 draws a wave."""
    src = os.path.join(ROOT, "consistent-viterbi_amd", "csrc", "kernels", "sample.hip")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950", "--cuda-device-only",
                        "-c", src, "-o", str(tmp_path / "sample.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert os.path.getsize(tmp_path / "sample.o") > 0
    blocks = re.split(r"Function Name: ", r.stderr)[1:]
    seen, names = 0, [b.split()[0] for b in blocks]
    for blk in blocks:
        name = blk.split()[0]
        if "sample_wave" in name:
            seen += 1
            assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blk).group(1)) == 0, name
            assert int(re.search(r"VGPRs Spill: (\d+)", blk).group(1)) == 0, name
    assert seen == 16, names
    assert any("sample_gen" in n for n in names) and any("sample_score" in n for n in names), names
