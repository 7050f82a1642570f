"""CPU: the likelihood-gradient feature's host-side checks (cv_loglik_grad_emissions*,
cviterbi.autograd.sequence_loglik) -- the symbols and wrappers exist and the documents name them,
the two references of tests/grad_ref.py (a numpy weighted forward-backward and torch's autograd of
a log-space forward algorithm) agree inside the stated bounds, bad arguments are CV_EINVAL or
ValueError before any device is touched, and hipcc builds grad.hip for gfx950 without scratch."""
import os
import re
import subprocess

import numpy as np
import pytest

import cviterbi as cv
from conftest import ROOT, has_gpu
from counts_ref import np_counts
from cviterbi import _lib as L
from emis_ref import as_discrete, offsets_of
from grad_ref import SEQ_EMPTY, SEQ_OK, grad_ratios, np_grad, torch_grad
from test_posterior import random_model

ENTRIES = ("cv_loglik_grad_emissions", "cv_loglik_grad_emissions_device")
KERNELS = os.path.join(ROOT, "consistent-viterbi_amd", "csrc", "kernels")


def test_symbols_and_wrappers_exist():
    lib = L.lib()
    for name in ENTRIES:
        assert name in L.EXPORTS
        assert getattr(lib, name) is not None
    for f in (cv.loglik_grad_emissions, cv.loglik_grad_emissions_device, cv.autograd.sequence_loglik):
        assert callable(f)


def test_header_and_integration_name_the_entries():
    header = open(os.path.join(ROOT, "include", "cviterbi.h")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRIES:
        assert re.search(r"CV_API cv_status %s\(" % name, header), name
        assert re.search(r"fn %s\(" % name, integ), name
    assert "sequence_loglik" in integ and "ld_grad" in header
    # the three bounds as the header states them
    assert "(4 T (N + 8) + L + 9) u a_abs + 1e-290 L" in header
    assert "(4 T (N + 8) + B + 1) u pi_abs + 1e-290 B" in header
    assert "(4 T (N + 8) + 1) u |w_s| gamma + 1e-290 max(1, |w_s|)" in header


def oracle_case(N, seed):
    """(pi, a, E, off, w, forced): ~10% zeros in the model, ~5% -inf scores (every row keeps a
    finite one), lengths 0, 1 and 2 among the ragged ones, signed weights, partial tags."""
    rng = np.random.default_rng(seed)
    pi, a, _ = random_model(N, 2, seed=seed)
    lengths = [7, 0, 1, 2, 5, 3, 12, 1, 9]
    off = offsets_of(lengths)
    total = int(off[-1])
    E = rng.normal(0.0, 2.0, size=(total, N))
    hole = rng.random(E.shape) < 0.05
    hole[np.arange(total), rng.integers(0, N, size=total)] = False
    E[hole] = -np.inf
    w = rng.normal(0.0, 2.0, size=len(lengths))
    w[0] = -abs(w[0])
    # tags on a third of the elements, along a path the model and the scores allow
    forced = np.full(total, -1, np.int32)
    P, A = 10.0 ** pi, 10.0 ** a
    for lo, hi in zip(off[:-1], off[1:]):
        prev = None
        for e in range(lo, hi):
            ok = np.isfinite(E[e]) & ((P > 0) if prev is None else (A[prev] > 0))
            if not ok.any():
                break
            prev = int(rng.choice(np.nonzero(ok)[0]))
            forced[e] = prev
    forced[rng.random(total) < 2.0 / 3.0] = -1
    return pi, a, E, off, w, forced


@pytest.mark.parametrize("N", [3, 17, 65])
def test_the_two_oracles_agree(N):
    pi, a, E, off, w, forced = oracle_case(N, 4200 + N)
    assert {0, 1, 2} <= set(np.diff(off).tolist()) and (w < 0).any() and (w > 0).any()
    assert np.isinf(E).any() and np.isinf(a).any()
    worst = 0.0
    for tags in (None, forced):
        ref = np_grad(pi, a, E, off, w, tags)
        tg = torch_grad(pi, a, E, off, w, tags)
        assert list(ref["status"] == SEQ_OK) == list(~np.isnan(tg["loglik"]))
        assert ref["status"][1] == SEQ_EMPTY and (ref["status"] == SEQ_OK).sum() >= 6
        ratios = grad_ratios(tg["pi"], tg["a"], tg["e"], ref, off, N, w, 1.0)
        assert max(ratios) <= 1.0, (N, tags is not None, ratios)
        worst = max(worst, *ratios)
        # exactly 0 on every -inf parameter and score, in both
        for g in (ref, tg):
            assert np.all(g["a"][np.isinf(a)] == 0.0) and np.all(g["pi"][np.isinf(pi)] == 0.0)
            assert np.all(g["e"][np.isinf(E)] == 0.0)
        if tags is not None:
            on = tags >= 0
            others = np.ones_like(E, bool)
            others[on, tags[on]] = False
            others[~on] = False
            assert np.all(ref["e"][others] == 0.0) and np.all(tg["e"][others] == 0.0)
    print(f"N={N}: the oracles agree at {worst:.4f} of the bounds")


@pytest.mark.parametrize("N", [3, 17, 65])
def test_unit_weights_are_np_counts(N):
    pi, a, E, off, _, forced = oracle_case(N, 4200 + N)
    b, obs = as_discrete(E, N)
    for tags in (None, forced):
        ref = np_grad(pi, a, E, off, None, tags)
        pi_cnt, a_cnt = np_counts(pi, a, b, off, obs, tags)
        assert np.array_equal(ref["pi"], pi_cnt) and np.array_equal(ref["a"], a_cnt)
        assert np.array_equal(ref["pi"], ref["pi_abs"]) and np.array_equal(ref["a"], ref["a_abs"])
        # gamma rows sum to 1 on every OK sequence
        lens = np.diff(off)
        rows = np.repeat(ref["status"] == SEQ_OK, lens)
        assert np.allclose(ref["e"][rows].sum(axis=1), 1.0, rtol=0, atol=1e-12)


def test_numpy_oracle_scales_rows_that_underflow():
    N = 4
    pi, a, _ = random_model(N, 2, seed=31, zero_frac=0.0)
    rng = np.random.default_rng(5)
    E = rng.normal(0.0, 2.0, size=(6, N))
    off = offsets_of([6])
    shifted = E.copy()
    shifted[2] -= 5000.0
    x, y = np_grad(pi, a, E, off, [1.5]), np_grad(pi, a, shifted, off, [1.5])
    assert y["status"][0] == SEQ_OK
    for k in ("pi", "a", "e"):  # x - 5000 rounds at 5000 u = 6e-13, so 10^x moves by 1.3e-12 relative
        assert np.allclose(x[k], y[k], rtol=1e-10, atol=0), k


@pytest.mark.skipif(has_gpu(), reason="checks the no-device error path")
def test_gradients_without_device_fail_loudly():
    pi, a, b = random_model(4, 3, seed=1)
    h = cv.HMM(pi, a, b)
    with pytest.raises(cv.CVError) as e:
        cv.loglik_grad_emissions(h, [0, 3], np.zeros((3, 4)), weights=[1.0])
    assert e.value.status == L.CV_EDEVICE


def test_null_and_bad_arguments_are_einval():
    pi, a, b = random_model(4, 3, seed=1)
    h = cv.HMM(pi, a, b)
    off = np.array([0, 2], np.int64)
    E, w = np.zeros((2, 4)), np.ones(1)
    ll, pg, ag, eg, st8 = np.zeros(1), np.zeros(4), np.zeros(16), np.zeros((2, 4)), np.zeros(1, np.uint8)
    p = lambda x: x.ctypes.data
    f, fd = L.lib().cv_loglik_grad_emissions, L.lib().cv_loglik_grad_emissions_device
    EINVAL = L.CV_EINVAL
    assert f(None, 1, p(off), p(E), 4, p(w), None, p(ll), p(pg), p(ag), p(eg), 4, p(st8)) == EINVAL
    assert f(h.handle, 1, p(off), p(E), 4, p(w), None, p(ll), p(pg), None, p(eg), 4, p(st8)) == EINVAL  # a_grad_out
    assert f(h.handle, 1, p(off), p(E), 4, p(w), None, p(ll), None, p(ag), p(eg), 4, p(st8)) == EINVAL
    assert f(h.handle, 1, p(off), p(E), 4, p(w), None, p(ll), p(pg), p(ag), p(eg), 3, p(st8)) == EINVAL  # ld_grad < N
    assert f(h.handle, 1, p(off), p(E), 3, p(w), None, p(ll), p(pg), p(ag), p(eg), 4, p(st8)) == EINVAL  # ld < N
    assert f(h.handle, 1, p(off), None, 4, p(w), None, p(ll), p(pg), p(ag), p(eg), 4, p(st8)) == EINVAL
    assert f(h.handle, 1, p(off), p(E), 4, p(w), None, None, p(pg), p(ag), p(eg), 4, p(st8)) == EINVAL
    assert f(h.handle, 1, p(off), p(E), 4, p(w), None, p(ll), p(pg), p(ag), p(eg), 4, None) == EINVAL
    assert f(h.handle, -1, p(off), p(E), 4, p(w), None, p(ll), p(pg), p(ag), p(eg), 4, p(st8)) == EINVAL
    assert fd(h.handle, 1, None, p(off), p(E), 4, p(w), None, p(ll), p(pg), None, p(eg), 4, p(st8)) == EINVAL
    assert fd(h.handle, 1, None, p(off), p(E), 4, p(w), None, p(ll), p(pg), p(ag), p(eg), 3, p(st8)) == EINVAL
    assert fd(h.handle, 1, None, p(off), p(E), 3, p(w), None, p(ll), p(pg), p(ag), p(eg), 4, p(st8)) == EINVAL
    assert fd(h.handle, 1, None, None, p(E), 4, p(w), None, p(ll), p(pg), p(ag), p(eg), 4, p(st8)) == EINVAL
    import ctypes
    o = L.opts(L.DTYPE_F32)
    assert f(h.handle, 1, p(off), p(E), 4, p(w), ctypes.byref(o), p(ll), p(pg), p(ag), p(eg), 4,
             p(st8)) == L.CV_EUNSUPPORTED
    with pytest.raises(ValueError):
        cv.loglik_grad_emissions(h, off, np.zeros((2, 3)))  # fewer columns than states
    with pytest.raises(ValueError):
        cv.loglik_grad_emissions(h, off, E, weights=np.ones(2))  # one weight per sequence


def test_sequence_loglik_rejects_f32_cpu_and_shapes():
    torch = pytest.importorskip("torch")
    N = 4
    pi, a, _ = random_model(N, 2, seed=1)
    lp, la = torch.tensor(pi), torch.tensor(a)
    off = [0, 2]
    f = cv.autograd.sequence_loglik
    with pytest.raises(ValueError, match="GPU"):
        f(torch.zeros((2, N), dtype=torch.float64), off, lp, la)  # emis on the CPU
    with pytest.raises(ValueError, match="float64"):
        f(torch.zeros((2, N), dtype=torch.float32), off, lp, la)
    with pytest.raises(ValueError, match="float64"):
        f(torch.zeros((2, N), dtype=torch.float64), off, lp.float(), la)
    with pytest.raises(ValueError, match="torch tensor"):
        f(np.zeros((2, N)), off, lp, la)
    meta = torch.zeros((2, N), dtype=torch.float64, device="meta")  # no GPU: still not a CPU tensor
    with pytest.raises(ValueError):
        f(meta, off, lp, la)
    with pytest.raises(ValueError, match=r"\[N\] and \[N, N\]"):
        f(torch.zeros((2, N), dtype=torch.float64), off, lp, la[:, :3])


def test_hipcc_builds_the_gradient_kernels_for_gfx950(tmp_path):
    """grad.hip (the backward bodies of post_bwd.h with their gradient arm) compiles for gfx950; the
    resource remarks show no scratch and no spills, and the matrix-core kernels keep two waves per
    SIMD at every NP."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950", "--cuda-device-only",
                        "-c", os.path.join(KERNELS, "grad.hip"), "-o", str(tmp_path / "grad.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert os.path.getsize(tmp_path / "grad.o") > 0
    seen = {}
    for blk in re.split(r"Function Name: ", r.stderr)[1:]:
        name = blk.split()[0]
        key = next(k for k in ("post_grad_bwd_mm", "post_grad_bwd_gen") if k in name)
        seen[key] = seen.get(key, 0) + 1
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blk).group(1)) == 0, name
        assert int(re.search(r"VGPRs Spill: (\d+)", blk).group(1)) == 0, name
        if key == "post_grad_bwd_mm":
            assert int(re.search(r" VGPRs: (\d+)", blk).group(1)) <= 256, name
            assert int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", blk).group(1)) >= 2, name
            assert 2 * int(re.search(r"LDS Size \[bytes/block\]: (\d+)", blk).group(1)) <= 160 * 1024, name
    # NP 64 / 128 / 192 / 256, with the gradient rows of E and without
    assert seen == dict(post_grad_bwd_mm=8, post_grad_bwd_gen=1), seen


def test_gradient_kernels_use_no_atomics_and_the_makefile_builds_them():
    code = re.sub(r"//[^\n]*", "", open(os.path.join(KERNELS, "grad.hip")).read())
    assert "atomic" not in code.lower()
    for kernel in ("post_grad_bwd_mm", "post_grad_bwd_gen"):
        assert re.search(r"void %s\(" % kernel, code), kernel
    mk = open(os.path.join(ROOT, "consistent-viterbi_amd", "csrc", "Makefile")).read()
    assert "$(BUILD)/grad.o:" in mk and "grad.resource.txt" in mk
