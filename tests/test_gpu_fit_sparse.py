"""Baum-Welch (cv_hmm_fit_train) on sparse models: every E-step kernel family on the inputs
where normalize()'s zero-sum branch (hmm.rs:274-282, 306-317) fires, where exact zeros must
survive, where a state is never visited, and where tiny arcs sit beside zeros -- against
the numpy oracle (oracle/fit_oracle.py), NaN / +inf / -inf position for position and every
other log10 value to 1e-9.  The families S1-S4 are built in tests/fit_cases.py.

The zero tests are structural (a sum of non-negative f64 terms is 0 only when every term is
0), so another summation order cannot flip them: the project's tolerance holds unchanged.

The CPU tests here pin the preconditions -- that S1 really reaches all four fallbacks and
S2 none -- so the GPU tests exercise what they claim.  Each oracle result is computed once
per session (fit_cases.case) and shared."""
import numpy as np
import pytest

import fit_cases as FC

V = 7
# (N, sequences, tmax) per kernel family.  70 sequences where a workgroup advances 32 at a
# time (two full groups and a partly filled one), 27 elsewhere (one-wave kernels: 4 waves per
# block, 2 sequences per wave -- a partly filled last block and an odd last pair).
WAVE = [(3, 27, 30), (16, 27, 30), (17, 27, 130), (33, 27, 30), (48, 27, 30), (49, 27, 30), (64, 27, 130)]
MM = [(n, 70, 40) for n in (65, 128, 129, 192, 193, 255, 256)]  # NP = 128 / 192 / 256
STRIDED = [(257, 27, 16), (520, 27, 16)]
# tuning keys (read per call): global scratch above 256 states, the per-sequence kernels with
# bw_xi_gemm<2,1> (N <= 128) or bw_stats / bw_xi_gemm_lds (64 < N <= 256)
KNOBS = [(300, 27, 16, ("CV_BW_GLOBAL",)), (20, 27, 30, ("CV_BW_GEMM_PATH",)), (100, 27, 40, ("CV_BW_PERSEQ",)),
         (200, 27, 40, ("CV_BW_PERSEQ",)), (100, 27, 40, ("CV_BW_PERSEQ", "CV_BW_GEMM_PATH"))]
SHAPES = [s + ((),) for s in WAVE + MM + STRIDED] + KNOBS
IDS = ["-".join([str(n)] + [k[6:].lower() for k in keys]) for n, _, _, keys in SHAPES]
S34 = [(20, 27, 30), (100, 70, 40), (300, 27, 16)]  # one-wave, matrix-core and strided kernels


def _run(monkeypatch, keys, inputs, iters):
    import cviterbi as cv

    for k in keys:
        monkeypatch.setenv(k, "1")
    gp, ga, gb, it = cv.fit_train(*inputs, max_iter=iters, tol=0.0)
    assert it == iters
    st = cv.last_fit_stats()  # unhooked: one chunk, one pair per wave (tests/test_gpu_fit_chunks.py: several)
    assert st["chunks"] == 1 and st["pairs_per_wave_max"] <= 1, st
    return gp, ga, gb


def _s1_precondition(n, counts):
    fired = {k for k, c in counts.items() if c > 0}
    need = {"alpha", "beta", "gamma", "xi"} if n >= 20 else {"alpha", "beta", "xi"}
    assert need <= fired, (n, counts)


def _s2_precondition(inputs, counts, ref):
    pi0, a0 = inputs[:2]
    assert counts == {"alpha": 0, "beta": 0, "gamma": 0, "xi": 0}
    assert (a0 == 0).any() or a0.shape[0] < 5
    assert np.array_equal(np.isneginf(ref[1]), a0 == 0)  # A's zeros, and only they
    assert np.array_equal(np.isneginf(ref[0]), pi0 == 0)
    assert not any(np.isnan(x).any() or np.isposinf(x).any() for x in ref)


@pytest.mark.parametrize("n,nseq,tmax,keys", SHAPES, ids=IDS)
def test_s1_reaches_the_fallbacks(n, nseq, tmax, keys):
    inputs, counts, ref = FC.case("s1", n, V, nseq, tmax, 2)
    _s1_precondition(n, counts)
    assert not any(np.isnan(x).any() for x in ref)  # the reference's semantics are well defined here


@pytest.mark.parametrize("n,nseq,tmax,keys", SHAPES, ids=IDS)
def test_s2_reaches_no_fallback_and_keeps_zeros(n, nseq, tmax, keys):
    inputs, counts, ref = FC.case("s2", n, V, nseq, tmax, 2)
    _s2_precondition(inputs, counts, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("n,nseq,tmax,keys", SHAPES, ids=IDS)
def test_gpu_train_s1_fallback_heavy(gpu, monkeypatch, n, nseq, tmax, keys):
    """S1: alpha, beta, gamma and xi go uniform tens to hundreds of times per iteration (1 / N
    over the real states, never over the padded width; uniform xi_t counted and added as
    z / N^2 in the M-step; zero arcs skipped in the factored xi sum).  Two EM iterations."""
    inputs, counts, ref = FC.case("s1", n, V, nseq, tmax, 2)
    _s1_precondition(n, counts)
    FC.assert_params_match(_run(monkeypatch, keys, inputs, 2), ref, atol=1e-9)


@pytest.mark.gpu
@pytest.mark.parametrize("n,nseq,tmax,keys", SHAPES, ids=IDS)
def test_gpu_train_s2_zeros_preserved(gpu, monkeypatch, n, nseq, tmax, keys):
    """S2: no fallback fires, so after two EM iterations A and pi are -inf exactly where the
    start was 0 -- the kernels must reproduce that pattern (assert_params_match compares the
    -inf positions) and the finite entries to 1e-9."""
    inputs, counts, ref = FC.case("s2", n, V, nseq, tmax, 2)
    _s2_precondition(inputs, counts, ref)
    got = _run(monkeypatch, keys, inputs, 2)
    FC.assert_params_match(got, ref, atol=1e-9)
    assert np.array_equal(np.isneginf(got[1]), inputs[1] == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("n,nseq,tmax,keys", KNOBS, ids=IDS[-len(KNOBS):])
def test_gpu_train_knobbed_kernels_dense(gpu, monkeypatch, n, nseq, tmax, keys):
    """The kernels behind the tuning keys on a strictly positive model with 30% random tags:
    the per-sequence ones of bw_perseq / bw_gemm_path had no test at all.  Two EM iterations."""
    inputs, _, ref = FC.case("dense", n, V, nseq, tmax, 2)
    FC.assert_params_match(_run(monkeypatch, keys, inputs, 2), ref, atol=1e-9)


@pytest.mark.gpu
@pytest.mark.parametrize("n,nseq,tmax", S34)
def test_gpu_train_s3_dead_state(gpu, monkeypatch, n, nseq, tmax):
    """S3: state N-1 is never visited, so a_den = b_den = 0 there and the reference divides
    0 by 0 (hmm.rs:152-154, 170-172): rows N-1 of A and B are NaN, column N-1 of A and pi[N-1]
    are -inf.  ONE iteration only: what a second iteration does with NaN parameters is out of
    scope (every sum they touch is NaN in an order-dependent set of places)."""
    inputs, counts, ref = FC.case("s3", n, V, nseq, tmax, 1)
    assert np.isnan(ref[1][n - 1]).all() and np.isnan(ref[2][n - 1]).all()
    assert np.isnan(ref[1]).sum() == n and np.isnan(ref[2]).sum() == V and not np.isnan(ref[0]).any()
    assert np.isneginf(ref[0][n - 1]) and np.isneginf(ref[1][:n - 1, n - 1]).all()
    FC.assert_params_match(_run(monkeypatch, (), inputs, 1), ref, atol=1e-9)


@pytest.mark.gpu
@pytest.mark.parametrize("n,nseq,tmax", S34)
def test_gpu_train_s4_tiny_arcs_beside_zeros(gpu, monkeypatch, n, nseq, tmax):
    """S4: a 1e-306 and a subnormal arc, each forced by tagged runs, in a banded A: the E-step
    runs on A 2^K, whose minimum scan must skip the exact zeros and whose scaled zeros must
    stay zero (the -inf pattern of A survives two EM iterations)."""
    inputs, counts, ref = FC.case("s4", n, V, nseq, tmax, 2)
    a0 = inputs[1]
    (p, q), (p2, q2) = FC.S4_ARCS
    assert 0 < a0[p2, q2] < 2.3e-308 and 0 < a0[p, q] < 2e-306
    assert counts == {"alpha": 0, "beta": 0, "gamma": 0, "xi": 0}
    assert np.array_equal(np.isneginf(ref[1]), a0 == 0) and ref[1][p, q] > -3 and ref[1][p2, q2] > -3
    got = _run(monkeypatch, (), inputs, 2)
    FC.assert_params_match(got, ref, atol=1e-9)
