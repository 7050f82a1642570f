"""Baum-Welch (cv_hmm_fit_train) across its two host-side splitting rules, which a realistic
corpus reaches and a test-sized one never did: several pairs of sequences per backward wave
(N <= 64: more than 8 waves per compute unit's worth of pairs) and several chunks of alpha /
beta rows (more elements than the device-memory cap).  The tuning keys bw_max_waves and
bw_chunk_elems (CV_BW_MAX_WAVES, CV_BW_CHUNK_ELEMS, read per call) bring both down to test
size; cv_hmm_fit_last_stats (cviterbi.last_fit_stats) says which path a call took, and every
test here asserts it, so none passes on one chunk and one pair per wave.

Reference and tolerance are the project's: oracle/fit_oracle.py through
fit_cases.assert_params_match -- NaN / +inf / -inf position for position, every finite log10
value to 1e-9 after two EM iterations -- and the 60-digit fixtures under the bounds of
test_fit.test_gpu_train_matches_60_digit_golden.  Oracle results come from fit_cases.case
(once per session, shared with tests/test_gpu_fit_sparse.py where the shapes coincide).

CPU tests pin the preconditions: the corpora of part A put the odd-step flush between two
pairs of one wave, the caps of part C give the chunk counts the tests expect, the fixtures
split as part D needs, and part E's tolerance sits clear of every per-iteration d.
"""
import ctypes
import functools

import numpy as np
import pytest

import fit_cases as FC
import fit_oracle as FO
import test_fit as TF
from conftest import load_golden

V = 7
ATOL = 1e-9
ITERS = 2


def _run(monkeypatch, env, inputs, iters=ITERS, tol=0.0):
    """fit_train under the environment `env` -> ((pi, a, b), iterations, last_fit_stats)."""
    import cviterbi as cv

    for k in ("CV_BW_CHUNK_ELEMS", "CV_BW_MAX_WAVES", "CV_BW_GLOBAL", "CV_BW_PERSEQ", "CV_BW_GEMM_PATH"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    gp, ga, gb, it = cv.fit_train(*inputs, max_iter=iters, tol=tol)
    return (gp, ga, gb), it, cv.last_fit_stats()


def _ceil_div(x, y):
    return -(-x // y)


# ---- A. several pairs per wave, hooked -----------------------------------------------------------
# one N per register layout of the one-wave kernels (NP = 16 / 32 / 48 / 64); tmax 130 crosses
# the 8-step prefetch windows many times.  S4 needs states 0..8 (fit_cases.S4_ARCS), so N = 3
# runs dense and S1 only; S4 appends 24 forced sequences to the 27 / 28.
PAIRS_N = [(3, 30), (17, 130), (48, 30), (64, 130)]
PAIRS = [(fam, n, nseq, tmax) for n, tmax in PAIRS_N for nseq in (27, 28) for fam in ("dense", "s1", "s4")
         if not (fam == "s4" and n < 9)]
PAIRS_IDS = [f"{fam}-n{n}-r{nseq}" for fam, n, nseq, tmax in PAIRS]
WAVES = (1, 3)


@pytest.mark.parametrize("fam,n,nseq,tmax", PAIRS, ids=PAIRS_IDS)
def test_pair_corpora_put_the_flush_between_two_pairs(fam, n, nseq, tmax):
    """With 1 and with 3 backward waves some wave walks a pair with L - 1 odd (its last step
    staged alone: the flush arm) and next a pair with L - 1 even; the odd corpora leave their last
    pair without a second sequence, and 1 and 3 waves mean 14 and 5 pairs for the busiest."""
    inputs, counts, ref = FC.case(fam, n, V, nseq, tmax, ITERS)
    off = inputs[3]
    r = len(off) - 1
    assert r == nseq + (24 if fam == "s4" else 0) and r % 2 == nseq % 2
    for key in WAVES:
        assert FC.flush_then_full_stage(off, key), (key, FC.pair_steps(off))
    if fam != "s4":
        assert [_ceil_div(_ceil_div(r, 2), key) for key in WAVES] == [14, 5]
    if fam == "s1":
        assert counts["xi"] > 0  # uniform xi steps: the count z a wave carries across its pairs
    if fam == "s4":
        assert 0 < inputs[1][FC.S4_ARCS[1]] < 2.3e-308  # the E-step runs on A 2^K


@pytest.mark.gpu
@pytest.mark.parametrize("key", WAVES)
@pytest.mark.parametrize("fam,n,nseq,tmax", PAIRS, ids=PAIRS_IDS)
def test_gpu_train_several_pairs_per_wave(gpu, monkeypatch, fam, n, nseq, tmax, key):
    """One or three backward waves for 14 pairs and more: every wave carries its matrix-core
    accumulators, staging rows, prefetch slots, beta and gamma sums from one pair to the next."""
    inputs, _, ref = FC.case(fam, n, V, nseq, tmax, ITERS)
    r = len(inputs[3]) - 1
    got, it, st = _run(monkeypatch, {"CV_BW_MAX_WAVES": key}, inputs)
    assert it == ITERS
    assert st["family"] == "wave" and st["chunks"] == 1, st
    assert st["pairs_per_wave_max"] == _ceil_div(_ceil_div(r, 2), key) >= 5, st
    FC.assert_params_match(got, ref, atol=ATOL)


# ---- B. several pairs per wave, unhooked ---------------------------------------------------------
def _short_nseq(cus):
    return 4 * (8 * cus) + 75


def test_short_corpus_size():
    """On 256 compute units: 8,267 sequences in about 25 k elements, 4,134 pairs for 2,048
    backward waves -- three pairs for the busiest."""
    r = _short_nseq(256)
    assert r == 8267
    off = FC.short(20, V, r, 5, seed=9020)[3]
    assert 24000 < off[-1] < 26000 and np.diff(off).min() == 1 and np.diff(off).max() == 5
    assert _ceil_div(_ceil_div(r, 2), 8 * 256) == 3


@pytest.mark.gpu
@pytest.mark.parametrize("n", [20, 64])
def test_gpu_train_more_pairs_than_waves(gpu, monkeypatch, n):
    """No key set: 4 x (8 waves per compute unit) + 75 sequences of 1..5 elements, so the default
    wave count itself sends every wave through three pairs or more (and the forward kernel's
    dump-slot index wraps)."""
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    r = _short_nseq(cus)
    inputs, _, ref = FC.case("short", n, V, r, 5, ITERS)
    got, it, st = _run(monkeypatch, {}, inputs)
    assert it == ITERS
    assert st["family"] == "wave" and st["chunks"] == 1, st
    assert st["pairs_per_wave_max"] == _ceil_div(_ceil_div(r, 2), 8 * cus) >= 3, (st, cus)
    FC.assert_params_match(got, ref, atol=ATOL)


# ---- C. several chunks, hooked -------------------------------------------------------------------
# (name, N, sequences, tmax, keys, family last_fit_stats must report): one shape or two per E-step
# family; 70 sequences where a workgroup advances 32 at a time, so chunks cut those groups
CHUNK_SHAPES = [
    ("wave", 20, 27, 30, (), "wave"), ("wave", 64, 27, 130, (), "wave"),
    ("mm", 100, 70, 40, (), "mm"), ("mm", 256, 70, 40, (), "mm"),
    ("perseq", 100, 27, 40, ("CV_BW_PERSEQ",), "perseq"), ("perseq", 200, 27, 40, ("CV_BW_PERSEQ",), "perseq"),
    ("gemm", 20, 27, 30, ("CV_BW_GEMM_PATH",), "perseq"),
    ("strided", 300, 27, 16, (), "strided"), ("global", 300, 27, 16, ("CV_BW_GLOBAL",), "strided_global"),
]
S4_SHAPES = {("wave", 20), ("mm", 100), ("strided", 300)}
CHUNKS = [(fam,) + s for s in CHUNK_SHAPES for fam in ("dense", "s1", "s4")
          if fam != "s4" or (s[0], s[1]) in S4_SHAPES]
CHUNKS_IDS = [f"{fam}-{name}-n{n}" for fam, name, n, *_ in CHUNKS]
CAPS = ("third", "tmax", "one")


def _cap(which, off, tmax):
    """(i) a third of the corpus: three or four chunks; (ii) tmax: one or two sequences per
    chunk, the longest fills one exactly; (iii) 1: every sequence its own chunk, all but the
    T = 1 ones longer than the cap."""
    return {"third": int(off[-1]) // 3 + 1, "tmax": tmax, "one": 1}[which]


@pytest.mark.parametrize("which", CAPS)
@pytest.mark.parametrize("fam,name,n,nseq,tmax,keys,family", CHUNKS, ids=CHUNKS_IDS)
def test_caps_split_the_corpora_as_expected(fam, name, n, nseq, tmax, keys, family, which):
    inputs, _, _ = FC.case(fam, n, V, nseq, tmax, ITERS)
    off = inputs[3]
    r = len(off) - 1
    lengths = np.diff(off)
    assert lengths.min() == 1 and lengths.max() == tmax
    chunks, biggest, most = FC.chunk_stats(off, _cap(which, off, tmax))
    if which == "third":
        assert chunks in (3, 4) and biggest <= int(off[-1]) // 3 + 1
        if name == "mm":  # chunks cut the 32-sequence groups: no chunk is a multiple of 32
            assert all((s1 - s0) % 32 for s0, s1 in FC.greedy_chunks(off, _cap(which, off, tmax)))
    elif which == "tmax":
        assert biggest == tmax and 3 <= chunks < r
        sizes = [s1 - s0 for s0, s1 in FC.greedy_chunks(off, tmax)]
        assert 1 in sizes and max(sizes) >= 2  # (S4's forced sequences of 2 and 3 share chunks in numbers)
        k = int(np.argmax(lengths))
        assert (k, k + 1) in FC.greedy_chunks(off, tmax)  # the longest fills a chunk exactly
    else:
        assert chunks == r and most == 1 and biggest == tmax > 1


@pytest.mark.gpu
@pytest.mark.parametrize("which", CAPS)
@pytest.mark.parametrize("fam,name,n,nseq,tmax,keys,family", CHUNKS, ids=CHUNKS_IDS)
def test_gpu_train_several_chunks(gpu, monkeypatch, fam, name, n, nseq, tmax, keys, family, which):
    """Every E-step family with its alpha / beta rows reused chunk after chunk: the chunk's
    offsets, element base and longest-first order, the row count of the xi GEMM (1 for a T = 1
    sequence alone), and the sums accumulated across chunks."""
    inputs, _, ref = FC.case(fam, n, V, nseq, tmax, ITERS)
    off = inputs[3]
    cap = _cap(which, off, tmax)
    env = {k: 1 for k in keys}
    env["CV_BW_CHUNK_ELEMS"] = cap
    got, it, st = _run(monkeypatch, env, inputs)
    assert it == ITERS
    chunks, biggest, _ = FC.chunk_stats(off, cap)
    assert (st["chunks"], st["max_chunk_elems"]) == (chunks, biggest) and chunks >= 3, (st, chunks, biggest)
    assert st["family"] == family, st
    assert st["pairs_per_wave_max"] == (1 if family == "wave" else 0), st
    assert st["scratch_batches"] == (1 if family == "strided_global" else 0), st
    FC.assert_params_match(got, ref, atol=ATOL)


@pytest.mark.gpu
@pytest.mark.parametrize("fam", ["dense", "s1", "s4"])
def test_gpu_train_chunks_and_one_wave(gpu, monkeypatch, fam):
    """Both rules at once at N = 20: three or four chunks, each walked by a single wave."""
    inputs, _, ref = FC.case(fam, 20, V, 27, 30, ITERS)
    off = inputs[3]
    cap = _cap("third", off, 30)
    got, it, st = _run(monkeypatch, {"CV_BW_CHUNK_ELEMS": cap, "CV_BW_MAX_WAVES": 1}, inputs)
    chunks, biggest, most = FC.chunk_stats(off, cap)
    assert it == ITERS and st["family"] == "wave", st
    assert (st["chunks"], st["max_chunk_elems"]) == (chunks, biggest) and chunks >= 3, (st, chunks, biggest)
    assert st["pairs_per_wave_max"] == _ceil_div(most, 2) >= 3, (st, most)
    FC.assert_params_match(got, ref, atol=ATOL)


@pytest.mark.gpu
def test_gpu_train_scratch_batches_inside_a_chunk(gpu, monkeypatch):
    """The global-scratch kernels take 2,048 sequences per launch: a first chunk of 2,060
    sequences (two launches, the second from sequence 2,048 of the chunk's offsets) and a second
    chunk of 40, N = 300 (lengths 1 and 2: the oracle's time goes with the elements)."""
    inputs, _, ref = FC.case("short", 300, V, 2100, 2, ITERS)
    off = inputs[3]
    cap = int(off[2060])
    assert FC.greedy_chunks(off, cap) == [(0, 2060), (2060, 2100)]
    got, it, st = _run(monkeypatch, {"CV_BW_GLOBAL": 1, "CV_BW_CHUNK_ELEMS": cap}, inputs)
    assert it == ITERS
    assert st == dict(chunks=2, max_chunk_elems=cap, pairs_per_wave_max=0, scratch_batches=2,
                      family="strided_global", family_code=5), st
    FC.assert_params_match(got, ref, atol=ATOL)


# ---- D. against the 60-digit fixtures ------------------------------------------------------------
GOLDEN_ENV = [("fit_dense_n5.npz", True), ("fit_s1_n17.npz", True), ("fit_s1_n70.npz", False)]


def _golden_cap(z):
    return int(z["offsets"][-1] - z["offsets"][0]) // 3 + 1


@pytest.mark.parametrize("name,one_wave", GOLDEN_ENV)
def test_golden_corpora_split(name, one_wave):
    z = load_golden(name)
    off = z["offsets"] - z["offsets"][0]
    chunks, _, most = FC.chunk_stats(off, _golden_cap(z))
    assert chunks >= 3
    if one_wave:
        assert z["a"].shape[0] <= 64 and most >= 3  # a chunk of two pairs or more for its one wave


@pytest.mark.gpu
@pytest.mark.parametrize("name,one_wave", GOLDEN_ENV)
def test_gpu_train_chunked_matches_60_digit_golden(gpu, monkeypatch, name, one_wave):
    """The fixtures of test_gpu_train_matches_60_digit_golden in chunks of a third of the corpus
    (the one-wave ones on a single backward wave), under that test's bounds: error <= 1e-9 and
    <= 32 x max(the oracle's own error, 4 ulp of the value) -- a check that does not depend on
    the oracle's summation order.  The ratios are printed (pytest -s) and recorded in DESIGN.md §4.

    Measured on an MI355X (four chunks each; iterations 1 / 2): ratios 0.75 / 0.50 (N = 5),
    0.40 / 0.43 (N = 17), 0.15 / 0.20 (N = 70)."""
    z = load_golden(name)
    off = z["offsets"] - z["offsets"][0]
    cap = _golden_cap(z)
    env = {"CV_BW_CHUNK_ELEMS": cap}
    if one_wave:
        env["CV_BW_MAX_WAVES"] = 1
    chunks, biggest, most = FC.chunk_stats(off, cap)
    for it in (1, 2):
        got, n_it, st = _run(monkeypatch, env, (z["pi"], z["a"], z["b"], z["offsets"], z["obs"], z["tags"]), iters=it)
        assert n_it == it
        assert (st["chunks"], st["max_chunk_elems"]) == (chunks, biggest) and chunks >= 3, (st, chunks, biggest)
        if one_wave:
            assert st["pairs_per_wave_max"] == _ceil_div(most, 2) >= 2, st
        err, ratio = TF._golden_err(got, z, it)
        print(f"{name} it={it} chunks={chunks}: gpu err {err:.3e}, oracle err "
              f"{float(z['oracle_err'][it - 1]):.3e}, ratio {ratio:.2f}")
        assert err <= 1e-9
        assert ratio <= 32.0


# ---- E. the M-step's grid stride -----------------------------------------------------------------
# bw_mstep_b is grid-strided over 1,024 x 256 threads: V N above 262,144 sends threads through a
# second entry (the largest V N of the other tests is 45 k)
MSTEP = [(20, 14000), (100, 3000)]
MSTEP_THREADS = 1024 * 256


@pytest.mark.gpu
@pytest.mark.parametrize("n,v", MSTEP)
def test_gpu_train_mstep_grid_stride(gpu, monkeypatch, n, v):
    assert v * n > MSTEP_THREADS
    inputs, _, ref = FC.case("dense", n, v, 40, 30, ITERS)
    got, it, st = _run(monkeypatch, {}, inputs)
    assert it == ITERS and st["chunks"] == 1 and st["family"] == ("wave" if n <= 64 else "mm"), st
    FC.assert_params_match(got, ref, atol=ATOL)


@functools.lru_cache(maxsize=None)
def _convergence_case():
    """N = 100, V = 3,000: the oracle's d of the first four iterations, and a tolerance half way
    (geometrically) between the first's and the second's, so the oracle stops after the second.
    (On 600 elements for 300,000 emission entries d is not monotone: ~205, 38, 47, 58 -- only the
    first step down is a place to stop.)"""
    inputs, _, _ = FC.case("dense", 100, 3000, 40, 30, ITERS)
    pi, a, b = inputs[:3]
    ds = []
    for _ in range(4):
        pi, a, b, d = FO.train_step(pi, a, b, *inputs[3:])
        ds.append(float(d))
    return inputs, ds, float(np.sqrt(ds[0] * ds[1]))


def test_convergence_tolerance_is_clear_of_every_d():
    inputs, ds, tol = _convergence_case()
    assert ds[1] < tol < ds[0], (ds, tol)
    assert all(abs(d - tol) > 1e-6 * tol for d in ds), (ds, tol)
    assert FO.train(*inputs, 50, tol)[3] == 2


@pytest.mark.gpu
def test_gpu_train_mstep_grid_stride_converges_like_oracle(gpu, monkeypatch):
    """The convergence sum d = sum |new - old| over V N = 300,000 entries of b (per-block parts
    of the grid-strided M-step, added on the host) stops the iteration where the oracle stops."""
    inputs, ds, tol = _convergence_case()
    assert all(abs(d - tol) > 1e-6 * tol for d in ds)
    ref = FO.train(*inputs, 50, tol)
    assert ref[3] == 2
    got, it, st = _run(monkeypatch, {}, inputs, iters=50, tol=tol)
    assert it == ref[3], (it, ref[3], ds, tol)
    assert st["chunks"] == 1 and st["family"] == "mm", st
    FC.assert_params_match(got, ref[:3], atol=ATOL)


# ---- the stats contract --------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_fit_stats_are_consistent_and_length_checked(gpu, monkeypatch):
    """cv_hmm_fit_last_stats: five words, length-checked like cv_last_fixed_first_stats, the
    calling thread's last call; with no key set a test-sized corpus is one chunk and one pair per
    wave, and a failed call leaves zeros."""
    import cviterbi as cv
    from cviterbi import _lib as L

    inputs, _, _ = FC.case("dense", 20, V, 27, 30, ITERS)
    off = inputs[3]
    _, _, st = _run(monkeypatch, {}, inputs)
    assert st == dict(chunks=1, max_chunk_elems=int(off[-1]), pairs_per_wave_max=1, scratch_batches=0,
                      family="wave", family_code=1), st
    _, _, st = _run(monkeypatch, {"CV_BW_CHUNK_ELEMS": 40, "CV_BW_MAX_WAVES": 2}, inputs)
    chunks, biggest, most = FC.chunk_stats(off, 40)
    assert (st["chunks"], st["max_chunk_elems"], st["pairs_per_wave_max"]) == \
        (chunks, biggest, _ceil_div(_ceil_div(most, 2), 2)), st
    want = [st["chunks"], st["max_chunk_elems"], st["pairs_per_wave_max"], st["scratch_batches"], st["family_code"]]
    out = (ctypes.c_int64 * 7)(*([-7] * 7))
    assert L.lib().cv_hmm_fit_last_stats(out, 2) == 5 and list(out) == want[:2] + [-7] * 5
    assert L.lib().cv_hmm_fit_last_stats(out, 7) == 5 and list(out) == want + [-7] * 2
    assert L.lib().cv_hmm_fit_last_stats(None, 0) == 5
    assert L.lib().cv_hmm_fit_last_stats(None, 3) == -1 and L.lib().cv_hmm_fit_last_stats(out, -1) == -1
    # no E-step: the plan only
    _, it, st = _run(monkeypatch, {"CV_BW_CHUNK_ELEMS": 40}, inputs, iters=0)
    assert it == 0 and (st["chunks"], st["family"], st["pairs_per_wave_max"]) == (chunks, None, 0), st
    # a call that fails its argument check reports nothing of the call before
    bad = inputs[:4] + (np.full_like(inputs[4], V), inputs[5])
    with pytest.raises(cv.CVError):
        cv.fit_train(*bad, max_iter=1, tol=0.0)
    assert set(cv.last_fit_stats().values()) <= {0, None}
