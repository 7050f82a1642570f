"""Sparse low-word planes of the f64 trellis rows (tuning key t64_lo_every).

With t64_lo_every = K > 1 the forward pass writes the low plane of a delta row only at rows
r % K == 0 and at the last row; at a near tie on another row the backtrack's sparse resolver
recomputes the few exact values it needs (tests/test_sparse_lo_model.py describes and models
it), or replays the rows densely when a need-set exceeds its cap.  Every decode here must equal,
bit for bit, the same decode at t64_lo_every = 1 (every row full: the parent behaviour) and the
C oracle's f64 row-A0 decode: paths, score bits and statuses.
"""
import numpy as np
import pytest

import c_oracle as O
import cviterbi as cv
from cviterbi import synth

pytestmark = pytest.mark.gpu

KS = [2, 8, 16]
NS = [100, 192, 256]


def _assert_same(got, ref, what):
    gp, gs, gst = got
    rp, rs, rst = ref
    assert np.array_equal(gst, rst), f"{what}: status {gst} vs {rst}"
    assert np.array_equal(np.asarray(gs).view(np.uint64), np.asarray(rs, np.float64).view(np.uint64)), \
        f"{what}: score bits differ at {np.nonzero(gs != rs)[0][:8]}"
    assert np.array_equal(gp, rp), f"{what}: paths differ at {np.nonzero(gp != rp)[0][:8]}"


def _dirichlet(n, v, seed):
    return synth.random_hmm(n, v, seed=seed)


def _near_ties(n, v, seed):
    """test_t64_backtrack_interval_paths' near_ties model: transitions and emissions that differ
    below f32 resolution, so the threshold test finds several survivors at most steps."""
    rng = np.random.default_rng(seed)
    pi = np.round(rng.uniform(-2, 0, n) * 4) / 4
    a = np.round(rng.uniform(-2, 0, (n, n)) * 4) / 4 - rng.uniform(0, 1e-12, (n, n))
    b = np.round(rng.uniform(-2, 0, (n, v)) * 4) / 4 - rng.uniform(0, 1e-12, (n, v))
    return pi, a, b


def _dyadic(n, v, seed):
    """Three values, multiples of 1/4: every add is exact, so ties are exact and many, and
    need-sets overflow."""
    rng = np.random.default_rng(seed)
    q = lambda shape: -rng.integers(0, 3, size=shape) / 4.0  # noqa: E731
    return q(n), q((n, n)), q((n, v))


def _infs(n, v, seed):
    """golden_inf.npz's construction at size n: banded transitions, half the emissions and half
    of pi impossible -- infeasible sequences among feasible ones."""
    pi, a, b = synth.random_hmm(n, v, seed=seed)
    i, j = np.indices((n, n))
    a[(j - i) % n > 3] = -np.inf
    rng = np.random.default_rng(seed)
    b[rng.random((n, v)) < 0.5] = -np.inf
    pi[::2] = -np.inf
    return pi, a, b


def _ragged(K, v, seed, extra=40):
    """Lengths 1, 2, K, K+1, 2K+1 and 40 (and an empty sequence) mixed into a ragged batch of
    at most 64 sequences."""
    rng = np.random.default_rng(seed)
    lengths = np.concatenate([[1, 2, K, K + 1, 2 * K + 1, 40, 0], rng.integers(1, 41, size=extra)])
    rng.shuffle(lengths)
    off = synth.offsets_from_lengths(lengths)
    return off, rng.integers(0, v, size=int(off[-1])).astype(np.int32)


def _both(h, off, obs, K, what, ref=None):
    """Decode at lo_every = K and at 1; both equal each other and the oracle.  Returns the
    sparse call's stats."""
    h.set_tuning(t64_lo_every=K)
    got = cv.decode_batch(h, off, obs, dtype="f64", rescore_f64=False)
    st = cv.last_t64_stats(h)
    assert cv.last_timing(h)["kernel"] == "trellis_f64"
    h.set_tuning(t64_lo_every=1)
    full = cv.decode_batch(h, off, obs, dtype="f64", rescore_f64=False)
    assert cv.last_t64_stats(h)["lo_every"] == 1
    _assert_same(got, full, f"{what}: lo_every={K} vs 1")
    if ref is not None:
        _assert_same(got, ref, f"{what}: lo_every={K} vs the oracle")
    assert st["mismatches"] == 0, st
    return st


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("K", KS)
def test_dirichlet_ragged(gpu, n, K):
    pi, a, b = _dirichlet(n, 23, seed=300 + n)
    off, obs = _ragged(K, 23, seed=n + K)
    ref = O.decode_batch(pi, a, b, off, obs, O.VITERBI, np.float64)
    st = _both(cv.HMM(pi, a, b), off, obs, K, f"dirichlet N={n}", ref)
    assert st["lo_every"] == K and st["sequences"] == len(off) - 1, st


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("K", KS)
def test_near_ties_resolver_descends(gpu, n, K):
    pi, a, b = _near_ties(n, 17, seed=900 + n)
    off, obs = _ragged(K, 17, seed=2 * n + K)
    ref = O.decode_batch(pi, a, b, off, obs, O.VITERBI, np.float64)
    st = _both(cv.HMM(pi, a, b), off, obs, K, f"near ties N={n}", ref)
    assert st["lo_every"] == K and st["events"] > 0 and st["levels"] > 0 and st["scans"] > 0, st


@pytest.mark.parametrize("n", NS)
def test_dyadic_dense_replay_and_sticky_guard(gpu, n):
    """Exact ties overflow the need-sets: the dense replay decides (overflows > 0).  More than
    one replay per 64 sequences then pins the handle to full rows: the next call reports
    lo_every = 1, with the same results."""
    pi, a, b = _dyadic(n, 5, seed=70 + n)
    off, obs = _ragged(8, 5, seed=n)
    ref = O.decode_batch(pi, a, b, off, obs, O.VITERBI, np.float64)
    h = cv.HMM(pi, a, b)
    h.set_tuning(t64_lo_every=8)
    got = cv.decode_batch(h, off, obs, dtype="f64", rescore_f64=False)
    st = cv.last_t64_stats(h)
    _assert_same(got, ref, f"dyadic N={n}")
    assert st["lo_every"] == 8 and st["overflows"] > 0 and st["mismatches"] == 0, st
    assert st["overflows"] * 64 > st["sequences"], st
    again = cv.decode_batch(h, off, obs, dtype="f64", rescore_f64=False)
    st2 = cv.last_t64_stats(h)
    assert st2["lo_every"] == 1 and st2["events"] == 0, st2
    _assert_same(again, ref, f"dyadic N={n}, after the guard")
    assert h.tuning("t64_lo_every") == 8  # the key is the caller's; the guard is the handle's


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("K", [2, 8])
def test_infinite_entries_and_infeasible_sequences(gpu, n, K):
    pi, a, b = _infs(n, 8, seed=13 + n)
    b[:, 7] = -np.inf  # observation 7 is impossible: it ends every sixth sequence
    off, obs = _ragged(K, 7, seed=3 * n + K)
    for s in range(0, len(off) - 1, 6):
        if off[s + 1] > off[s]:
            obs[off[s + 1] - 1] = 7
    ref = O.decode_batch(pi, a, b, off, obs, O.VITERBI, np.float64)
    assert (ref[2] == 1).any() and (ref[2] == 0).any()
    _both(cv.HMM(pi, a, b), off, obs, K, f"-inf N={n}", ref)


def _equal_batch(n, v, nseq, T, seed, near):
    pi, a, b = (_near_ties if near else _dirichlet)(n, v, seed)
    off = np.arange(nseq + 1, dtype=np.int64) * T
    return pi, a, b, off, synth.iid_obs(v, nseq * T, seed)


@pytest.mark.parametrize("n,near", [(256, True), (192, False)])
def test_eight_wave_layout(gpu, n, near):
    """Equal lengths and enough sequences for 8 per wave (t64_wg_force = 1: the eight-wave
    workgroups whatever the device's size), T = 19: full rows 0, 8, 16 and the last."""
    nseq, T = 16384, 19
    pi, a, b, off, obs = _equal_batch(n, 11, nseq, T, seed=5 + n, near=near)
    h = cv.HMM(pi, a, b)
    h.set_tuning(t64_wg_force=1, t64_s=8)
    st = _both(h, off, obs, 8, f"eight waves N={n}")
    assert cv.last_timing(h)["seqs_per_wave"] == 8
    assert st["lo_every"] == 8 and (st["events"] > 0 or not near), st
    k = 256  # the oracle on a slice (its sequences are independent)
    sub = cv.decode_batch(h, off[:k + 1], obs[:k * T], dtype="f64", rescore_f64=False)
    ref = O.decode_batch(pi, a, b, off[:k + 1], obs[:k * T], O.VITERBI, np.float64)
    _assert_same(sub, ref, f"eight waves N={n} vs the oracle")


def test_row_split_layout(gpu):
    """N = 256, a batch of 4 sequences per wave: the row-split pairs (trellis_fwd_f64_rs)."""
    nseq, T = 1024, 21
    pi, a, b, off, obs = _equal_batch(256, 11, nseq, T, seed=77, near=True)
    for K in (2, 8):  # a handle each: near-tie models may trip the first handle's guard
        h = cv.HMM(pi, a, b)
        h.set_tuning(t64_s=4, t64_wg_force=1)
        st = _both(h, off, obs, K, "row split")
        assert st["lo_every"] == K and st["events"] > 0 and st["levels"] > 0, st
    k = 128
    h = cv.HMM(pi, a, b)
    h.set_tuning(t64_s=4, t64_wg_force=1, t64_lo_every=8)
    sub = cv.decode_batch(h, off[:k + 1], obs[:k * T], dtype="f64", rescore_f64=False)
    ref = O.decode_batch(pi, a, b, off[:k + 1], obs[:k * T], O.VITERBI, np.float64)
    _assert_same(sub, ref, "row split vs the oracle")


def test_other_paths_keep_full_rows(gpu):
    """The DPSolver / viterbi::decode associations and N <= 64 run with every row full whatever
    the key says."""
    pi, a, b = _near_ties(100, 9, seed=4)
    off, obs = _ragged(8, 9, seed=4)
    h = cv.HMM(pi, a, b)
    h.set_tuning(t64_lo_every=8)
    for assoc, code in (("dp", O.DP), ("decode", O.DECODE)):
        got = cv.decode_batch(h, off, obs, dtype="f64", assoc=assoc, rescore_f64=False)
        assert cv.last_t64_stats(h)["lo_every"] == 1
        _assert_same(got, O.decode_batch(pi, a, b, off, obs, code, np.float64), assoc)
    pi, a, b = _near_ties(48, 9, seed=5)
    h = cv.HMM(pi, a, b)
    h.set_tuning(t64_lo_every=8)
    got = cv.decode_batch(h, off, obs, dtype="f64", rescore_f64=False)
    assert cv.last_t64_stats(h)["lo_every"] == 1
    _assert_same(got, O.decode_batch(pi, a, b, off, obs, O.VITERBI, np.float64), "N=48")


def test_stats_call_is_length_checked(gpu):
    import ctypes

    from cviterbi import _lib as L

    pi, a, b = _dirichlet(100, 9, seed=1)
    off, obs = _ragged(8, 9, seed=1)
    h = cv.HMM(pi, a, b)
    cv.decode_batch(h, off, obs, dtype="f64", rescore_f64=False)
    out = (ctypes.c_int64 * 12)(*([-7] * 12))
    n = L.lib().cv_last_t64_stats(h.handle, out, 3)
    assert n == 8 and list(out[3:]) == [-7] * 9 and out[0] == h.tuning("t64_lo_every")
    assert L.lib().cv_last_t64_stats(h.handle, out, 12) == n and out[n] == -7
    assert L.lib().cv_last_t64_stats(h.handle, None, 0) == n
