"""GPU: cv_posterior_batch / cv_posterior_batch_device (sequence log-likelihood, posterior state
marginals, posterior decoding) against the 60-digit golden fixtures and, beyond them, the numpy
f64 oracle of tests/test_posterior.py at twice the bounds.  The bounds are derived (u = 2^-53):
  |loglik - ref| <= 2 T (N + 8) u / ln 10 + 4 T u max(1, S)
  |gamma  - ref| <= 4 T (N + 8) u ref + 1e-290,  rows sum to 1 within 4 (N + 8) u
Beyond accuracy: forced tags on every column tile / thread stride, the first-index rule of the
path on exact ties at every merge level of the argmax, bit-identical output modes, statuses
that disturb no neighbour, and the plain kernels' limit N = 4096.
Each test prints its largest error-to-bound ratio (pytest -s)."""
import ctypes
import functools

import numpy as np
import pytest

import cviterbi as cv
from conftest import load_golden
from cviterbi import _lib as L
from test_posterior import (FIXTURES, U, fixture_sequences, gamma_bound, loglik_bound, np_forward_backward,
                            random_model, rowsum_bound)

pytestmark = pytest.mark.gpu


def offsets_of(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def feasible_obs(pi, a, b, lengths, seed):
    """Random observations, redrawn per sequence until the likelihood is positive."""
    rng = np.random.default_rng(seed)
    v = b.shape[1]
    out = []
    for T in lengths:
        while True:
            o = rng.integers(0, v, size=T).astype(np.int32)
            if T == 0 or np_forward_backward(pi, a, b, o)[0] > -np.inf:
                break
        out.append(o)
    return np.concatenate(out) if out else np.zeros(0, np.int32)


def oracle(pi, a, b, off, obs, forced=None):
    res = []
    for k in range(len(off) - 1):
        lo, hi = int(off[k]), int(off[k + 1])
        res.append(np_forward_backward(pi, a, b, obs[lo:hi], None if forced is None else forced[lo:hi]))
    return res


def check(N, off, got, refs, factor=1.0):
    """got = (loglik, path, gamma, status); refs = [(loglik, gamma, S)] per sequence.
    Returns the largest error / bound ratio."""
    loglik, path, gamma, status = got
    worst = 0.0
    for k, (ref_ll, ref_g, ref_S) in enumerate(refs):
        lo, hi = int(off[k]), int(off[k + 1])
        T = hi - lo
        if T == 0:
            continue
        assert status[k] == L.SEQ_OK, (k, status[k])
        assert np.isfinite(loglik[k])
        r = abs(loglik[k] - ref_ll) / (factor * loglik_bound(T, N, ref_S))
        assert r <= 1.0, (k, T, loglik[k], ref_ll, r)
        worst = max(worst, r)
        if gamma is not None:
            g = gamma[lo:hi]
            rg = float(np.max(np.abs(g - ref_g) / (factor * gamma_bound(T, N, ref_g))))
            assert rg <= 1.0, (k, T, rg)
            worst = max(worst, rg)
            assert np.all(np.abs(g.sum(axis=1) - 1.0) <= rowsum_bound(N)), k
            assert np.all(g[ref_g == 0.0] == 0.0), k
        if path is not None:
            p = path[lo:hi]
            assert np.all((p >= 0) & (p < N)), k
            picked = ref_g[np.arange(T), p]
            assert np.all(picked >= ref_g.max(axis=1) * (1 - factor * 4 * T * (N + 8) * U)), k
            if gamma is not None:  # division by the row's positive sum is monotone: the path sits on gamma's own maximum
                assert np.array_equal(gamma[lo:hi][np.arange(T), p], gamma[lo:hi].max(axis=1)), k
    return worst


def viterbi_invariant(h, N, off, obs, loglik, refs, forced=None):
    """viterbi_score - tol <= loglik <= viterbi_score + T log10 N + tol (decode_batch f64)."""
    _, score, st = cv.decode_batch(h, off, obs, dtype="f64", forced=forced)
    for k, (_, _, S) in enumerate(refs):
        T = int(off[k + 1] - off[k])
        if T == 0:
            continue
        assert st[k] == L.SEQ_OK
        tol = 2 * loglik_bound(T, N, S)
        assert score[k] - tol <= loglik[k] <= score[k] + T * np.log10(N) + tol, (k, score[k], loglik[k])


# ---- golden fixtures (60-digit references), both kernels, free and with partial tags ----------------
@pytest.mark.parametrize("kernel", ["auto", "generic"])
@pytest.mark.parametrize("name", FIXTURES)
def test_golden(gpu, name, kernel):
    z = load_golden(name)
    N = len(z["pi"])
    h = cv.HMM(z["pi"], z["a"], z["b"], device=gpu)
    worst = 0.0
    for suffix, forced in (("", None), ("_f", z["forced"])):
        refs = [(z["loglik" + suffix][k], z["gamma" + suffix][lo:hi], z["S" + suffix][k])
                for k, lo, hi in fixture_sequences(z)]
        got = cv.posterior_batch(h, z["offsets"], z["obs"], forced=forced, gamma=True, kernel=kernel)
        t = cv.last_timing(h)
        assert t["padded_states"] == (N + 63) // 64 * 64
        mm = kernel == "auto" and N <= 256
        assert (t["seqs_per_wave"] == 32) == mm and t["kernel"] == ("none" if mm else "generic"), t
        worst = max(worst, check(N, z["offsets"], got, refs))
        ll, st = cv.score_batch(h, z["offsets"], z["obs"], forced=forced, kernel=kernel)
        assert np.array_equal(ll, got[0]) and np.array_equal(st, got[3])  # scoring mode: the same forward pass
        if forced is not None:  # gamma is exactly 0 off a forced state
            f = z["forced"]
            g = got[2]
            for e in np.nonzero(f >= 0)[0]:
                assert g[e, f[e]] == 1.0 and g[e].sum() == 1.0
                assert got[1][e] == f[e]
        viterbi_invariant(h, N, z["offsets"], z["obs"], got[0], refs, forced)
    print(f"{name} {kernel}: error / bound = {worst:.4f}")


def test_long_sequence_is_finite(gpu):
    """N = 4, T = 4096: loglik ~ -4000 (an unscaled forward underflows to -inf)."""
    z = load_golden("posterior_n4_t4096.npz")
    h = cv.HMM(z["pi"], z["a"], z["b"], device=gpu)
    ll, st = cv.score_batch(h, z["offsets"], z["obs"])
    assert st[0] == L.SEQ_OK and np.isfinite(ll[0]) and ll[0] < -3000
    assert abs(ll[0] - z["loglik"][0]) <= loglik_bound(4096, 4, z["S"][0])


# ---- shapes: the matrix-core kernel's tile edges, against the numpy oracle at twice the bounds ---------
@pytest.mark.parametrize("N", [1, 3, 16, 17, 64, 65, 130, 190, 255, 256])
def test_shapes_matrix_core(gpu, N):
    pi, a, b = random_model(N, 4, seed=1000 + N)
    lengths = [33, 1, 2, 5]
    off = offsets_of(lengths)
    obs = feasible_obs(pi, a, b, lengths, seed=N)
    refs = oracle(pi, a, b, off, obs)
    h = cv.HMM(pi, a, b, device=gpu)
    got = {}
    worst = 0.0
    for kernel in ("auto", "generic"):
        got[kernel] = cv.posterior_batch(h, off, obs, gamma=True, kernel=kernel)
        t = cv.last_timing(h)
        assert t["kernel"] == ("generic" if kernel == "generic" else "none") and t["launches"] == 1, t
        assert (t["seqs_per_wave"] == 32) == (kernel == "auto"), t
        worst = max(worst, check(N, off, got[kernel], refs, factor=2.0))
    # the two kernels agree within the bounds (each is within its bound of the exact value)
    fake = [(got["generic"][0][k], got["generic"][2][int(off[k]):int(off[k + 1])], refs[k][2]) for k in range(len(lengths))]
    check(N, off, (got["auto"][0], None, got["auto"][2], got["auto"][3]), fake, factor=2.0)
    viterbi_invariant(h, N, off, obs, got["auto"][0], refs)
    print(f"N={N}: error / (2 x bound) = {worst:.4f}")


@pytest.mark.parametrize("N", [257, 300, 1030])
def test_shapes_plain_kernel(gpu, N):
    pi, a, b = random_model(N, 3, seed=2000 + N)
    lengths = [6, 1, 4]
    off = offsets_of(lengths)
    obs = feasible_obs(pi, a, b, lengths, seed=N)
    refs = oracle(pi, a, b, off, obs)
    h = cv.HMM(pi, a, b, device=gpu)
    got = cv.posterior_batch(h, off, obs, gamma=True)
    assert cv.last_timing(h)["kernel"] == "generic"
    worst = check(N, off, got, refs, factor=2.0)
    viterbi_invariant(h, N, off, obs, got[0], refs)
    print(f"N={N}: error / (2 x bound) = {worst:.4f}")


# ---- batches of mixed lengths: a length-1 sequence shares a group with long ones ----------------------
@pytest.mark.parametrize("N,B", [pytest.param(20, 1, id="1"), pytest.param(20, 33, id="33"), pytest.param(20, 70, id="70"),
                                 pytest.param(130, 33, id="N130-33"), pytest.param(130, 70, id="N130-70"),
                                 pytest.param(256, 33, id="N256-33"), pytest.param(256, 70, id="N256-70")])
def test_mixed_batches_match_single_sequences(gpu, N, B):
    """The discrete entry (emission rows gathered by observation) on several workgroups, the
    longest-first order and a partly filled group, at one column tile and at three and four."""
    pi, a, b = random_model(N, 5, seed=77)
    lengths = [70] if B == 1 else [1 + (37 * k) % 70 for k in range(B)]
    assert B == 1 or (1 in lengths and max(lengths) >= 67)
    off = offsets_of(lengths)
    obs = feasible_obs(pi, a, b, lengths, seed=B)
    h = cv.HMM(pi, a, b, device=gpu)
    got = cv.posterior_batch(h, off, obs, gamma=True)
    refs = oracle(pi, a, b, off, obs)
    worst = check(N, off, got, refs, factor=2.0)
    alone = []
    for k in range(B):
        lo, hi = int(off[k]), int(off[k + 1])
        ll1, p1, g1, s1 = cv.posterior_batch(h, [0, hi - lo], obs[lo:hi], gamma=True)
        assert s1[0] == L.SEQ_OK
        assert np.array_equal(p1, got[1][lo:hi]), k
        alone.append((ll1[0], g1, refs[k][2]))
    check(N, off, (got[0], None, got[2], got[3]), alone)
    print(f"N={N} B={B}: error / (2 x bound) = {worst:.4f}")


# ---- forced tags -----------------------------------------------------------------------------------
def kernels_of(N):
    """The matrix-core kernels and the plain ones where both exist (N <= 256), else the plain ones."""
    return ("auto", "generic") if N <= 256 else ("auto",)


def tag_classes(N):
    """[(name, predicate)]: the kinds of state a set of tags has to reach.  The matrix-core
    kernels hold state j in wave j // (NP / 4), tile (j // 16) % (NP / 64), lane j % 16; the plain
    kernels in thread j % 256 at stride j // 256."""
    NP = (N + 63) // 64 * 64
    cls = []
    if N <= 256:
        for q in range(NP // 64):
            cls.append((f"quarter {q}", lambda j, q=q: j // 64 == q))
    else:
        cls.append(("below 256", lambda j: j < 256))
        cls.append(("256 and above", lambda j: j >= 256))
        if N > 512:
            cls.append(("512 and above", lambda j: j >= 512))
    cls.append(("j % 16 == 0", lambda j: j % 16 == 0))
    cls.append(("j % 16 == 15", lambda j: j % 16 == 15))
    cls.append(("state N - 1", lambda j: j == N - 1))
    return cls


def covering_tags(pi, a, b, off, obs, path, classes):
    """forced[sum T]: tags reaching every class.  A class takes a free element whose state on
    `path` (the decode's) is of the class; if the path visits none, any state of the class with a
    positive emission there that leaves the sequence feasible (numpy oracle)."""
    total = int(off[-1])
    seq_of = np.repeat(np.arange(len(off) - 1), np.diff(off))
    forced = np.full(total, -1, np.int32)
    N = len(pi)

    def exposed(e):
        """Inside its sequence with free neighbours: the tag's mask then shows in the forward
        row of e + 1 and in the backward row of e - 1 (next to another tag, gamma is one-hot anyway)."""
        lo, hi = int(off[seq_of[e]]), int(off[seq_of[e] + 1])
        return lo < e < hi - 1 and forced[e - 1] < 0 and forced[e + 1] < 0

    for name, pred in classes:
        if any(pred(int(j)) for j in forced[forced >= 0]):
            continue
        free = sorted((e for e in range(total) if forced[e] < 0), key=lambda e: (not exposed(e), e))
        cand = [(e, int(path[e])) for e in free if pred(int(path[e]))]
        cand += [(e, j) for e in free for j in range(N) if pred(j) and b[j, obs[e]] > -np.inf]
        for e, j in cand:
            lo, hi = int(off[seq_of[e]]), int(off[seq_of[e] + 1])
            trial = forced.copy()
            trial[e] = j
            if np_forward_backward(pi, a, b, obs[lo:hi], trial[lo:hi])[0] > -np.inf:
                forced = trial
                break
        else:
            raise AssertionError(f"no feasible tag of class '{name}'")
    for e in range(total):  # top up with tags from the path until three tags are exposed
        if sum(exposed(t) for t in np.nonzero(forced >= 0)[0]) >= 3:
            break
        if forced[e] < 0 and exposed(e):
            lo, hi = int(off[seq_of[e]]), int(off[seq_of[e] + 1])
            trial = forced.copy()
            trial[e] = path[e]
            if np_forward_backward(pi, a, b, obs[lo:hi], trial[lo:hi])[0] > -np.inf:
                forced = trial
    for name, pred in classes:  # the coverage the test is about
        assert any(pred(int(j)) for j in forced[forced >= 0]), name
    assert (forced < 0).sum() >= total // 2
    assert sum(exposed(e) for e in np.nonzero(forced >= 0)[0]) >= 3
    return forced


@pytest.mark.parametrize("N", [130, 192, 256, 300, 520])
def test_tags_at_every_tile_and_stride(gpu, N):
    """Partial tags on states of every column tile, both ends of a DPP row, the last state and,
    on the plain kernels, the strides beyond the first 256 states."""
    pi, a, b = random_model(N, 4, seed=4000 + N)
    lengths = [12, 1, 5, 2]
    off = offsets_of(lengths)
    obs = feasible_obs(pi, a, b, lengths, seed=N)
    h = cv.HMM(pi, a, b, device=gpu)
    path, _, st = cv.decode_batch(h, off, obs, dtype="f64")
    assert np.all(st == L.SEQ_OK)
    forced = covering_tags(pi, a, b, off, obs, path, tag_classes(N))
    tagged = np.nonzero(forced >= 0)[0]
    refs = oracle(pi, a, b, off, obs, forced)
    worst = 0.0
    for kernel in kernels_of(N):
        got = cv.posterior_batch(h, off, obs, forced=forced, gamma=True, kernel=kernel)
        t = cv.last_timing(h)
        assert (t["seqs_per_wave"] == 32) == (kernel == "auto" and N <= 256), t
        worst = max(worst, check(N, off, got, refs, factor=2.0))
        onehot = np.zeros((len(tagged), N))
        onehot[np.arange(len(tagged)), forced[tagged]] = 1.0
        assert np.array_equal(got[2][tagged], onehot), kernel
        assert np.array_equal(got[1][tagged], forced[tagged]), kernel
        ll, st = cv.score_batch(h, off, obs, forced=forced, kernel=kernel)
        assert np.array_equal(ll, got[0]) and np.array_equal(st, got[3])
        viterbi_invariant(h, N, off, obs, got[0], refs, forced)
    print(f"N={N}: tags on states {sorted(set(forced[tagged].tolist()))}, error / (2 x bound) = {worst:.4f}")


@pytest.mark.parametrize("N", [17, 130, 256, 300])
def test_all_tags_forced_gives_the_path_score(gpu, N):
    pi, a, b = random_model(N, 5, seed=5)
    lengths = [33, 5, 1]
    off = offsets_of(lengths)
    obs = feasible_obs(pi, a, b, lengths, seed=5)
    h = cv.HMM(pi, a, b, device=gpu)
    path, score, st = cv.decode_batch(h, off, obs, dtype="f64")  # score: the f64 re-score of the path
    assert np.all(st == L.SEQ_OK)
    for kernel in kernels_of(N):
        ll, p, g, s = cv.posterior_batch(h, off, obs, forced=path, gamma=True, kernel=kernel)
        assert np.all(s == L.SEQ_OK) and np.array_equal(p, path)
        for k, T in enumerate(lengths):
            S = np_forward_backward(pi, a, b, obs[off[k]:off[k + 1]], path[off[k]:off[k + 1]])[2]
            assert abs(ll[k] - score[k]) <= loglik_bound(T, N, S), (k, ll[k], score[k])
        onehot = np.zeros_like(g)
        onehot[np.arange(len(path)), path] = 1.0
        assert np.array_equal(g, onehot)


# ---- statuses: infeasible, empty and out-of-range sequences disturb nobody -----------------------------
def test_statuses_and_neighbours(gpu):
    N, V = 5, 4
    pi, a, b = random_model(N, V, seed=9, zero_frac=0.0)
    b[:, 3] = -np.inf  # observation 3 has probability 0 in every state
    good = [np.array([0, 1, 2, 1, 0], np.int32), np.array([2], np.int32), np.array([1, 1, 0, 2, 2, 0, 1], np.int32)]
    seqs = [good[0], np.array([0, 3, 1], np.int32), good[1], np.zeros(0, np.int32), np.array([1, 99, 0, -4], np.int32),
            good[2]]
    off = offsets_of([len(s) for s in seqs])
    obs = np.concatenate(seqs)
    goff = offsets_of([len(s) for s in good])
    h = cv.HMM(pi, a, b, device=gpu)
    for kernel in ("auto", "generic"):
        ll, path, g, st = cv.posterior_batch(h, off, obs, gamma=True, kernel=kernel)
        assert list(st) == [L.SEQ_OK, L.SEQ_INFEASIBLE, L.SEQ_OK, L.SEQ_EMPTY, L.SEQ_BADOBS, L.SEQ_OK]
        assert ll[1] == -np.inf and ll[3] == 0.0 and np.isnan(ll[4])
        for k in (1, 4):
            assert np.all(path[off[k]:off[k + 1]] == -1) and np.all(g[off[k]:off[k + 1]] == 0.0)
        ll2, path2, g2, st2 = cv.posterior_batch(h, goff, np.concatenate(good), gamma=True, kernel=kernel)
        assert np.all(st2 == L.SEQ_OK)
        for k2, k in enumerate((0, 2, 5)):
            assert ll[k] == ll2[k2]
            assert np.array_equal(path[off[k]:off[k + 1]], path2[goff[k2]:goff[k2 + 1]])
            assert np.array_equal(g[off[k]:off[k + 1]], g2[goff[k2]:goff[k2 + 1]])
        check(N, goff, (ll2, path2, g2, st2), oracle(pi, a, b, goff, np.concatenate(good)), factor=2.0)
        sl, ss = cv.score_batch(h, off, obs, kernel=kernel)
        assert np.array_equal(ss, st) and np.array_equal(sl[[0, 1, 2, 3, 5]], ll[[0, 1, 2, 3, 5]])
    # the C call itself reports the infeasible sequence, after writing every output
    o = L.opts(L.DTYPE_F64)
    llc, stc = np.zeros(6), np.zeros(6, np.uint8)
    rc = L.lib().cv_posterior_batch(h.handle, 6, off.ctypes.data, obs.ctypes.data, ctypes.byref(o), llc.ctypes.data,
                                    None, None, stc.ctypes.data)
    assert rc == L.CV_EINFEASIBLE and np.array_equal(stc, st) and llc[0] == ll[0]


def same_sequence(x, y, off, k):
    """Sequence k of two results (loglik, path, gamma, status) is the same bit for bit."""
    lo, hi = int(off[k]), int(off[k + 1])
    assert x[3][k] == y[3][k], k
    assert np.array_equal(x[0][k:k + 1].view(np.int64), y[0][k:k + 1].view(np.int64)), k
    assert np.array_equal(x[1][lo:hi], y[1][lo:hi]), k
    assert np.array_equal(x[2][lo:hi].view(np.int64), y[2][lo:hi].view(np.int64)), k


@pytest.mark.parametrize("N", [130, 300])
def test_a_tag_that_makes_one_sequence_infeasible(gpu, N):
    """40 ragged sequences (two groups of 32 on the matrix-core kernel); state N - 1 emits
    nothing, and one sequence in the middle of the first group is tagged with it."""
    pi, a, b = random_model(N, 4, seed=4100 + N)
    b[N - 1, :] = -np.inf
    B = 40
    lengths = np.array([1 + (11 * k) % 17 for k in range(B)])
    off = offsets_of(lengths)
    obs = feasible_obs(pi, a, b, lengths, seed=N)
    kb = int(np.argsort(-lengths, kind="stable")[16])  # rank 16 of the longest-first order
    assert lengths[kb] >= 3
    free = np.full(int(off[-1]), -1, np.int32)
    forced = free.copy()
    forced[off[kb] + 1] = N - 1
    h = cv.HMM(pi, a, b, device=gpu)
    for kernel in kernels_of(N):
        clean = cv.posterior_batch(h, off, obs, forced=free, gamma=True, kernel=kernel)
        assert np.all(clean[3] == L.SEQ_OK)
        got = cv.posterior_batch(h, off, obs, forced=forced, gamma=True, kernel=kernel)
        assert got[3][kb] == L.SEQ_INFEASIBLE and got[0][kb] == -np.inf
        assert np.all(got[1][off[kb]:off[kb + 1]] == -1) and np.all(got[2][off[kb]:off[kb + 1]] == 0.0)
        for k in range(B):
            if k != kb:
                same_sequence(got, clean, off, k)
        ll, st = cv.score_batch(h, off, obs, forced=forced, kernel=kernel)
        assert np.array_equal(st, got[3]) and np.array_equal(ll, got[0])
        # the C call reports the infeasible sequence, after writing every output
        o = L.opts(L.DTYPE_F64, L.ASSOC_VITERBI, L.KERNEL_GENERIC if kernel == "generic" else L.KERNEL_AUTO)
        o.forced = forced.ctypes.data
        llc, stc, pc = np.zeros(B), np.zeros(B, np.uint8), np.zeros(int(off[-1]), np.int32)
        rc = L.lib().cv_posterior_batch(h.handle, B, off.ctypes.data, obs.ctypes.data, ctypes.byref(o), llc.ctypes.data,
                                        pc.ctypes.data, None, stc.ctypes.data)
        assert rc == L.CV_EINFEASIBLE
        assert np.array_equal(stc, got[3]) and np.array_equal(llc, got[0]) and np.array_equal(pc, got[1])
    check(N, off, clean, oracle(pi, a, b, off, obs), factor=2.0)


def test_a_bad_observation_at_wide_N(gpu):
    """The range check of the observation runs on the device: the sequence is BADOBS, its 32
    neighbours in the group and the other groups are unchanged bit for bit."""
    N = 130
    h, off, obs, refs = _mixed(gpu, N)
    kb = 7
    assert off[kb + 1] - off[kb] >= 3
    bad = obs.copy()
    bad[off[kb] + 1] = 5  # the model has observations 0 .. 4
    for kernel in ("auto", "generic"):
        clean = cv.posterior_batch(h, off, obs, gamma=True, kernel=kernel)
        got = cv.posterior_batch(h, off, bad, gamma=True, kernel=kernel)
        assert got[3][kb] == L.SEQ_BADOBS and np.isnan(got[0][kb])
        assert np.all(got[1][off[kb]:off[kb + 1]] == -1) and np.all(got[2][off[kb]:off[kb + 1]] == 0.0)
        for k in range(len(off) - 1):
            if k != kb:
                same_sequence(got, clean, off, k)
        check(N, off, clean, refs, factor=2.0)


# ---- the documented tie rule: path = the FIRST index of the maximum ------------------------------------
def copies_model(N, M, seed):
    """N / M copies of an M-state model: state j behaves as state j % M, and the mass of base
    state j is split evenly, so columns and rows j, j + M, ... of A are identical and the exact
    marginals of the copies tie."""
    pi0, a0, b0 = random_model(M, 4, seed=seed)
    c = N // M
    assert c * M == N and c >= 2
    idx = np.arange(N) % M
    return pi0[idx] - np.log10(c), a0[np.ix_(idx, idx)] - np.log10(c), b0[idx].copy()


TIE_CASES = [(64, 4), (64, 16), (192, 48), (256, 4), (256, 16), (256, 64), (512, 8), (512, 64), (512, 256)]


@pytest.mark.parametrize("N,M", TIE_CASES)
def test_path_is_the_first_index_on_exact_ties(gpu, N, M):
    """The copies j, j + M, ... of a state tie exactly: the kernels' sums run in an order that
    does not depend on the column, so their p = alpha o beta tie bit for bit (asserted), and the
    path must name the first copy.  M puts the tied columns in one lane's registers, in the lanes
    of a DPP row and in different waves (matrix-core kernels), or in one thread's strided states,
    in one wave's shuffle tree and in different waves (plain kernels)."""
    pi, a, b = copies_model(N, M, seed=6000 + N + M)
    lengths = [20, 3]
    off = offsets_of(lengths)
    obs = feasible_obs(pi, a, b, lengths, seed=N + M)
    h = cv.HMM(pi, a, b, device=gpu)
    refs = oracle(pi, a, b, off, obs)
    for r in refs:  # the oracle's own sums are column-independent too
        assert np.array_equal(r[1][:, :M], r[1][:, M:2 * M])
    e_tag = 9
    for kernel in kernels_of(N):
        got = cv.posterior_batch(h, off, obs, gamma=True, kernel=kernel)
        check(N, off, got, refs, factor=2.0)
        g = got[2]
        for c in range(1, N // M):
            assert np.array_equal(g[:, :M].view(np.int64), g[:, c * M:(c + 1) * M].view(np.int64)), (kernel, c)
        assert np.all(got[1] < M), (kernel, got[1])
        only_path = cv.posterior_batch(h, off, obs, gamma=False, kernel=kernel)
        assert np.array_equal(only_path[1], got[1])
        # a tag on a later copy: the path is that copy there and the first copy everywhere else
        forced = np.full(int(off[-1]), -1, np.int32)
        forced[e_tag] = got[1][e_tag] + (N // M - 1) * M
        tg = cv.posterior_batch(h, off, obs, forced=forced, gamma=True, kernel=kernel)
        assert np.all(tg[3] == L.SEQ_OK)
        assert tg[1][e_tag] == forced[e_tag] and tg[2][e_tag, forced[e_tag]] == 1.0 and tg[2][e_tag].sum() == 1.0
        rest = np.arange(int(off[-1])) != e_tag
        for c in range(1, N // M):
            assert np.array_equal(tg[2][rest][:, :M].view(np.int64), tg[2][rest][:, c * M:(c + 1) * M].view(np.int64)), (kernel, c)
        assert np.all(tg[1][rest] < M), (kernel, tg[1])
        check(N, off, tg, oracle(pi, a, b, off, obs, forced), factor=2.0)


# ---- output modes: every subset of the outputs is the same computation -----------------------------------
@pytest.mark.parametrize("N", [20, 130, 256, 300])
def test_output_modes_are_bit_identical(gpu, N):
    h, off, obs, refs = _mixed(gpu, N)
    for kernel in kernels_of(N):
        both = cv.posterior_batch(h, off, obs, gamma=True, kernel=kernel)
        check(N, off, both, refs, factor=2.0)
        ll, path, g, st = cv.posterior_batch(h, off, obs, gamma=False, kernel=kernel)
        assert g is None and np.array_equal(path, both[1])
        assert np.array_equal(ll, both[0]) and np.array_equal(st, both[3])
        ll, path, g, st = cv.posterior_batch(h, off, obs, gamma=True, path=False, kernel=kernel)
        assert path is None and np.array_equal(g.view(np.int64), both[2].view(np.int64))
        assert np.array_equal(ll, both[0]) and np.array_equal(st, both[3])
        ll, st = cv.score_batch(h, off, obs, kernel=kernel)
        assert np.array_equal(ll, both[0]) and np.array_equal(st, both[3])


def test_output_modes_of_the_device_variant(gpu):
    import torch

    N = 130
    h, off, obs, _ = _mixed(gpu, N)
    both = cv.posterior_batch(h, off, obs, gamma=True)
    dev = torch.device("cuda", gpu)
    total, B = int(off[-1]), len(off) - 1
    d_off, d_obs = torch.from_numpy(off).to(dev), torch.from_numpy(obs).to(dev)
    for want_path, want_gamma in ((True, False), (False, True)):
        d_ll = torch.zeros(B, dtype=torch.float64, device=dev)
        d_st = torch.full((B,), 9, dtype=torch.uint8, device=dev)
        d_path = torch.full((total,), -7, dtype=torch.int32, device=dev) if want_path else None
        d_gamma = torch.full((total, N), 7.0, dtype=torch.float64, device=dev) if want_gamma else None
        torch.cuda.synchronize(dev)
        cv.posterior_batch_device(h, d_off, d_obs, d_ll, d_st, d_path, d_gamma, offsets_host=off)
        torch.cuda.synchronize(dev)
        assert np.array_equal(d_ll.cpu().numpy(), both[0]) and np.array_equal(d_st.cpu().numpy(), both[3])
        if want_path:
            assert np.array_equal(d_path.cpu().numpy(), both[1])
        if want_gamma:
            assert np.array_equal(d_gamma.cpu().numpy().view(np.int64), both[2].view(np.int64))


# ---- a long sequence beside short ones at four column tiles ----------------------------------------------
def test_long_beside_short_at_n256(gpu):
    """The short sequences ride masked for ~300 steps of the group; the ring of prefetched
    observations and the exponent sum run long."""
    N = 256
    pi, a, b = random_model(N, 4, seed=4256)
    lengths = [300, 1, 299, 2]
    off = offsets_of(lengths)
    obs = feasible_obs(pi, a, b, lengths, seed=256)
    refs = oracle(pi, a, b, off, obs)
    h = cv.HMM(pi, a, b, device=gpu)
    worst = 0.0
    for kernel in ("auto", "generic"):
        got = cv.posterior_batch(h, off, obs, gamma=True, kernel=kernel)
        worst = max(worst, check(N, off, got, refs, factor=2.0))
    print(f"N=256, T=300/1/299/2: error / (2 x bound) = {worst:.4f}")


# ---- the plain kernels' LDS limit: NP > 3072 raises the dynamic-LDS cap, N = 4096 is the advertised end ------
@pytest.mark.parametrize("N", [3073, 4096])
def test_lds_limit(gpu, N):
    pi, a, b = random_model(N, 2, seed=N)
    lengths = [3, 1, 2]
    off = offsets_of(lengths)
    obs = np.random.default_rng(N).integers(0, 2, size=6).astype(np.int32)
    forced = np.full(6, -1, np.int32)
    forced[1] = N - 1
    obs[1] = int(np.argmax(b[N - 1]))  # an observation state N - 1 emits
    refs = oracle(pi, a, b, off, obs, forced)
    assert all(np.isfinite(r[0]) for r in refs)
    h = cv.HMM(pi, a, b, device=gpu)
    got = cv.posterior_batch(h, off, obs, forced=forced, gamma=True)
    t = cv.last_timing(h)
    assert t["kernel"] == "generic" and t["padded_states"] == (N + 63) // 64 * 64, t
    worst = check(N, off, got, refs, factor=2.0)
    assert got[1][1] == N - 1 and got[2][1, N - 1] == 1.0 and got[2][1].sum() == 1.0
    ll, st = cv.score_batch(h, off, obs, forced=forced)
    assert cv.last_timing(h)["kernel"] == "generic"
    assert np.array_equal(ll, got[0]) and np.array_equal(st, got[3])
    print(f"N={N}: error / (2 x bound) = {worst:.4f}")


# ---- workspace chunks, the device variant, repeats, memory -------------------------------------------
@functools.lru_cache(maxsize=None)
def _mixed_case(N, B):
    """(pi, a, b, off, obs, refs) -- shared among the tests and never modified."""
    pi, a, b = random_model(N, 5, seed=31)
    lengths = [1 + (37 * k) % 70 for k in range(B)]
    off = offsets_of(lengths)
    obs = feasible_obs(pi, a, b, lengths, seed=31)
    for x in (pi, a, b):
        x.setflags(write=False)
    return pi, a, b, off, obs, oracle(pi, a, b, off, obs)


def _mixed(gpu, N=20, B=33):
    pi, a, b, off, obs, refs = _mixed_case(N, B)
    return cv.HMM(pi, a, b, device=gpu), off, obs, refs


@pytest.mark.parametrize("N", [20, 130, 256])
def test_small_workspace_chunks(gpu, N):
    h, off, obs, refs = _mixed(gpu, N)
    whole = cv.posterior_batch(h, off, obs, gamma=True)
    assert cv.last_timing(h)["launches"] == 1
    NP = (N + 63) // 64 * 64
    chunked = cv.posterior_batch(h, off, obs, gamma=True, workspace_bytes=NP * 8 * 300)
    assert cv.last_timing(h)["launches"] >= 3
    check(N, off, chunked, refs, factor=2.0)
    same = [(whole[0][k], whole[2][int(off[k]):int(off[k + 1])], refs[k][2]) for k in range(len(refs))]
    check(N, off, (chunked[0], None, chunked[2], chunked[3]), same)
    assert np.array_equal(chunked[1], whole[1])


def test_device_variant_and_repeat_are_bit_identical(gpu):
    import torch

    h, off, obs, _ = _mixed(gpu)
    first = cv.posterior_batch(h, off, obs, gamma=True)
    again = cv.posterior_batch(h, off, obs, gamma=True)
    for x, y in zip(first, again):
        assert np.array_equal(x, y)
    dev = torch.device("cuda", gpu)
    total, B, N = int(off[-1]), len(off) - 1, 20
    d_off, d_obs = torch.from_numpy(off).to(dev), torch.from_numpy(obs).to(dev)
    d_ll = torch.zeros(B, dtype=torch.float64, device=dev)
    d_path = torch.zeros(total, dtype=torch.int32, device=dev)
    d_gamma = torch.zeros(total, N, dtype=torch.float64, device=dev)
    d_st = torch.zeros(B, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    for host_off in (off, None):
        cv.posterior_batch_device(h, d_off, d_obs, d_ll, d_st, d_path, d_gamma, offsets_host=host_off,
                                  stream=stream.cuda_stream)
        stream.synchronize()
        assert np.array_equal(d_ll.cpu().numpy(), first[0])
        assert np.array_equal(d_path.cpu().numpy(), first[1])
        assert np.array_equal(d_gamma.cpu().numpy(), first[2])
        assert np.array_equal(d_st.cpu().numpy(), first[3])
        d_ll.zero_(), d_path.zero_(), d_gamma.zero_()
        torch.cuda.synchronize(dev)
    # scoring mode on the device: the same log-likelihoods
    cv.posterior_batch_device(h, d_off, d_obs, d_ll, d_st, offsets_host=off, stream=stream.cuda_stream)
    stream.synchronize()
    assert np.array_equal(d_ll.cpu().numpy(), first[0])
    t = cv.last_timing(h)
    assert t["fwd_ms"] > 0 and t["launches"] == 1


def test_timing_and_release_workspaces(gpu):
    N = 20
    h, off, obs, _ = _mixed(gpu, N)
    cv.posterior_batch(h, off, obs)
    t = cv.last_timing(h)
    assert t["fwd_ms"] > 0 and t["bt_ms"] > 0 and t["total_ms"] >= t["fwd_ms"]
    rows_bytes = int(off[-1]) * 64 * 8  # the stored forward rows: NP = 64 doubles per element
    before = cv.device_memory()["current"]
    h.release_workspaces()
    after = cv.device_memory()["current"]
    assert before - after >= rows_bytes, (before, after, rows_bytes)
    ll, st = cv.score_batch(h, off, obs)  # the tables stayed; scoring mode stores no rows
    assert np.all(st == L.SEQ_OK)
    assert cv.device_memory()["current"] - after < rows_bytes
    h.release_workspaces()


def test_argument_errors(gpu):
    pi, a, b = random_model(4, 3, seed=1)
    h = cv.HMM(pi, a, b, device=gpu)
    off, obs = [0, 3], np.array([0, 1, 2], np.int32)

    def status_of(**kw):
        with pytest.raises(cv.CVError) as e:
            cv.posterior_batch(h, off, obs, **kw)
        return e.value.status

    assert status_of(dtype="f32") == L.CV_EUNSUPPORTED
    assert status_of(kernel="trellis") == L.CV_EINVAL
    assert status_of(kernel="trellis_f64") == L.CV_EINVAL
    assert status_of(forced=np.array([0, 7, -1], np.int32)) == L.CV_EINVAL
    st8, o64 = np.zeros(1, np.uint8), np.array(off, np.int64)
    assert L.lib().cv_posterior_batch(h.handle, 1, o64.ctypes.data, obs.ctypes.data, None, None, None, None,
                                      st8.ctypes.data) == L.CV_EINVAL
    big = 4097  # one state above the limit
    hb = cv.HMM(np.full(big, -np.log10(big)), np.full((big, big), -np.log10(big)), np.zeros((big, 1)), device=gpu)
    with pytest.raises(cv.CVError) as e:
        cv.score_batch(hb, [0, 2], np.zeros(2, np.int32))
    assert e.value.status == L.CV_EUNSUPPORTED
    ll, st = cv.score_batch(h, off, obs)  # the handle still works after the errors
    assert st[0] in (L.SEQ_OK, L.SEQ_INFEASIBLE)
