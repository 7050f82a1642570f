"""GPU: cv_posterior_batch / cv_posterior_batch_device (sequence log-likelihood, posterior state
marginals, posterior decoding) against the 60-digit golden fixtures and, beyond them, the numpy
f64 oracle of tests/test_posterior.py at twice the bounds.  The bounds are derived (u = 2^-53):
  |loglik - ref| <= 2 T (N + 8) u / ln 10 + 4 T u max(1, S)
  |gamma  - ref| <= 4 T (N + 8) u ref + 1e-290,  rows sum to 1 within 4 (N + 8) u
Each test prints its largest error-to-bound ratio (pytest -s)."""
import ctypes

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
        assert (t["seqs_per_wave"] == 32) == (kernel == "auto"), t
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
@pytest.mark.parametrize("B", [1, 33, 70])
def test_mixed_batches_match_single_sequences(gpu, B):
    N = 20
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
    print(f"B={B}: error / (2 x bound) = {worst:.4f}")


# ---- forced tags -----------------------------------------------------------------------------------
def test_all_tags_forced_gives_the_path_score(gpu):
    N = 17
    pi, a, b = random_model(N, 5, seed=5)
    lengths = [33, 5, 1]
    off = offsets_of(lengths)
    obs = feasible_obs(pi, a, b, lengths, seed=5)
    h = cv.HMM(pi, a, b, device=gpu)
    path, score, st = cv.decode_batch(h, off, obs, dtype="f64")  # score: the f64 re-score of the path
    assert np.all(st == L.SEQ_OK)
    for kernel in ("auto", "generic"):
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


# ---- workspace chunks, the device variant, repeats, memory -------------------------------------------
def _mixed(gpu, N=20, B=33):
    pi, a, b = random_model(N, 5, seed=31)
    lengths = [1 + (37 * k) % 70 for k in range(B)]
    off = offsets_of(lengths)
    obs = feasible_obs(pi, a, b, lengths, seed=31)
    return cv.HMM(pi, a, b, device=gpu), off, obs, oracle(pi, a, b, off, obs)


def test_small_workspace_chunks(gpu):
    N = 20
    h, off, obs, refs = _mixed(gpu, N)
    whole = cv.posterior_batch(h, off, obs, gamma=True)
    assert cv.last_timing(h)["launches"] == 1
    chunked = cv.posterior_batch(h, off, obs, gamma=True, workspace_bytes=64 * 8 * 300)
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
