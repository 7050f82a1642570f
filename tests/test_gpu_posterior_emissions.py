"""GPU: cv_posterior_emissions / cv_posterior_emissions_device (log-likelihood, state marginals
and the posterior path under caller-supplied emission scores) against the 60-digit fixtures of
tools/make_posterior_emissions_golden.py at the derived bounds and, beyond them, the numpy f64
oracle of tests/test_posterior.py on the substituted model b[j][e] = E[e][j], obs[e] = e, at twice
the bounds (as tests/test_gpu_posterior.py does).  The bounds are those of cv_posterior_batch
with N + 8 read as N + 6 + c, c = 2 the worst case of one staged entry (exp10_scaled.h), so
check()'s factor (N + 6 + c) / (N + 8) is 1.  Each test prints its largest error / bound ratio."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import cviterbi as cv
from conftest import load_golden
from cviterbi import _lib as L
from emis_ref import as_discrete, model, offsets_of
from test_gpu_posterior import check, covering_tags, kernels_of, tag_classes
from test_posterior import U, gamma_bound, loglik_bound, np_forward_backward, random_model, rowsum_bound
from test_posterior_emissions import C, FIXTURES

pytestmark = pytest.mark.gpu


def factor(N):
    return (N + 6 + C) / (N + 8)


def oracle(pi, a, E, off, forced=None):
    """[(loglik, gamma, S)] per sequence: np_forward_backward on the substituted model."""
    b, obs = as_discrete(E, len(pi))
    return [np_forward_backward(pi, a, b, obs[lo:hi], None if forced is None else forced[lo:hi])
            for lo, hi in zip(off[:-1], off[1:])]


def feasible_scores(N, lengths, seed, ninf_frac=0.1, scale=3.0):
    """E [sum T, N] ~ normal(0, scale) with -inf entries; every row keeps a finite entry (with the
    dense A of emis_ref.model every sequence is then feasible)."""
    rng = np.random.default_rng(seed)
    total = int(sum(lengths))
    E = rng.normal(0.0, scale, size=(total, N))
    hole = rng.random(E.shape) < ninf_frac
    hole[np.arange(total), rng.integers(0, N, size=total)] = False
    E[hole] = -np.inf
    return E


def ragged(B):
    """B lengths with 0, 1 and 2 among them (B >= 3), else one sequence."""
    return [9] if B == 1 else [(5, 0, 1, 2, 7, 3, 12)[k % 7] for k in range(B)]


def on_device(h, off, E_dev, gamma=True, path=True, forced=None, **kw):
    """posterior_emissions_device on a torch tensor (or a strided view of one) -> numpy results."""
    dev = E_dev.device
    total, nseq, N = int(off[-1]), len(off) - 1, h.nstates()
    off_d = torch.from_numpy(np.ascontiguousarray(off)).to(dev)
    ll = torch.full((max(nseq, 1),), 77.0, dtype=torch.float64, device=dev)
    st = torch.full((max(nseq, 1),), 9, dtype=torch.uint8, device=dev)
    p = torch.full((max(total, 1),), -7, dtype=torch.int32, device=dev) if path else None
    g = torch.full((max(total, 1), N), 7.0, dtype=torch.float64, device=dev) if gamma else None
    if forced is not None:
        kw["forced_dev"] = torch.from_numpy(np.ascontiguousarray(forced, np.int32)).to(dev)
    torch.cuda.synchronize(dev)
    cv.posterior_emissions_device(h, off_d, E_dev, ll, st, p, g, offsets_host=off, **kw)
    torch.cuda.synchronize(dev)
    return (ll.cpu().numpy()[:nseq], p.cpu().numpy()[:total] if path else None,
            g.cpu().numpy()[:total] if gamma else None, st.cpu().numpy()[:nseq])


def same_bits(x, y, what=""):
    for name, u, v in zip(("loglik", "path", "gamma", "status"), x, y):
        if u is None or v is None:
            assert u is None and v is None, (what, name)
            continue
        assert u.shape == v.shape and u.dtype == v.dtype, (what, name)
        assert np.array_equal(u.view(np.uint8), v.view(np.uint8)), (what, name, np.argwhere(u != v)[:5])


# ---- golden fixtures (60-digit references), both kernels, free and with the partial tags ------------
@pytest.mark.parametrize("kernel", ["auto", "generic"])
@pytest.mark.parametrize("name", FIXTURES)
def test_golden(gpu, name, kernel):
    z = load_golden(name)
    N, off, E = len(z["pi"]), z["offsets"], z["E"]
    rows = z["gamma_rows"]
    full = len(rows) == len(E)
    h = cv.HMM(z["pi"], z["a"], model(N)[2], device=gpu)  # the handle's own b is ignored
    worst = 0.0
    for suffix, forced in (("", None), ("_f", z["forced"])):
        got = cv.posterior_emissions(h, off, E, forced=forced, gamma=True, kernel=kernel)
        t = cv.last_timing(h)
        assert t["padded_states"] == (N + 63) // 64 * 64
        assert (t["seqs_per_wave"] == 32) == (kernel == "auto"), t
        ref_g = z["gamma" + suffix]
        if full:
            refs = [(z["loglik" + suffix][k], ref_g[lo:hi], z["S" + suffix][k])
                    for k, (lo, hi) in enumerate(zip(off[:-1], off[1:]))]
            worst = max(worst, check(N, off, got, refs, factor=factor(N)))
        else:  # one long sequence, gamma stored at the rows `rows` only
            T = len(E)
            refs = [(z["loglik" + suffix][0], None, z["S" + suffix][0])]
            assert np.isfinite(got[0][0])
            worst = max(worst, check(N, off, (got[0], None, None, got[3]), refs, factor=factor(N)))
            g = got[2]
            rg = float(np.max(np.abs(g[rows] - ref_g) / (factor(N) * gamma_bound(T, N, ref_g))))
            assert rg <= 1.0, rg
            worst = max(worst, rg)
            assert np.all(np.abs(g.sum(axis=1) - 1.0) <= factor(N) * rowsum_bound(N))
            assert np.all(g[rows][ref_g == 0.0] == 0.0)
            picked = g[np.arange(T), got[1]]
            assert np.all((got[1] >= 0) & (got[1] < N)) and np.all(picked == g.max(axis=1))
        ll, st = cv.score_emissions(h, off, E, forced=forced, kernel=kernel)
        assert np.array_equal(ll, got[0]) and np.array_equal(st, got[3])  # scoring mode: the same forward pass
        if forced is not None:  # gamma is exactly 0 off a forced state
            f = z["forced"]
            for e in np.nonzero(f >= 0)[0]:
                assert got[2][e, f[e]] == 1.0 and got[2][e].sum() == 1.0 and got[1][e] == f[e]
    print(f"{name} {kernel}: error / bound = {worst:.4f}")


# ---- shapes: both sides of every 64 boundary, the plain kernels, group and batch edges ---------------
@functools.lru_cache(maxsize=None)
def shape_case(N, B):
    """(pi, a, b0, off, E, refs) -- shared and never modified."""
    pi, a, b0 = model(N)
    lengths = ragged(B)
    off = offsets_of(lengths)
    E = feasible_scores(N, lengths, seed=100 * N + B, ninf_frac=0.0 if N == 1 else 0.1)
    E.setflags(write=False)
    return pi, a, b0, off, E, oracle(pi, a, E, off)


@pytest.mark.parametrize("B", [1, 33, 70])
@pytest.mark.parametrize("N", [1, 3, 64, 65, 130, 256, 257, 300])
def test_shapes(gpu, N, B):
    pi, a, b0, off, E, refs = shape_case(N, B)
    h = cv.HMM(pi, a, b0, device=gpu)
    worst = 0.0
    got = {}
    for kernel in ("auto", "generic") if N <= 256 else ("auto",):
        got[kernel] = cv.posterior_emissions(h, off, E, gamma=True, kernel=kernel)
        t = cv.last_timing(h)
        mm = kernel == "auto" and N <= 256
        assert t["kernel"] == ("none" if mm else "generic") and t["launches"] == 1, t
        assert (t["seqs_per_wave"] == 32) == mm and t["padded_states"] == (N + 63) // 64 * 64, t
        assert t["fwd_ms"] > 0 and t["bt_ms"] > 0
        st = got[kernel][3]
        for k in range(len(off) - 1):
            assert st[k] == (L.SEQ_EMPTY if off[k] == off[k + 1] else L.SEQ_OK), (k, st[k])
            if off[k] == off[k + 1]:
                assert got[kernel][0][k] == 0.0
        worst = max(worst, check(N, off, got[kernel], refs, factor=2.0 * factor(N)))
    E_dev = torch.from_numpy(np.array(E)).to(f"cuda:{gpu}")
    same_bits(on_device(h, off, E_dev), got["auto"], (N, B))
    print(f"N={N} B={B}: error / (2 x bound) = {worst:.4f}")


# ---- layout: row stride, odd stride, a base 8 bytes off the 16-byte alignment -------------------------
def _views(E, N, full, addr):
    rows = len(E)
    out = [("ld = N + 3, NaN beyond N", full((rows, N + 3))[:, :N]), ("ld = 128", full((rows, 128))[:, :N]),
           ("odd ld", full((rows, N + 1 + N % 2))[:, :N])]
    flat = full((rows * (N + 3) + 2,))
    start = 0 if addr(flat) % 16 == 8 else 1
    shifted = flat[start:start + rows * (N + 3)].reshape(rows, N + 3)[:, :N]
    assert addr(shifted) % 16 == 8
    out.append(("base 8 bytes off 16-byte alignment", shifted))
    for _, v in out:
        v[...] = E if isinstance(v, np.ndarray) else torch.from_numpy(np.array(E)).to(v.device)
    return out


@pytest.mark.parametrize("N", [64, 65])
def test_row_strides_and_alignment(gpu, N):
    pi, a, b0, off, E, refs = shape_case(N, 33)
    h = cv.HMM(pi, a, b0, device=gpu)
    ref = cv.posterior_emissions(h, off, E, gamma=True)
    check(N, off, ref, refs, factor=2.0 * factor(N))
    for name, v in _views(E, N, lambda s: np.full(s, np.nan), lambda x: x.ctypes.data):
        assert not v.flags.c_contiguous
        same_bits(cv.posterior_emissions(h, off, v, gamma=True), ref, name)
    dev = f"cuda:{gpu}"
    for name, v in _views(E, N, lambda s: torch.full(s, float("nan"), dtype=torch.float64, device=dev),
                          lambda x: x.data_ptr()):
        assert not v.is_contiguous()
        for kernel in ("auto", "generic"):
            sliced = on_device(h, off, v, kernel=kernel)
            same_bits(sliced, on_device(h, off, v.contiguous(), kernel=kernel), (name, kernel))
            if kernel == "auto":
                same_bits(sliced, ref, name)


# ---- chunking, host against device, repeats ------------------------------------------------------------
def test_chunks_are_bit_identical(gpu):
    N = 65
    pi, a, b0, off, E, refs = shape_case(N, 70)
    h = cv.HMM(pi, a, b0, device=gpu)
    total = int(off[-1])
    whole = cv.posterior_emissions(h, off, E, gamma=True)
    assert cv.last_timing(h)["launches"] == 1
    per_elem = 128 * 8 * 2 + 4  # forward rows, staged rows and the index
    chunked = cv.posterior_emissions(h, off, E, gamma=True, workspace_bytes=per_elem * (total // 4))
    assert cv.last_timing(h)["launches"] >= 3
    same_bits(chunked, whole, "gamma mode")
    # scoring mode: chunked under the cap by the staged bytes alone
    o = L.opts(L.DTYPE_F64, L.ASSOC_VITERBI, L.KERNEL_AUTO, workspace_bytes=(128 * 8 + 4) * (total // 4))
    ll, st = np.zeros(len(off) - 1), np.zeros(len(off) - 1, np.uint8)
    Ec = np.ascontiguousarray(E)
    rc = L.lib().cv_posterior_emissions(h.handle, len(off) - 1, off.ctypes.data, Ec.ctypes.data, N, ctypes.byref(o),
                                        ll.ctypes.data, None, None, st.ctypes.data)
    assert rc == L.CV_OK and cv.last_timing(h)["launches"] >= 3
    one_ll, one_st = cv.score_emissions(h, off, E)
    assert cv.last_timing(h)["launches"] == 1
    assert np.array_equal(ll, one_ll) and np.array_equal(st, one_st) and np.array_equal(ll, whole[0])
    # a single sequence over the cap
    for kw in (dict(gamma=True), dict(gamma=False, path=False)):
        with pytest.raises(cv.CVError) as e:
            cv.posterior_emissions(h, off, E, workspace_bytes=(128 * 8 + 4) * 11, **kw)  # the longest has 12
        assert e.value.status == L.CV_ENOMEM
    same_bits(cv.posterior_emissions(h, off, E, gamma=True), whole, "after the errors")


def test_device_variant_and_repeat_are_bit_identical(gpu):
    N = 130
    pi, a, b0, off, E, refs = shape_case(N, 33)
    h = cv.HMM(pi, a, b0, device=gpu)
    first = cv.posterior_emissions(h, off, E, gamma=True)
    same_bits(cv.posterior_emissions(h, off, E, gamma=True), first, "repeat")
    dev = torch.device("cuda", gpu)
    E_dev = torch.from_numpy(np.array(E)).to(dev)
    same_bits(on_device(h, off, E_dev), first, "device")
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    d_off = torch.from_numpy(np.ascontiguousarray(off)).to(dev)
    d_ll = torch.zeros(len(off) - 1, dtype=torch.float64, device=dev)
    d_st = torch.zeros(len(off) - 1, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    # scoring mode, the offsets fetched from the device, on a stream of the caller's
    cv.posterior_emissions_device(h, d_off, E_dev, d_ll, d_st, stream=stream.cuda_stream)
    stream.synchronize()
    assert np.array_equal(d_ll.cpu().numpy(), first[0]) and np.array_equal(d_st.cpu().numpy(), first[3])
    t = cv.last_timing(h)
    assert t["fwd_ms"] > 0 and t["launches"] == 1


def test_release_workspaces_frees_the_staged_rows(gpu):
    N = 65
    pi, a, b0, off, E, _ = shape_case(N, 70)
    h = cv.HMM(pi, a, b0, device=gpu)
    cv.score_emissions(h, off, E)
    staged = int(off[-1]) * (128 * 8 + 4)
    before = cv.device_memory()["current"]
    h.release_workspaces()
    assert before - cv.device_memory()["current"] >= staged
    ll, st = cv.score_emissions(h, off, E)
    assert np.all((st == L.SEQ_OK) | (st == L.SEQ_EMPTY))
    h.release_workspaces()


# ---- statuses: a bad score flags its own sequence only -------------------------------------------------
@pytest.mark.parametrize("kernel", ["auto", "generic"])
def test_statuses_and_neighbours(gpu, kernel):
    N = 65
    pi, a, b0, off, E, refs = shape_case(N, 33)
    h = cv.HMM(pi, a, b0, device=gpu)
    clean = cv.posterior_emissions(h, off, E, gamma=True, kernel=kernel)
    bad = np.array(E)
    lens = np.diff(off)
    k_nan, k_inf, k_big, k_dead = [int(k) for k in np.nonzero(lens >= 3)[0][:4]]
    bad[off[k_nan] + 1, 64] = np.nan
    bad[off[k_inf], 0] = np.inf
    bad[off[k_big] + 2, 7] = -(2.0 ** 41)
    bad[off[k_dead] + 1, :] = -np.inf
    got = cv.posterior_emissions(h, off, bad, gamma=True, kernel=kernel)
    for k in range(len(off) - 1):
        lo, hi = int(off[k]), int(off[k + 1])
        if k in (k_nan, k_inf, k_big):
            assert got[3][k] == L.SEQ_BADOBS and np.isnan(got[0][k])
        elif k == k_dead:
            assert got[3][k] == L.SEQ_INFEASIBLE and got[0][k] == -np.inf
        else:  # unchanged bit for bit, in the same group of 32 or not
            assert got[3][k] == clean[3][k]
            same_bits((got[0][k:k + 1], got[1][lo:hi], got[2][lo:hi], got[3][k:k + 1]),
                      (clean[0][k:k + 1], clean[1][lo:hi], clean[2][lo:hi], clean[3][k:k + 1]), k)
            continue
        assert np.all(got[1][lo:hi] == -1) and np.all(got[2][lo:hi] == 0.0)
    ll, st = cv.score_emissions(h, off, bad, kernel=kernel)
    assert np.array_equal(st, got[3]) and np.array_equal(ll, got[0], equal_nan=True)
    # 2^40 itself is rejected, the largest double below it is a score like any other
    edge = np.array(E)
    edge[off[k_big] + 2, 7] = 2.0 ** 40
    assert cv.score_emissions(h, off, edge, kernel=kernel)[1][k_big] == L.SEQ_BADOBS
    edge[off[k_big] + 2, 7] = -np.nextafter(2.0 ** 40, 0)
    assert cv.score_emissions(h, off, edge, kernel=kernel)[1][k_big] == L.SEQ_OK
    # the host variant reports the infeasible sequence after writing every output
    o = L.opts(L.DTYPE_F64, L.ASSOC_VITERBI, L.KERNEL_GENERIC if kernel == "generic" else L.KERNEL_AUTO)
    llc, stc = np.zeros(len(off) - 1), np.zeros(len(off) - 1, np.uint8)
    rc = L.lib().cv_posterior_emissions(h.handle, len(off) - 1, off.ctypes.data, bad.ctypes.data, N, ctypes.byref(o),
                                        llc.ctypes.data, None, None, stc.ctypes.data)
    assert rc == L.CV_EINFEASIBLE and np.array_equal(stc, got[3]) and np.array_equal(llc, got[0], equal_nan=True)


def test_negative_zero_reads_as_zero(gpu):
    N = 17
    pi, a, b0 = model(N)
    off = offsets_of([9, 4])
    E = feasible_scores(N, [9, 4], seed=3)
    E[::2, ::3] = 0.0
    Em = np.array(E)
    Em[::2, ::3] = -0.0
    assert np.signbit(Em).any() and np.array_equal(E, Em)
    h = cv.HMM(pi, a, b0, device=gpu)
    same_bits(cv.posterior_emissions(h, off, Em, gamma=True), cv.posterior_emissions(h, off, E, gamma=True))


def test_a_lone_density_row_neither_overflows_nor_flags(gpu):
    N = 5
    pi, a, b0 = model(N)
    off = offsets_of([6])
    E = feasible_scores(N, [6], seed=8, ninf_frac=0.0)
    E[3] += 300.0  # 10^300-ish densities: three such rows would overflow an unscaled product
    E[4] += 305.0
    E[1] += 290.0
    h = cv.HMM(pi, a, b0, device=gpu)
    got = cv.posterior_emissions(h, off, E, gamma=True)
    shifted = np.array(E)
    shifted[[1, 3, 4]] -= np.array([[290.0], [300.0], [305.0]])
    refs = oracle(pi, a, shifted, off)
    refs = [(refs[0][0] + 895.0, refs[0][1], refs[0][2] + 895.0)]
    check(N, off, got, refs, factor=2.0 * factor(N))


# ---- consistency with the discrete entry, the dense decode and forced tags ------------------------------
def test_agrees_with_posterior_batch_on_a_discrete_model(gpu):
    N, V = 20, 5
    pi, a, b = random_model(N, V, seed=31)
    lengths = [1 + (37 * k) % 40 for k in range(33)]
    off = offsets_of(lengths)
    obs = np.random.default_rng(5).integers(0, V, size=int(off[-1])).astype(np.int32)
    h = cv.HMM(pi, a, b, device=gpu)
    disc = cv.posterior_batch(h, off, obs, gamma=True)
    dense = cv.posterior_emissions(h, off, b.T[obs], gamma=True)
    assert np.array_equal(dense[3], disc[3])
    ok = disc[3] == L.SEQ_OK
    assert ok.sum() >= 5
    worst = 0.0
    for k in np.nonzero(ok)[0]:  # both are within the bound of the exact value: twice the bound apart
        lo, hi = int(off[k]), int(off[k + 1])
        S = np_forward_backward(pi, a, b, obs[lo:hi])[2]
        fake = [(disc[0][k], disc[2][lo:hi], S)]
        one = (dense[0][k:k + 1], None, dense[2][lo:hi], dense[3][k:k + 1])
        worst = max(worst, check(N, offsets_of([hi - lo]), one, fake, factor=2.0))
    for k in np.nonzero(~ok)[0]:
        assert disc[3][k] == L.SEQ_INFEASIBLE and dense[0][k] == -np.inf
    print(f"dense against discrete: difference / (2 x bound) = {worst:.4f}")


def test_viterbi_invariant_and_all_tags_forced(gpu):
    N = 17
    pi, a, b0, = model(N)
    lengths = [33, 5, 1]
    off = offsets_of(lengths)
    E = feasible_scores(N, lengths, seed=12)
    refs = oracle(pi, a, E, off)
    h = cv.HMM(pi, a, b0, device=gpu)
    path, score, st = cv.decode_emissions(h, off, E)  # score: the f64 fold along the best path
    assert np.all(st == L.SEQ_OK)
    for kernel in ("auto", "generic"):
        ll, _ = cv.score_emissions(h, off, E, kernel=kernel)
        for k, T in enumerate(lengths):
            tol = 2 * loglik_bound(T, N, refs[k][2])
            assert score[k] - tol <= ll[k] <= score[k] + T * np.log10(N) + tol, (k, score[k], ll[k])
        fl, fp, fg, fs = cv.posterior_emissions(h, off, E, forced=path, gamma=True, kernel=kernel)
        assert np.all(fs == L.SEQ_OK) and np.array_equal(fp, path)
        frefs = oracle(pi, a, E, off, forced=path)
        for k, T in enumerate(lengths):
            assert abs(fl[k] - score[k]) <= loglik_bound(T, N, frefs[k][2]), (k, fl[k], score[k])
        onehot = np.zeros_like(fg)
        onehot[np.arange(len(path)), path] = 1.0
        assert np.array_equal(fg, onehot)


# ---- scaling invariance: a per-row constant moves loglik by its sum and leaves gamma alone ---------------
@pytest.mark.parametrize("shift", ["exact", "log10_2"])
def test_row_shifts(gpu, shift):
    """E' = E + d_e per row.  "exact": E and d are multiples of 2^-10, so E' is exact and the two
    results differ by sum d within the sum of their bounds.  "log10_2": d_e = m_e log10(2) (the
    row scale 2^-k_e moves by exactly m_e), where forming E' rounds each score by at most u |E'|:
    since d loglik / d E[t][j] = gamma[t][j] and the gamma of a row sum to 1, that moves loglik by at
    most T u max|E'| and a gamma entry by a factor within exp(+-2 ln10 T u max|E'|)."""
    N = 17
    pi, a, b0 = model(N)
    lengths = [33, 2, 7]
    off = offsets_of(lengths)
    rng = np.random.default_rng(77)
    E = np.round(feasible_scores(N, lengths, seed=21) * 1024.0) / 1024.0
    if shift == "exact":
        d = rng.integers(-60 * 1024, 60 * 1024, size=len(E)) / 1024.0
    else:
        d = rng.integers(-190, 190, size=len(E)) * math.log10(2.0)
    E2 = E + d[:, None]
    M = float(np.max(np.abs(E2[np.isfinite(E2)])))
    if shift == "exact":
        finite = np.isfinite(E)
        assert np.array_equal((E2 - d[:, None])[finite], E[finite])
    refs, refs2 = oracle(pi, a, E, off), oracle(pi, a, E2, off)
    h = cv.HMM(pi, a, b0, device=gpu)
    worst = 0.0
    for kernel in ("auto", "generic"):
        g1 = cv.posterior_emissions(h, off, E, gamma=True, kernel=kernel)
        g2 = cv.posterior_emissions(h, off, E2, gamma=True, kernel=kernel)
        check(N, off, g1, refs, factor=2.0 * factor(N))
        check(N, off, g2, refs2, factor=2.0 * factor(N))
        for k, T in enumerate(lengths):
            lo, hi = int(off[k]), int(off[k + 1])
            dsum = math.fsum(d[lo:hi])
            inp = 0.0 if shift == "exact" else T * U * M
            tol = factor(N) * (loglik_bound(T, N, refs[k][2]) + loglik_bound(T, N, refs2[k][2])) + inp + abs(dsum) * 2 * U
            r = abs((g2[0][k] - g1[0][k]) - dsum) / tol
            assert r <= 1.0, (kernel, k, g1[0][k], g2[0][k], dsum, r)
            ref_g = refs[k][1]
            gtol = 2 * factor(N) * gamma_bound(T, N, ref_g) + 2 * np.log(10) * inp * ref_g * 1.01
            rg = float(np.max(np.abs(g2[2][lo:hi] - g1[2][lo:hi]) / gtol))
            assert rg <= 1.0, (kernel, k, rg)
            worst = max(worst, r, rg)
    print(f"row shifts ({shift}): difference / bound = {worst:.4f}")


# ---- partial tags beyond the first column tile / the first 256 states, host and device ------------------
@pytest.mark.parametrize("N", [130, 300])
def test_partial_tags_at_every_tile_and_stride(gpu, N):
    """Tags on states of every column tile, both ends of a DPP row, the last state and (N = 300) a
    state >= 256 (test_gpu_posterior.tag_classes), as `forced` on the host and `forced_dev` on the device."""
    pi, a, b0 = model(N)
    lengths = [12, 1, 5, 2]
    off = offsets_of(lengths)
    E = feasible_scores(N, lengths, seed=900 + N)
    b, obs = as_discrete(E, N)
    h = cv.HMM(pi, a, b0, device=gpu)
    path, _, st = cv.decode_emissions(h, off, E)
    assert np.all(st == L.SEQ_OK)
    forced = covering_tags(pi, a, b, off, obs, path, tag_classes(N))
    tagged = np.nonzero(forced >= 0)[0]
    refs = oracle(pi, a, E, off, forced=forced)
    E_dev = torch.from_numpy(E).to(f"cuda:{gpu}")
    worst = 0.0
    for kernel in kernels_of(N):
        got = cv.posterior_emissions(h, off, E, forced=forced, gamma=True, kernel=kernel)
        t = cv.last_timing(h)
        assert (t["seqs_per_wave"] == 32) == (kernel == "auto" and N <= 256), t
        worst = max(worst, check(N, off, got, refs, factor=2.0 * factor(N)))
        onehot = np.zeros((len(tagged), N))
        onehot[np.arange(len(tagged)), forced[tagged]] = 1.0
        assert np.array_equal(got[2][tagged], onehot) and np.array_equal(got[1][tagged], forced[tagged]), kernel
        ll, st = cv.score_emissions(h, off, E, forced=forced, kernel=kernel)
        assert np.array_equal(ll, got[0]) and np.array_equal(st, got[3])
        same_bits(on_device(h, off, E_dev, forced=forced, kernel=kernel), got, (N, kernel))
    print(f"N={N}: tags on states {sorted(set(forced[tagged].tolist()))}, error / (2 x bound) = {worst:.4f}")


# ---- output modes: every subset of the outputs is the same computation -----------------------------------
def test_output_modes_are_bit_identical(gpu):
    N = 130
    pi, a, b0, off, E, refs = shape_case(N, 33)
    h = cv.HMM(pi, a, b0, device=gpu)
    E_dev = torch.from_numpy(np.array(E)).to(f"cuda:{gpu}")
    for kernel in ("auto", "generic"):
        both = cv.posterior_emissions(h, off, E, gamma=True, kernel=kernel)
        check(N, off, both, refs, factor=2.0 * factor(N))
        only_path = (both[0], both[1], None, both[3])
        only_gamma = (both[0], None, both[2], both[3])
        same_bits(cv.posterior_emissions(h, off, E, gamma=False, kernel=kernel), only_path, (kernel, "path"))
        same_bits(cv.posterior_emissions(h, off, E, gamma=True, path=False, kernel=kernel), only_gamma, (kernel, "gamma"))
        same_bits(on_device(h, off, E_dev, gamma=False, kernel=kernel), only_path, (kernel, "device path"))
        same_bits(on_device(h, off, E_dev, path=False, kernel=kernel), only_gamma, (kernel, "device gamma"))
        ll, st = cv.score_emissions(h, off, E, kernel=kernel)
        assert np.array_equal(ll, both[0]) and np.array_equal(st, both[3])


# ---- the plain kernels' LDS limit and the widest staging stride ---------------------------------------------
def test_lds_limit(gpu):
    """N = 4096: 64 KiB of dynamic LDS in the plain kernels, 16 states per thread, staged rows of NP = 4096."""
    N = 4096
    pi, a, b0 = model(N)
    lengths = [3, 1, 2]
    off = offsets_of(lengths)
    E = feasible_scores(N, lengths, seed=4096)
    refs = oracle(pi, a, E, off)
    h = cv.HMM(pi, a, b0, device=gpu)
    got = cv.posterior_emissions(h, off, E, gamma=True)
    t = cv.last_timing(h)
    assert t["kernel"] == "generic" and t["padded_states"] == N and t["launches"] == 1, t
    worst = check(N, off, got, refs, factor=2.0 * factor(N))
    ll, st = cv.score_emissions(h, off, E)
    assert np.array_equal(ll, got[0]) and np.array_equal(st, got[3])
    same_bits(on_device(h, off, torch.from_numpy(E).to(f"cuda:{gpu}")), got, "device")
    print(f"N={N}: error / (2 x bound) = {worst:.4f}")
