"""GPU: cv_expected_counts* (expected initial and transition counts, the E-step's statistics of
pi and A) against the 60-digit fixtures of tools/make_counts_golden.py at the derived bounds and,
beyond them, the numpy oracle of tests/counts_ref.py at twice the bounds (u = 2^-53, T the longest
sequence, L the elements, B the sequences of the call):
  |a_cnt  - ref| <= (4 T (N + 8) + L + 8) u ref + 1e-290 L
  |pi_cnt - ref| <= (4 T (N + 8) + B) u ref + 1e-290 B
Beyond accuracy: exact zeros wherever A is 0, several GEMM parts (tuning key xi_part_rows) and
several chunks inside the same bounds, bit-identical repeats and host / device variants, statuses
that count nothing and disturb nobody, dense emissions of any magnitude, the EM property, and the
workspaces' release.  Each test prints its largest error-to-bound ratio (pytest -s)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import cviterbi as cv
from conftest import load_golden
from counts_ref import a_bound, np_counts, pi_bound, within
from cviterbi import _lib as L
from emis_ref import as_discrete, offsets_of
from test_counts import EMIS_FIXTURES, check_counts
from test_gpu_posterior import feasible_obs
from test_gpu_posterior_emissions import ragged, shape_case
from test_posterior import FIXTURES, loglik_bound, np_forward_backward, random_model
from test_posterior_emissions import C

pytestmark = pytest.mark.gpu


def bits(x):
    return None if x is None else np.ascontiguousarray(x).view(np.uint8)


def same_bits(x, y, what=""):
    """Two results (loglik, pi_cnt, a_cnt, gamma, status) -- or posterior results -- bit for bit."""
    assert len(x) == len(y)
    for k, (u, v) in enumerate(zip(x, y)):
        if u is None or v is None:
            assert u is None and v is None, (what, k)
            continue
        assert u.shape == v.shape and u.dtype == v.dtype, (what, k)
        assert np.array_equal(bits(u), bits(v)), (what, k, np.argwhere(u != v)[:5])


def same_as_posterior(got, post, what=""):
    """loglik, gamma and status of a counts call are those of the posterior call, bit for bit."""
    same_bits((got[0], got[3], got[4]), (post[0], post[2], post[3]), what)


def dims(off):
    lens = np.diff(off)
    return int(lens.max()), int(lens.sum()), len(lens)


def check_against(got_pi, got_a, ref_pi, ref_a, off, N, a_log, factor):
    T, Lel, B = dims(off)
    ra = within(got_a, ref_a, factor * a_bound(T, N, Lel, ref_a))
    rp = within(got_pi, ref_pi, factor * pi_bound(T, N, B, ref_pi))
    assert ra <= 1.0 and rp <= 1.0, (ra, rp)
    assert np.all(got_a[a_log == -np.inf] == 0.0)
    return max(ra, rp)


def on_device(h, off, src, dense, gamma=True, forced=None, **kw):
    """The _device variant on torch tensors (src: obs int32, or a float64 tensor / strided view of
    emission scores already on the device) -> numpy results like the host wrappers'."""
    dev = torch.device("cuda", h.device)
    total, nseq, N = int(off[-1]), len(off) - 1, h.nstates()
    off_d = torch.from_numpy(np.ascontiguousarray(off)).to(dev)
    ll = torch.full((max(nseq, 1),), 77.0, dtype=torch.float64, device=dev)
    st = torch.full((max(nseq, 1),), 9, dtype=torch.uint8, device=dev)
    pc = torch.full((N,), 7.0, dtype=torch.float64, device=dev)
    ac = torch.full((N, N), 7.0, dtype=torch.float64, device=dev)
    g = torch.full((max(total, 1), N), 7.0, dtype=torch.float64, device=dev) if gamma else None
    if forced is not None:
        kw["forced_dev"] = torch.from_numpy(np.ascontiguousarray(forced, np.int32)).to(dev)
    if not dense:
        src = torch.from_numpy(np.array(src, np.int32)).to(dev)
    torch.cuda.synchronize(dev)
    f = cv.expected_counts_emissions_device if dense else cv.expected_counts_device
    f(h, off_d, src, ll, pc, ac, st, gamma_dev=g, offsets_host=off, **kw)  # raises unless CV_OK
    torch.cuda.synchronize(dev)
    return (ll.cpu().numpy()[:nseq], pc.cpu().numpy(), ac.cpu().numpy(), g.cpu().numpy()[:total] if gamma else None,
            st.cpu().numpy()[:nseq])


# ---- golden fixtures (60-digit references): both kernels, free and tagged, one part and many -------
@pytest.mark.parametrize("kernel", ["auto", "generic"])
@pytest.mark.parametrize("name", FIXTURES + EMIS_FIXTURES)
def test_golden(gpu, name, kernel):
    z, c = load_golden(name), load_golden("counts_" + name)
    N, off = len(z["pi"]), z["offsets"]
    dense = "E" in z
    h = cv.HMM(z["pi"], z["a"], np.log10(np.full((N, 2), 0.5)) if dense else z["b"], device=gpu)
    worst = 0.0
    for part_rows in (0, 4):  # 4: several parts, boundaries inside sequences, a short last part
        h.set_tuning(xi_part_rows=part_rows)
        assert h.tuning("xi_part_rows") == part_rows
        for suffix, forced in (("", None), ("_f", z["forced"])):
            if dense:
                got = cv.expected_counts_emissions(h, off, z["E"], forced=forced, gamma=True, kernel=kernel)
                post = cv.posterior_emissions(h, off, z["E"], forced=forced, gamma=True, kernel=kernel)
            else:
                got = cv.expected_counts(h, off, z["obs"], forced=forced, gamma=True, kernel=kernel)
                post = cv.posterior_batch(h, off, z["obs"], forced=forced, gamma=True, kernel=kernel)
            assert np.all(got[4] == L.SEQ_OK)
            same_as_posterior(got, post, (name, suffix))
            worst = max(worst, check_counts(got[1], got[2], z, c, suffix, z["a"]))
    t = cv.last_timing(h)
    assert t["padded_states"] == (N + 63) // 64 * 64
    print(f"{name} {kernel}: error / bound = {worst:.4f}")


def test_fixtures_cover_the_shapes():
    """One tile, NP = 192 and 256 on the matrix cores, NP = 320 on the plain kernels; T = 1 and 2;
    a total of elements that is no multiple of 4 (the last part at xi_part_rows = 4 is short)."""
    ns, lens = set(), set()
    for name in FIXTURES:
        z = load_golden(name)
        ns.add(len(z["pi"]))
        lens |= set(np.diff(z["offsets"]).tolist())
    assert {3, 17, 64, 130, 250, 300} <= ns and {1, 2} <= lens
    assert any(int(load_golden(name)["offsets"][-1]) % 4 for name in FIXTURES)


# ---- more than two groups of 32, ragged lengths (0, 1 and 2 among them) ---------------------------
@functools.lru_cache(maxsize=None)
def discrete_case(N=65, B=70):
    """(pi, a, b, off, obs, (pi_cnt, a_cnt) of the oracle) -- shared and never modified."""
    pi, a, b = random_model(N, 5, seed=8000 + N)
    lengths = ragged(B)
    off = offsets_of(lengths)
    obs = feasible_obs(pi, a, b, lengths, seed=B)
    obs.setflags(write=False)
    return pi, a, b, off, obs, np_counts(pi, a, b, off, obs)


@functools.lru_cache(maxsize=None)
def dense_case(N=65, B=70):
    pi, a, b0, off, E, _ = shape_case(N, B)
    b, obs = as_discrete(E, N)
    return pi, a, b0, off, E, np_counts(pi, a, b, off, obs)


def dense_factor(N):
    return (N + 6 + C) / (N + 8)


@pytest.mark.parametrize("kernel", ["auto", "generic"])
def test_ragged_batch_over_three_groups(gpu, kernel):
    N = 65
    pi, a, b, off, obs, (ref_pi, ref_a) = discrete_case(N, 70)
    assert {0, 1, 2} <= set(np.diff(off).tolist()) and len(off) - 1 > 64
    h = cv.HMM(pi, a, b, device=gpu)
    got = cv.expected_counts(h, off, obs, gamma=True, kernel=kernel)
    same_as_posterior(got, cv.posterior_batch(h, off, obs, gamma=True, kernel=kernel))
    worst = check_against(got[1], got[2], ref_pi, ref_a, off, N, a, 2.0)
    nogamma = cv.expected_counts(h, off, obs, kernel=kernel)  # the arm without gamma: the same sums
    assert nogamma[3] is None
    same_bits(nogamma[:3] + nogamma[4:], got[:3] + got[4:], "gamma=False")
    t = cv.last_timing(h)
    assert t["fwd_ms"] > 0 and t["bt_ms"] > 0 and t["launches"] == 1, t
    print(f"discrete N={N} {kernel}: error / (2 x bound) = {worst:.4f}")


@pytest.mark.parametrize("kernel", ["auto", "generic"])
def test_emissions_agree_with_the_discrete_oracle(gpu, kernel):
    N = 65
    pi, a, b0, off, E, (ref_pi, ref_a) = dense_case(N, 70)
    h = cv.HMM(pi, a, b0, device=gpu)
    got = cv.expected_counts_emissions(h, off, E, gamma=True, kernel=kernel)
    same_as_posterior(got, cv.posterior_emissions(h, off, E, gamma=True, kernel=kernel))
    worst = check_against(got[1], got[2], ref_pi, ref_a, off, N, a, 2.0 * dense_factor(N))
    print(f"dense N={N} {kernel}: error / (2 x bound) = {worst:.4f}")


# ---- bit-identity: repeats, host against device ----------------------------------------------------
def test_repeat_and_device_variant_are_bit_identical(gpu):
    N = 65
    pi, a, b, off, obs, _ = discrete_case(N, 70)
    h = cv.HMM(pi, a, b, device=gpu)
    first = cv.expected_counts(h, off, obs, gamma=True)
    same_bits(cv.expected_counts(h, off, obs, gamma=True), first, "repeat")
    same_bits(on_device(h, off, obs, dense=False), first, "device")
    pi, a, b0, off, E, _ = dense_case(N, 70)
    h = cv.HMM(pi, a, b0, device=gpu)
    first = cv.expected_counts_emissions(h, off, E, gamma=True)
    same_bits(cv.expected_counts_emissions(h, off, E, gamma=True), first, "dense repeat")
    wide = torch.full((len(E), N + 7), float("nan"), dtype=torch.float64, device=f"cuda:{gpu}")
    wide[:, 3:3 + N] = torch.from_numpy(np.array(E)).to(wide.device)
    view = wide[:, 3:3 + N]  # a strided view: ld = N + 7
    assert view.stride(0) == N + 7
    same_bits(on_device(h, off, view, dense=True), first, "dense device")
    same_bits(cv.expected_counts_emissions(h, off, wide.cpu().numpy()[:, 3:3 + N], gamma=True), first, "dense host view")


# ---- chunking: inside the bounds of the one-chunk result, and repeatable ---------------------------
@pytest.mark.parametrize("dense", [False, True])
def test_chunks_stay_inside_the_bound(gpu, dense):
    N = 65
    if dense:
        pi, a, b, off, src, (ref_pi, ref_a) = dense_case(N, 70)
        call, fac = cv.expected_counts_emissions, dense_factor(N)
    else:
        pi, a, b, off, src, (ref_pi, ref_a) = discrete_case(N, 70)
        call, fac = cv.expected_counts, 1.0
    h = cv.HMM(pi, a, b, device=gpu)
    whole = call(h, off, src, gamma=True)
    assert cv.last_timing(h)["launches"] == 1
    per_elem = 2 * 128 * 8 + 8 + (128 * 8 + 4 if dense else 0)
    ws = 2 * per_elem * (int(off[-1]) // 4)  # half of the cap is the partial tiles'
    chunked = call(h, off, src, gamma=True, workspace_bytes=ws)
    assert cv.last_timing(h)["launches"] >= 3
    same_bits(call(h, off, src, gamma=True, workspace_bytes=ws), chunked, "chunked repeat")
    same_bits((chunked[0], chunked[3], chunked[4]), (whole[0], whole[3], whole[4]), "per-sequence outputs")
    # each is within its bound of the exact counts, so the two are within twice the bound of each other
    worst = check_against(chunked[1], chunked[2], whole[1], whole[2], off, N, a, 2.0 * fac)
    check_against(chunked[1], chunked[2], ref_pi, ref_a, off, N, a, 2.0 * fac)
    print(f"dense={dense}: chunked against whole, error / (2 x bound) = {worst:.4f}")


# ---- statuses: BADOBS, INFEASIBLE and EMPTY sequences count nothing and disturb nobody --------------
def test_statuses_discrete(gpu):
    N, V = 5, 4
    pi, a, b = random_model(N, V, seed=9, zero_frac=0.0)
    b[:, 3] = -np.inf  # observation 3 has probability 0 in every state
    good = [np.array([0, 1, 2, 1, 0], np.int32), np.array([2], np.int32), np.array([1, 1, 0, 2, 2, 0, 1], np.int32)]
    seqs = [good[0], np.array([0, 3, 1], np.int32), good[1], np.zeros(0, np.int32), np.array([1, 99, 0, -4], np.int32),
            good[2]]
    off, obs = offsets_of([len(s) for s in seqs]), np.concatenate(seqs)
    goff, gobs = offsets_of([len(s) for s in good]), np.concatenate(good)
    ref_pi, ref_a = np_counts(pi, a, b, goff, gobs)
    h = cv.HMM(pi, a, b, device=gpu)
    for kernel in ("auto", "generic"):
        got = cv.expected_counts(h, off, obs, gamma=True, kernel=kernel)
        same_as_posterior(got, cv.posterior_batch(h, off, obs, gamma=True, kernel=kernel), kernel)
        assert list(got[4]) == [L.SEQ_OK, L.SEQ_INFEASIBLE, L.SEQ_OK, L.SEQ_EMPTY, L.SEQ_BADOBS, L.SEQ_OK]
        clean = cv.expected_counts(h, goff, gobs, kernel=kernel)
        check_against(got[1], got[2], clean[1], clean[2], off, N, a, 2.0)
        check_against(got[1], got[2], ref_pi, ref_a, off, N, a, 2.0)
        # three sequences counted: once each in pi, T - 1 times each in A
        assert abs(got[1].sum() - 3) <= pi_bound(7, N, 6, 3.0) + N * 2.0 ** -53 * 3
        assert abs(got[2].sum() - (4 + 0 + 6)) <= a_bound(7, N, 20, 10.0) + N * N * 2.0 ** -53 * 10
        dev = on_device(h, off, obs, dense=False, kernel=kernel)  # CV_OK: it did not raise
        same_bits(dev, got, "device")
    # the host C call reports the infeasible sequence, after writing every output
    o = L.opts(L.DTYPE_F64)
    llc, stc, pc, ac = np.zeros(6), np.zeros(6, np.uint8), np.full(N, 7.0), np.full((N, N), 7.0)
    rc = L.lib().cv_expected_counts(h.handle, 6, off.ctypes.data, obs.ctypes.data, ctypes.byref(o), llc.ctypes.data,
                                    pc.ctypes.data, ac.ctypes.data, None, stc.ctypes.data)
    assert rc == L.CV_EINFEASIBLE
    last = cv.expected_counts(h, off, obs)
    same_bits((llc, pc, ac, None, stc), last, "C call")


@pytest.mark.parametrize("kernel", ["auto", "generic"])
def test_statuses_emissions(gpu, kernel):
    N = 65
    pi, a, b0, off, E, _ = dense_case(N, 33)
    h = cv.HMM(pi, a, b0, device=gpu)
    lens = np.diff(off)
    k_nan, k_inf, k_dead = [int(k) for k in np.nonzero(lens >= 3)[0][:3]]
    bad = np.array(E)
    bad[off[k_nan] + 1, 64] = np.nan
    bad[off[k_inf], 0] = np.inf
    bad[off[k_dead] + 1, :] = -np.inf
    got = cv.expected_counts_emissions(h, off, bad, gamma=True, kernel=kernel)
    same_as_posterior(got, cv.posterior_emissions(h, off, bad, gamma=True, kernel=kernel))
    assert got[4][k_nan] == L.SEQ_BADOBS and got[4][k_inf] == L.SEQ_BADOBS and got[4][k_dead] == L.SEQ_INFEASIBLE
    assert np.all(np.isfinite(got[1])) and np.all(np.isfinite(got[2]))
    keep = [k for k in range(len(lens)) if k not in (k_nan, k_inf, k_dead)]
    koff = offsets_of(lens[keep])
    kE = np.concatenate([E[off[k]:off[k + 1]] for k in keep])
    clean = cv.expected_counts_emissions(h, koff, kE, kernel=kernel)
    b, obs = as_discrete(kE, N)
    ref_pi, ref_a = np_counts(pi, a, b, koff, obs)
    fac = 2.0 * dense_factor(N)
    worst = check_against(got[1], got[2], clean[1], clean[2], off, N, a, fac)
    check_against(got[1], got[2], ref_pi, ref_a, off, N, a, fac)
    dev = on_device(h, off, torch.from_numpy(bad).to(f"cuda:{gpu}"), dense=True, kernel=kernel)  # CV_OK
    same_bits(dev, got, "device")
    o = L.opts(L.DTYPE_F64, L.ASSOC_VITERBI, L.KERNEL_GENERIC if kernel == "generic" else L.KERNEL_AUTO)
    B = len(lens)
    llc, stc, pc, ac = np.zeros(B), np.zeros(B, np.uint8), np.full(N, 7.0), np.full((N, N), 7.0)
    rc = L.lib().cv_expected_counts_emissions(h.handle, B, off.ctypes.data, bad.ctypes.data, N, ctypes.byref(o),
                                              llc.ctypes.data, pc.ctypes.data, ac.ctypes.data, None, stc.ctypes.data)
    assert rc == L.CV_EINFEASIBLE
    same_bits((llc, pc, ac, stc), got[:3] + got[4:], "C call")
    print(f"{kernel}: with the flagged sequences against without, error / (2 x bound) = {worst:.4f}")


def test_empty_batches_write_zeros(gpu):
    pi, a, b = random_model(5, 4, seed=9)
    h = cv.HMM(pi, a, b, device=gpu)
    got = cv.expected_counts(h, np.zeros(1, np.int64), np.zeros(0, np.int32))
    assert got[1].shape == (5,) and not got[1].any() and not got[2].any()
    got = cv.expected_counts(h, np.zeros(4, np.int64), np.zeros(0, np.int32))  # three empty sequences
    assert list(got[4]) == [L.SEQ_EMPTY] * 3 and not got[1].any() and not got[2].any()
    got = cv.expected_counts(h, np.array([0, 1, 2]), np.array([0, 1], np.int32))  # T = 1: pi only
    assert np.all(got[4] == L.SEQ_OK) and abs(got[1].sum() - 2) <= 1e-14 and not got[2].any()


# ---- dense emissions of a magnitude no probability holds -------------------------------------------
def test_scores_near_minus_5000_per_step(gpu):
    N, T = 4, 300
    pi, a, b0 = random_model(N, 2, seed=31, zero_frac=0.0)
    rng = np.random.default_rng(5)
    E = -5000.0 + rng.normal(0.0, 2.0, size=(T, N))
    off = offsets_of([T])
    h = cv.HMM(pi, a, b0, device=gpu)
    for kernel in ("auto", "generic"):
        ll, pc, ac, _, st = cv.expected_counts_emissions(h, off, E, kernel=kernel)
        assert st[0] == L.SEQ_OK and ll[0] < -1.4e6
        assert np.all(np.isfinite(pc)) and np.all(np.isfinite(ac)) and np.all(ac >= 0)
        fac = dense_factor(N)
        assert abs(ac.sum() - (T - 1)) <= fac * a_bound(T, N, T, T - 1) + N * N * 2.0 ** -53 * (T - 1)
        assert abs(pc.sum() - 1) <= fac * pi_bound(T, N, 1, 1.0) + N * 2.0 ** -53
        # the row scale cancels: the same counts from the scores shifted up by 5000 per step
        ref_pi, ref_a = np_counts(pi, a, *as_discrete(E + 5000.0, N)[:1], off, np.arange(T))
        check_against(pc, ac, ref_pi, ref_a, off, N, a, 2.0 * fac)


# ---- the EM property: the likelihood never decreases ------------------------------------------------
def test_em_rounds_never_lose_likelihood(gpu):
    N = 5
    lengths = [20, 7, 1, 13, 2, 16]
    off = offsets_of(lengths)
    rng = np.random.default_rng(77)
    E = rng.normal(0.0, 1.5, size=(int(off[-1]), N))
    pi, a, b0 = random_model(N, 2, seed=78, zero_frac=0.0)
    b, obs = as_discrete(E, N)
    totals, slack = [], 0.0
    for _ in range(5):
        h = cv.HMM(pi, a, b0, device=gpu)
        S = [np_forward_backward(pi, a, b, obs[lo:hi])[2] for lo, hi in zip(off[:-1], off[1:])]
        # twice the summed loglik bound, the largest over the rounds
        slack = max(slack, 2 * dense_factor(N) * sum(loglik_bound(T, N, s) for T, s in zip(lengths, S)))
        ll, pi_cnt, a_cnt, _, st = cv.expected_counts_emissions(h, off, E)
        assert np.all(st == L.SEQ_OK)
        totals.append(float(ll.sum()))
        pi, a = cv.reestimate(pi_cnt, a_cnt, pi, a)
    assert len(totals) == 5  # four rounds of counts -> reestimate -> new handle, scored by the fifth
    for before, after in zip(totals, totals[1:]):
        assert after >= before - slack, (totals, slack)
    assert totals[-1] > totals[0]
    print(f"total loglik over the rounds: {totals}")


# ---- workspaces ------------------------------------------------------------------------------------
def test_release_workspaces_frees_everything_new(gpu):
    N = 65
    pi, a, b, off, obs, _ = discrete_case(N, 70)
    h = cv.HMM(pi, a, b, device=gpu)
    first = cv.posterior_batch(h, off, obs, gamma=True)  # builds the tables
    h.release_workspaces()
    before = cv.device_memory()["current"]
    h.set_tuning(xi_part_rows=8)
    cv.expected_counts(h, off, obs, gamma=True)
    held = cv.device_memory()["current"]
    total = int(off[-1])
    assert held - before >= total * (2 * 128 * 8 + 8) + 128 * 128 * 8 * ((total + 7) // 8) + 70 * 128 * 8
    h.release_workspaces()
    assert cv.device_memory()["current"] == before
    again = cv.posterior_batch(h, off, obs, gamma=True)
    for u, v in zip(first, again):
        assert np.array_equal(bits(u), bits(v))
    h.release_workspaces()


def test_argument_errors(gpu):
    pi, a, b = random_model(5, 4, seed=9)
    h = cv.HMM(pi, a, b, device=gpu)
    off, obs = np.array([0, 2]), np.array([0, 1], np.int32)
    for kw, status in ((dict(kernel="trellis"), L.CV_EINVAL), (dict(kernel="trellis_f64"), L.CV_EINVAL)):
        with pytest.raises(cv.CVError) as e:
            cv.expected_counts(h, off, obs, **kw)
        assert e.value.status == status
    with pytest.raises(ValueError):
        cv.expected_counts_emissions(h, off, np.zeros((2, 4)))  # fewer columns than states
    with pytest.raises(cv.CVError) as e:  # a single sequence over the cap, as in posterior_emissions
        cv.expected_counts_emissions(h, np.array([0, 12]), np.zeros((12, 5)), workspace_bytes=2 * (3 * 64 * 8 + 12) * 11)
    assert e.value.status == L.CV_ENOMEM
