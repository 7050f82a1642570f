"""GPU: cv_expected_counts_model*, cviterbi.autograd.discrete_loglik and full EM -- the expected
emission counts b_cnt[j][v] = sum_s w_s sum_{e in s, obs[e] = v} gamma_e[j] of the discrete model
against the numpy reference of tests/bcnt_ref.py at twice the bound of include/cviterbi.h (u = 2^-53,
T the longest sequence, L the elements of the call, b_abs the statistic with |w_s|):
  |b_cnt - ref| <= (4 T (N + 8) + L + 1) u b_abs + 1e-290 L max(1, max |w|)
(twice: the reference's own sums carry the same error, the convention of counts_ref.py), with
pi_cnt, a_cnt and gamma at the bounds they already have.  Beyond accuracy: everything
cv_expected_counts returns comes back bit for bit, repeats and the device variant are bit-identical,
part sizes (tuning key bcnt_part_rows) and chunk plans regroup the sums within the bound, exact
zeros, NaN and zero weights, mass identities, torch's autograd, EM's monotone likelihood and the
release of the new workspaces.  Each test prints its largest error-to-bound ratio (pytest -s)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import cviterbi as cv
from cviterbi import _lib as L
from bcnt_ref import SEQ_BADOBS, SEQ_INFEASIBLE, SEQ_OK, b_bound, np_model_counts, within
from grad_ref import a_grad_bound, emis_grad_bound, pi_grad_bound, row_weights
from test_posterior import loglik_bound, np_forward_backward, random_model

pytestmark = pytest.mark.gpu

NS = [3, 64, 65, 256, 300]   # NP padding, the last matrix-core size, the plain kernels
VS = [1, 2, 7, 300]
B = 70                        # more than two groups of 32
BAD_HI, BAD_LO, DEAD = 10, 20, 30   # the sequences holding obs = V, obs = -1, and the infeasible one


def bits(x):
    return None if x is None else np.ascontiguousarray(x).view(np.uint8)


def same_bits(x, y, what=""):
    assert len(x) == len(y)
    for k, (u, v) in enumerate(zip(x, y)):
        if u is None or v is None:
            assert u is None and v is None, (what, k)
            continue
        assert u.shape == v.shape and u.dtype == v.dtype, (what, k)
        assert np.array_equal(bits(u), bits(v)), (what, k, np.argwhere(u != v)[:5])


def lengths70():
    """0 .. 40, every small length among them."""
    return [(7 * k + 3) % 41 for k in range(B)]


def tags_along_a_path(pi, a, b, off, obs, rng, keep=0.25):
    """Tags on about `keep` of the elements, along a path the model and the observations allow."""
    forced = np.full(len(obs), -1, np.int32)
    V = b.shape[1]
    for lo, hi in zip(off[:-1], off[1:]):
        prev = None
        for e in range(lo, hi):
            if not 0 <= obs[e] < V:
                break
            ok = np.isfinite(b[:, obs[e]]) & np.isfinite(pi if prev is None else a[prev])
            if not ok.any():
                break
            prev = int(rng.choice(np.nonzero(ok)[0]))
            forced[e] = prev
    forced[rng.random(len(obs)) >= keep] = -1
    return forced


@functools.lru_cache(maxsize=None)
def case(N, V):
    """dict(pi, a, b, off, obs, w, forced, ref (w None), ref_w, only_bad: a value of [0, V) that
    only the BADOBS sequence holds or None, dead: the value only the infeasible sequence holds or
    None) -- built once, shared, never modified.
    V >= 2: the last column of b is -inf and only sequence DEAD observes it (INFEASIBLE).  V = 1
    has no column to spare: there two tags force a transition that A forbids."""
    pi, a, b = random_model(N, V, seed=4100 + 7 * N + V)
    rng = np.random.default_rng(4200 + 7 * N + V)
    lengths = lengths70()
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    free = V                      # the values every sequence draws from: [0, free)
    dead = only_bad = None
    if V >= 2:
        dead = V - 1
        b[:, dead] = -np.inf
        free = V - 1
    else:
        a[0, 1] = -np.inf         # the transition the tags of sequence DEAD force
    if V >= 7:
        only_bad = V - 2
        free = V - 2
    obs = rng.integers(0, free, size=int(off[-1])).astype(np.int32)
    assert min(lengths[BAD_HI], lengths[BAD_LO], lengths[DEAD]) >= 3
    obs[off[BAD_HI] + 1] = V
    obs[off[BAD_LO] + 2] = -1
    if only_bad is not None:
        obs[off[BAD_HI]] = only_bad
    forced = tags_along_a_path(pi, a, b, off, obs, rng)
    if dead is not None:
        obs[off[DEAD] + 1] = dead
    else:
        forced[off[DEAD]:off[DEAD] + 2] = (0, 1)
    w = rng.normal(0.0, 2.0, size=B)
    w[:2] = (-1.75, 0.5)
    for x in (pi, a, b, off, obs, w, forced):
        x.setflags(write=False)
    ref = np_model_counts(pi, a, b, off, obs, None, forced)
    ref_w = np_model_counts(pi, a, b, off, obs, w, forced)
    st = ref["status"]
    assert st[BAD_HI] == SEQ_BADOBS and st[BAD_LO] == SEQ_BADOBS and st[DEAD] == SEQ_INFEASIBLE
    assert (st == SEQ_OK).sum() >= 50, st
    return dict(pi=pi, a=a, b=b, off=off, obs=obs, w=w, forced=forced, ref=ref, ref_w=ref_w, only_bad=only_bad,
                dead=dead)


def check(got, ref, c, w=None, factor=2.0):
    """(loglik, pi_cnt, a_cnt, b_cnt, gamma, status) against np_model_counts' dict; the ratios."""
    off, N = c["off"], len(c["pi"])
    lens = np.diff(off)
    T, Ltot, nseq = int(lens.max()), int(off[-1]), len(lens)
    wv = np.ones(nseq) if w is None else np.asarray(w)
    assert np.array_equal(got[5], ref["status"])
    ratios = [within(got[3], ref["b"], factor * b_bound(T, N, Ltot, ref["b_abs"], float(np.abs(wv).max()))),
              within(got[1], ref["pi"], factor * pi_grad_bound(T, N, nseq, ref["pi_abs"])),
              within(got[2], ref["a"], factor * a_grad_bound(T, N, Ltot, ref["a_abs"]))]
    if got[4] is not None:
        ratios.append(within(got[4], ref["g"], factor * emis_grad_bound(T, N, ref["g_abs"], row_weights(off, wv))))
    assert max(ratios) <= 1.0, ratios
    # exact zeros: b = -inf, values no counted element observes, A = 0, pi = 0
    assert np.all(got[3][np.isinf(c["b"])] == 0.0)
    ok_rows = np.repeat(ref["status"] == SEQ_OK, lens)
    seen = np.zeros(c["b"].shape[1], bool)
    seen[c["obs"][ok_rows]] = True
    assert np.all(got[3][:, ~seen] == 0.0)
    assert np.all(got[2][np.isinf(c["a"])] == 0.0) and np.all(got[1][np.isinf(c["pi"])] == 0.0)
    return max(ratios)


def on_device(h, c, w=None, gamma=True, forced=True, **kw):
    """The _device variant on torch tensors -> numpy results like the host wrapper's."""
    dev = torch.device("cuda", 0)
    off, obs = c["off"], c["obs"]
    total, nseq, N, V = int(off[-1]), len(off) - 1, h.nstates(), h.nobs()
    off_d = torch.from_numpy(np.array(off, np.int64)).to(dev)
    obs_d = torch.from_numpy(np.array(obs, np.int32)).to(dev)
    ll = torch.full((max(nseq, 1),), 77.0, dtype=torch.float64, device=dev)
    st = torch.full((max(nseq, 1),), 9, dtype=torch.uint8, device=dev)
    pg = torch.full((N,), 7.0, dtype=torch.float64, device=dev)
    ag = torch.full((N, N), 7.0, dtype=torch.float64, device=dev)
    bg = torch.full((N, V), 7.0, dtype=torch.float64, device=dev)
    gm = torch.full((max(total, 1), N), 7.0, dtype=torch.float64, device=dev) if gamma else None
    if forced:
        kw["forced_dev"] = torch.from_numpy(np.array(c["forced"], np.int32)).to(dev)
    w_d = None if w is None else torch.from_numpy(np.array(w, np.float64)).to(dev)
    torch.cuda.synchronize(dev)
    cv.expected_counts_model_device(h, off_d, obs_d, ll, pg, ag, bg, st, weight_dev=w_d, gamma_dev=gm,
                                    offsets_host=off, **kw)
    torch.cuda.synchronize(dev)
    return (ll.cpu().numpy()[:nseq], pg.cpu().numpy(), ag.cpu().numpy(), bg.cpu().numpy(),
            gm.cpu().numpy()[:total] if gamma else None, st.cpu().numpy()[:nseq])


# ---- 1. accuracy and the bit identities, over the whole grid ----------------------------------------
@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("N", NS)
def test_accuracy_and_bit_identities(gpu, N, V):
    c = case(N, V)
    lens = np.diff(c["off"])
    assert len(lens) == B and {0, 1, 2} <= set(lens.tolist()) and lens.max() <= 40
    assert (c["forced"] >= 0).any() and (c["w"] < 0).any() and (c["w"] > 0).any()
    h = cv.HMM(c["pi"], c["a"], c["b"], device=gpu)
    args = (h, c["off"], c["obs"])
    plain = cv.expected_counts_model(*args, forced=c["forced"], gamma=True)
    worst = check(plain, c["ref"], c)
    weighted = cv.expected_counts_model(*args, weight=c["w"], forced=c["forced"], gamma=True)
    worst = max(worst, check(weighted, c["ref_w"], c, c["w"]))
    if c["only_bad"] is not None:  # held by the BADOBS sequence alone; the dead value by the infeasible one
        assert not plain[3][:, c["only_bad"]].any() and not weighted[3][:, c["only_bad"]].any()
    if c["dead"] is not None:
        assert not plain[3][:, c["dead"]].any()
    # what cv_expected_counts returns, bit for bit, on the same handle
    base = cv.expected_counts(*args, forced=c["forced"], gamma=True)
    same_bits((plain[0], plain[1], plain[2], plain[4], plain[5]), base, "expected_counts")
    same_bits(cv.expected_counts_model(*args, weight=np.ones(B), forced=c["forced"], gamma=True), plain, "unit weights")
    # repeats and the device variant
    same_bits(cv.expected_counts_model(*args, weight=c["w"], forced=c["forced"], gamma=True), weighted, "repeat")
    same_bits(on_device(h, c, c["w"]), weighted, "device")
    # without gamma the rows go through the workspace (stride NP): the same bound
    nog = cv.expected_counts_model(*args, weight=c["w"], forced=c["forced"])
    assert nog[4] is None
    worst = max(worst, check(nog, c["ref_w"], c, c["w"]))
    same_bits(on_device(h, c, c["w"], gamma=False), nog, "device, no gamma")
    print(f"N={N} V={V}: worst error / (2 x bound) = {worst:.3g}")


def test_generic_kernels_below_257(gpu):
    c = case(65, 7)
    h = cv.HMM(c["pi"], c["a"], c["b"], device=gpu)
    got = cv.expected_counts_model(h, c["off"], c["obs"], weight=c["w"], forced=c["forced"], gamma=True, kernel="generic")
    print(f"generic N=65: {check(got, c['ref_w'], c, c['w']):.3g}")
    base = cv.expected_counts(h, c["off"], c["obs"], forced=c["forced"], gamma=True, kernel="generic")
    plain = cv.expected_counts_model(h, c["off"], c["obs"], forced=c["forced"], gamma=True, kernel="generic")
    same_bits((plain[0], plain[1], plain[2], plain[4], plain[5]), base, "expected_counts, generic")


# ---- 2. plans: part sizes and chunks regroup the sums within the bound ------------------------------
@pytest.mark.parametrize("V", [1, 7, 300])
@pytest.mark.parametrize("N", [65, 300])
def test_parts_and_chunks(gpu, N, V):
    """bcnt_part_rows = 4 and 64: every segment of V = 1 spans all parts, segments of V = 300 are
    mostly shorter than a part.  A workspace cap for at least 3 chunks: segments cross chunks."""
    c = case(N, V)
    h = cv.HMM(c["pi"], c["a"], c["b"], device=gpu)
    args = (h, c["off"], c["obs"])
    NP = (N + 63) // 64 * 64
    total = int(c["off"][-1])
    small = 2 * (total // 4) * (3 * NP * 8 + 8)  # half of the cap goes to the GEMM's partial tiles
    worst = 0.0
    for part_rows in (4, 64, 0):
        h.set_tuning(bcnt_part_rows=part_rows)
        assert h.tuning("bcnt_part_rows") == part_rows
        for ws, gamma in ((0, True), (small, False), (2 * (total // 4) * (2 * NP * 8 + 8), True)):
            got = cv.expected_counts_model(*args, weight=c["w"], forced=c["forced"], gamma=gamma, workspace_bytes=ws)
            if ws:
                assert cv.last_timing(h)["launches"] >= 3, cv.last_timing(h)
            worst = max(worst, check(got, c["ref_w"], c, c["w"]))
            again = cv.expected_counts_model(*args, weight=c["w"], forced=c["forced"], gamma=gamma, workspace_bytes=ws)
            same_bits(again, got, f"repeat at part_rows={part_rows}, workspace={ws}")
    h.set_tuning(bcnt_part_rows=0)
    print(f"N={N} V={V}: worst over the plans = {worst:.3g}")


# ---- 3. exact zeros under tags ----------------------------------------------------------------------
def test_a_value_seen_only_under_a_tag_counts_for_that_state_alone(gpu):
    N, V = 5, 4
    pi, a, b = random_model(N, V, seed=51, zero_frac=0.0)
    rng = np.random.default_rng(52)
    lengths = [6, 1, 9, 4]
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    obs = rng.integers(0, 3, size=int(off[-1])).astype(np.int32)
    forced = np.full(len(obs), -1, np.int32)
    for e in (2, 6, 9, 15):   # value 3 appears here only, each time tagged with state 2
        obs[e], forced[e] = 3, 2
    h = cv.HMM(pi, a, b, device=gpu)
    got = cv.expected_counts_model(h, off, obs, forced=forced, gamma=True)
    assert np.all(got[5] == SEQ_OK)
    col = got[3][:, 3]
    assert abs(col[2] - 4.0) <= 4 * 2.0 ** -50 and not np.delete(col, 2).any()
    assert not np.delete(got[4][[2, 6, 9, 15]], 2, axis=1).any()


# ---- 4. weights: isolation ----------------------------------------------------------------------------
def test_nan_and_zero_weights(gpu):
    c = case(65, 7)
    h = cv.HMM(c["pi"], c["a"], c["b"], device=gpu)
    args = (h, c["off"], c["obs"])
    base = cv.expected_counts_model(*args, weight=c["w"], forced=c["forced"], gamma=True)
    # a sequence that is not OK contributes nothing whatever its weight holds
    w = c["w"].copy()
    w[[BAD_HI, BAD_LO, DEAD]] = (np.nan, np.inf, np.nan)
    w[np.diff(c["off"]) == 0] = np.nan
    same_bits(cv.expected_counts_model(*args, weight=w, forced=c["forced"], gamma=True), base, "NaN on sequences not OK")
    # an OK sequence with a NaN weight: only the entries it touches
    s = 3
    assert c["ref"]["status"][s] == SEQ_OK
    lo, hi = c["off"][s], c["off"][s + 1]
    w = c["w"].copy()
    w[s] = np.nan
    got = cv.expected_counts_model(*args, weight=w, forced=c["forced"], gamma=True)
    touched = np.zeros(7, bool)
    touched[c["obs"][lo:hi]] = True
    assert np.all(np.isnan(got[3][:, touched])) and np.all(np.isfinite(got[3][:, ~touched]))
    assert np.array_equal(bits(got[3][:, ~touched]), bits(base[3][:, ~touched]))
    assert np.all(np.isnan(got[4][lo:hi])) and np.all(np.isfinite(np.delete(got[4], np.arange(lo, hi), axis=0)))
    assert np.array_equal(bits(got[0]), bits(base[0])) and np.array_equal(got[5], base[5])
    # weight 0 adds only +-0
    w = c["w"].copy()
    w[s] = 0.0
    got = cv.expected_counts_model(*args, weight=w, forced=c["forced"], gamma=True)
    assert not got[4][lo:hi].any() and np.all(np.isfinite(got[3]))
    check(got, np_model_counts(c["pi"], c["a"], c["b"], c["off"], c["obs"], w, c["forced"]), c, w)


# ---- 5. mass identities --------------------------------------------------------------------------------
@pytest.mark.parametrize("N,V", [(64, 2), (300, 7)])
def test_mass_identities(gpu, N, V):
    c = case(N, V)
    h = cv.HMM(c["pi"], c["a"], c["b"], device=gpu)
    ll, pc, ac, bc, g, st = cv.expected_counts_model(h, c["off"], c["obs"], forced=c["forced"], gamma=True)
    lens = np.diff(c["off"])
    T, Ltot = int(lens.max()), int(c["off"][-1])
    per_state = b_bound(T, N, Ltot, bc).sum(axis=1) + b_bound(T, N, Ltot, g).sum(axis=0)
    assert np.all(np.abs(bc.sum(axis=1) - g.sum(axis=0)) <= per_state + (V + Ltot) * 2.0 ** -53 * bc.sum(axis=1))
    counted = int(lens[st == SEQ_OK].sum())
    assert abs(bc.sum() - counted) <= b_bound(T, N, Ltot, bc).sum() + N * V * 2.0 ** -53 * counted


# ---- 6. torch.autograd -----------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [3, 65])
@pytest.mark.parametrize("side_stream", [False, True])
def test_autograd_discrete_loglik(gpu, N, side_stream):
    V = 7
    c = case(N, V)
    dev = torch.device("cuda", gpu)
    obs = torch.from_numpy(np.array(c["obs"])).to(dev)
    lp = torch.tensor(c["pi"], dtype=torch.float64, requires_grad=True)
    la = torch.tensor(c["a"], dtype=torch.float64, device=dev, requires_grad=True)
    lb = torch.tensor(c["b"], dtype=torch.float64, device=dev, requires_grad=True)
    coef = torch.from_numpy(np.array(c["w"])).to(dev)

    def run(lp, la, lb):
        ll, st = cv.autograd.discrete_loglik(obs, c["off"], lp, la, lb, forced=np.array(c["forced"]), return_status=True)
        ok = st == SEQ_OK
        (coef[ok] * ll[ok]).sum().backward()
        return ll, st

    if side_stream:
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            ll, st = run(lp, la, lb)
        torch.cuda.current_stream(dev).wait_stream(s)
    else:
        ll, st = run(lp, la, lb)
    torch.cuda.synchronize(dev)
    ref = c["ref_w"]
    assert np.array_equal(st.cpu().numpy(), ref["status"])
    assert lp.grad.device.type == "cpu" and la.grad.device == dev and lb.grad.shape == (N, V)
    got = (ll.detach().cpu().numpy(), lp.grad.numpy(), la.grad.cpu().numpy(), lb.grad.cpu().numpy(), None,
           st.cpu().numpy())
    print(f"autograd N={N}: {check(got, ref, c, c['w']):.3g}")
    h = cv.HMM(c["pi"], c["a"], c["b"], device=gpu)
    score, _ = cv.score_batch(h, c["off"], c["obs"], forced=c["forced"])
    assert np.array_equal(bits(got[0]), bits(score))
    # a parameter that does not require grad gets None; hmm= is reused
    lb2 = torch.tensor(c["b"], dtype=torch.float64, device=dev, requires_grad=True)
    la2 = torch.tensor(c["a"], dtype=torch.float64, device=dev)
    lp2 = torch.tensor(c["pi"], dtype=torch.float64)
    ll2 = cv.autograd.discrete_loglik(obs, c["off"], lp2, la2, lb2, forced=np.array(c["forced"]), hmm=h)
    ok = torch.from_numpy(ref["status"] == SEQ_OK).to(dev)
    (coef[ok] * ll2[ok]).sum().backward()
    torch.cuda.synchronize(dev)
    assert la2.grad is None and lp2.grad is None
    assert np.array_equal(bits(lb2.grad.cpu().numpy()), bits(got[3]))


# ---- 7. full EM: the likelihood never decreases ---------------------------------------------------------
def test_em_rounds_never_lose_likelihood(gpu):
    N, V, nseq = 8, 12, 64
    rng = np.random.default_rng(177)
    lengths = rng.integers(1, 31, size=nseq)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    _, _, tb = random_model(N, V, seed=178, zero_frac=0.0)
    p = 10.0 ** tb[0]
    obs = rng.choice(V, size=int(off[-1]), p=p / p.sum()).astype(np.int32)
    pi, a, b = random_model(N, V, seed=179, zero_frac=0.0)
    totals, slack = [], 0.0
    for _ in range(6):
        h = cv.HMM(pi, a, b, device=gpu)
        S = [np_forward_backward(pi, a, b, obs[lo:hi])[2] for lo, hi in zip(off[:-1], off[1:])]
        slack = max(slack, 2 * sum(loglik_bound(T, N, s) for T, s in zip(lengths, S)))
        ll, pi_cnt, a_cnt, b_cnt, _, st = cv.expected_counts_model(h, off, obs)
        assert np.all(st == SEQ_OK)
        totals.append(float(ll.sum()))
        pi, a, b = cv.reestimate_model(pi_cnt, a_cnt, b_cnt, pi, a, b)
    assert len(totals) == 6  # five rounds of counts -> reestimate_model -> new handle, scored by the sixth
    for before, after in zip(totals, totals[1:]):
        assert after >= before - slack, (totals, slack)
    assert totals[-1] > totals[0]
    print(f"total loglik over the rounds: {totals}")


# ---- 8. workspaces, empty batches, errors ------------------------------------------------------------------
def test_release_workspaces_frees_the_new_buffers(gpu):
    c = case(65, 300)
    h = cv.HMM(c["pi"], c["a"], c["b"], device=gpu)
    first = cv.posterior_batch(h, c["off"], c["obs"], gamma=True)  # builds the tables
    h.release_workspaces()
    before = cv.device_memory()["current"]
    cv.expected_counts_model(h, c["off"], c["obs"])
    held = cv.device_memory()["current"]
    total = int(c["off"][-1])
    # three rows per element, the [V][NP] accumulator, 20 bytes per element of sort buffers
    assert held - before >= total * (3 * 128 * 8 + 8) + 300 * 128 * 8 + 20 * total
    h.release_workspaces()
    assert cv.device_memory()["current"] == before
    again = cv.posterior_batch(h, c["off"], c["obs"], gamma=True)
    for u, v in zip(first, again):
        assert np.array_equal(bits(u), bits(v))
    h.release_workspaces()


def test_empty_batches_and_argument_errors(gpu):
    pi, a, b = random_model(5, 4, seed=9)
    h = cv.HMM(pi, a, b, device=gpu)
    got = cv.expected_counts_model(h, np.array([0]), np.zeros(0, np.int32))  # nseq = 0: zeros
    assert got[3].shape == (5, 4) and not got[1].any() and not got[2].any() and not got[3].any()
    got = cv.expected_counts_model(h, np.array([0, 0, 0]), np.zeros(0, np.int32))  # empty sequences
    assert not got[3].any() and list(got[5]) == [L.SEQ_EMPTY] * 2
    off, obs = np.array([0, 2], np.int64), np.array([0, 1], np.int32)
    for kw in (dict(kernel="trellis"), dict(kernel="trellis_f64")):
        with pytest.raises(cv.CVError) as e:
            cv.expected_counts_model(h, off, obs, **kw)
        assert e.value.status == L.CV_EINVAL
    with pytest.raises(ValueError):
        cv.expected_counts_model(h, off, obs, weight=np.ones(3))
    ll, st = np.zeros(1), np.zeros(1, np.uint8)
    pc, ac, bc = np.zeros(5), np.zeros((5, 5)), np.zeros((5, 4))
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    for hole in range(3):  # a null pi_cnt, a_cnt or b_cnt
        outs = [p(pc), p(ac), p(bc)]
        outs[hole] = None
        assert L.lib().cv_expected_counts_model(h.handle, 1, p(off), p(obs), None, None, p(ll), *outs, None,
                                                p(st)) == L.CV_EINVAL
