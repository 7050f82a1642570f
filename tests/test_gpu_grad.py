"""GPU: cv_loglik_grad_emissions* and cviterbi.autograd.sequence_loglik -- the gradient of
sum_s w_s log10 P(o_s) in the emission scores, log10 pi and log10 A -- against the numpy oracle of
tests/grad_ref.py at twice the bounds of include/cviterbi.h (u = 2^-53, T the longest sequence, L
the elements, B the sequences of the call, X_abs the statistic with |w_s|):
  |a_grad  - ref| <= (4 T (N + 8) + L + 9) u a_abs + 1e-290 L
  |pi_grad - ref| <= (4 T (N + 8) + B + 1) u pi_abs + 1e-290 B
  |emis_grad[e][j] - w_s gamma| <= (4 T (N + 8) + 1) u |w_s| gamma + 1e-290 max(1, |w_s|)
Beyond accuracy: unit weights reproduce the counts call bit for bit, exact scaling identities,
strides and shifted bases, chunks and GEMM parts, statuses under NaN and inf weights, torch's
autograd against the pure-torch oracle, and the workspaces' release.  Each test prints its largest
error-to-bound ratio (pytest -s)."""
import functools

import numpy as np
import pytest
import torch

import cviterbi as cv
from cviterbi import _lib as L
from emis_ref import offsets_of
from grad_ref import grad_ratios, np_grad, torch_grad
from test_gpu_posterior_emissions import feasible_scores, ragged
from test_posterior import random_model

pytestmark = pytest.mark.gpu


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


def tags_along_a_path(pi, a, E, off, rng, keep=1.0 / 3.0):
    """Tags on about `keep` of the elements, along a path the model and the scores allow."""
    forced = np.full(len(E), -1, np.int32)
    for lo, hi in zip(off[:-1], off[1:]):
        prev = None
        for e in range(lo, hi):
            ok = np.isfinite(E[e]) & np.isfinite(pi if prev is None else a[prev])
            if not ok.any():
                break
            prev = int(rng.choice(np.nonzero(ok)[0]))
            forced[e] = prev
    forced[rng.random(len(E)) >= keep] = -1
    return forced


@functools.lru_cache(maxsize=None)
def grad_case(N, B=70):
    """(pi, a, b0, off, E, w, forced, ref_free, ref_tagged) -- shared and never modified.  B = 70:
    three groups of 32 with lengths 0, 1 and 2 among them, -inf scores, one row near -5000,
    signed weights."""
    pi, a, b0 = random_model(N, 2, seed=9100 + N)
    lengths = ragged(B)
    off = offsets_of(lengths)
    E = feasible_scores(N, lengths, seed=9200 + N, ninf_frac=0.05)
    rng = np.random.default_rng(9300 + N)
    far = int(off[np.nonzero(np.diff(off) >= 5)[0][0]]) + 2
    E[far] = np.where(np.isfinite(E[far]), -5000.0 + rng.normal(0.0, 2.0, size=N), -np.inf)
    w = rng.normal(0.0, 2.0, size=B)
    w[:2] = (-1.75, 0.5)
    forced = tags_along_a_path(pi, a, E, off, rng)
    for x in (pi, a, b0, off, E, w, forced):
        x.setflags(write=False)
    return pi, a, b0, off, E, w, forced, np_grad(pi, a, E, off, w), np_grad(pi, a, E, off, w, forced)


def check(got, ref, off, N, w, a_log, factor=2.0):
    """(loglik, pi_grad, a_grad, emis_grad, status) against np_grad's dict; the worst ratio."""
    assert np.array_equal(got[4], ref["status"])
    ratios = grad_ratios(got[1], got[2], got[3], ref, off, N, w, factor)
    assert max(ratios) <= 1.0, ratios
    assert np.all(got[2][np.isinf(a_log)] == 0.0)
    return max(ratios)


def on_device(h, off, E_dev, w=None, egrad=True, forced=None, grad_view=None, **kw):
    """The _device variant on torch tensors (E_dev: a float64 tensor or strided view on the
    device; grad_view: the tensor view the gradient rows go to) -> numpy results like the host
    wrapper's."""
    dev = E_dev.device
    total, nseq, N = int(off[-1]), len(off) - 1, h.nstates()
    off_d = torch.from_numpy(np.array(off, np.int64)).to(dev)
    ll = torch.full((max(nseq, 1),), 77.0, dtype=torch.float64, device=dev)
    st = torch.full((max(nseq, 1),), 9, dtype=torch.uint8, device=dev)
    pg = torch.full((N,), 7.0, dtype=torch.float64, device=dev)
    ag = torch.full((N, N), 7.0, dtype=torch.float64, device=dev)
    if grad_view is None and egrad:
        grad_view = torch.full((max(total, 1), N), 7.0, dtype=torch.float64, device=dev)
    if forced is not None:
        kw["forced_dev"] = torch.from_numpy(np.array(forced, np.int32)).to(dev)
    w_d = None if w is None else torch.from_numpy(np.ascontiguousarray(w, np.float64)).to(dev)
    torch.cuda.synchronize(dev)
    cv.loglik_grad_emissions_device(h, off_d, E_dev, ll, pg, ag, st, weight_dev=w_d, emis_grad_dev=grad_view,
                                    offsets_host=off, **kw)
    torch.cuda.synchronize(dev)
    return (ll.cpu().numpy()[:nseq], pg.cpu().numpy(), ag.cpu().numpy(),
            grad_view.cpu().numpy()[:total] if grad_view is not None else None, st.cpu().numpy()[:nseq])


# ---- 1. accuracy: every NP of the matrix-core kernels, the plain kernels, free and tagged -----------
@pytest.mark.parametrize("kernel,N", [("auto", 3), ("auto", 64), ("auto", 65), ("auto", 130), ("auto", 256),
                                      ("generic", 65), ("generic", 300)])
def test_accuracy(gpu, kernel, N):
    pi, a, b0, off, E, w, forced, ref_free, ref_tag = grad_case(N)
    lens = np.diff(off)
    assert len(lens) == 70 and {0, 1, 2} <= set(lens.tolist()) and lens.max() <= 64
    assert (w < 0).any() and (w > 0).any() and np.isinf(E).any() and (E[np.isfinite(E)] < -4900).any()
    h = cv.HMM(pi, a, b0, device=gpu)
    worst = 0.0
    for tags, ref in ((None, ref_free), (forced, ref_tag)):
        got = cv.loglik_grad_emissions(h, off, E, weights=w, forced=tags, kernel=kernel)
        t = cv.last_timing(h)
        assert t["padded_states"] == (N + 63) // 64 * 64 and t["fwd_ms"] > 0 and t["bt_ms"] > 0 and t["launches"] == 1, t
        worst = max(worst, check(got, ref, off, N, w, a))
        assert np.all(got[3][np.isinf(E)] == 0.0) and np.all(got[1][np.isinf(pi)] == 0.0)
        post = cv.posterior_emissions(h, off, E, forced=tags, path=False, kernel=kernel)
        same_bits((got[0], got[4]), (post[0], post[3]), "loglik and status")
    assert (ref_free["status"] == L.SEQ_OK).sum() >= 50
    print(f"N={N} {kernel}: error / (2 x bound) = {worst:.4f}")


# ---- 2. unit weights: the counts call bit for bit --------------------------------------------------
@pytest.mark.parametrize("kernel,N", [("auto", 65), ("auto", 256), ("generic", 65)])
def test_unit_weights_reproduce_the_counts_call(gpu, kernel, N):
    pi, a, b0, off, E, _, forced, _, _ = grad_case(N)
    h = cv.HMM(pi, a, b0, device=gpu)
    for tags in (None, forced):
        counts = cv.expected_counts_emissions(h, off, E, forced=tags, gamma=True, kernel=kernel)
        same_bits(cv.loglik_grad_emissions(h, off, E, forced=tags, kernel=kernel), counts, "weights=None")
        ones = cv.loglik_grad_emissions(h, off, E, weights=np.ones(len(off) - 1), forced=tags, kernel=kernel)
        same_bits(ones, counts, "all ones")
        without = cv.loglik_grad_emissions(h, off, E, forced=tags, emis_grad=False, kernel=kernel)
        assert without[3] is None
        same_bits(without[:3] + without[4:], counts[:3] + counts[4:], "emis_grad=False")


# ---- 3. exact scaling identities, repeats, host against device -------------------------------------
@pytest.mark.parametrize("kernel", ["auto", "generic"])
def test_scaling_identities_and_bit_identity(gpu, kernel):
    N = 65
    pi, a, b0, off, E, w, forced, _, _ = grad_case(N)
    h = cv.HMM(pi, a, b0, device=gpu)
    first = cv.loglik_grad_emissions(h, off, E, weights=w, forced=forced, kernel=kernel)
    same_bits(cv.loglik_grad_emissions(h, off, E, weights=w, forced=forced, kernel=kernel), first, "repeat")
    for scale in (2.0, -1.0):
        got = cv.loglik_grad_emissions(h, off, E, weights=scale * w, forced=forced, kernel=kernel)
        same_bits((got[0], got[4]), (first[0], first[4]), "loglik and status")
        # + 0.0: a term -0.0 (a zero times a negative weight) compares as the +0.0 it is
        same_bits([x + 0.0 for x in got[1:4]], [scale * x + 0.0 for x in first[1:4]], f"weights x {scale}")
    dev = on_device(h, off, torch.from_numpy(np.array(E)).to(f"cuda:{gpu}"), w, forced=forced, kernel=kernel)
    same_bits(dev, first, "device")


# ---- 4. layout: strided scores, strided gradient rows on a shifted base ----------------------------
@pytest.mark.parametrize("kernel,N", [("auto", 65), ("auto", 256), ("generic", 65)])
def test_strides_and_shifted_base(gpu, kernel, N):
    pi, a, b0, off, E, w, forced, _, _ = grad_case(N)
    h = cv.HMM(pi, a, b0, device=gpu)
    dev = torch.device("cuda", gpu)
    total = int(off[-1])
    plain = on_device(h, off, torch.from_numpy(np.array(E)).to(dev), w, forced=forced, kernel=kernel)
    wide = torch.full((total, N + 3), float("nan"), dtype=torch.float64, device=dev)
    wide[:, 2:2 + N] = torch.from_numpy(np.array(E)).to(dev)
    view = wide[:, 2:2 + N]  # ld = N + 3
    assert view.stride(0) == N + 3
    for ld_grad in sorted({N + 5, (N + 5) | 1}):  # N + 5, and an odd one
        flat = torch.full((total * ld_grad + 1,), -123.25, dtype=torch.float64, device=dev)
        rows = flat[1:].view(total, ld_grad)  # the base 8 bytes past the allocation's: rows 8-byte aligned only
        gview = rows[:, :N]
        assert gview.stride(0) == ld_grad and gview.data_ptr() % 16 == 8
        got = on_device(h, off, view, w, forced=forced, grad_view=gview, kernel=kernel)
        same_bits(got, plain, f"ld_grad={ld_grad}")
        host = flat.cpu().numpy()
        assert host[0] == -123.25 and np.all(host[1:].reshape(total, ld_grad)[:, N:] == -123.25)


# ---- 5. chunks and GEMM parts ----------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["auto", "generic"])
def test_chunks_and_parts_stay_inside_the_bounds(gpu, kernel):
    N = 65
    pi, a, b0, off, E, w, forced, _, ref = grad_case(N)
    h = cv.HMM(pi, a, b0, device=gpu)
    whole = cv.loglik_grad_emissions(h, off, E, weights=w, forced=forced, kernel=kernel)
    assert cv.last_timing(h)["launches"] == 1
    per_elem = 2 * 128 * 8 + 8 + 128 * 8 + 4
    ws = 2 * per_elem * (int(off[-1]) // 4)  # half of the cap is the partial tiles'
    chunked = cv.loglik_grad_emissions(h, off, E, weights=w, forced=forced, kernel=kernel, workspace_bytes=ws)
    assert cv.last_timing(h)["launches"] >= 3
    h.set_tuning(xi_part_rows=4)
    parts = cv.loglik_grad_emissions(h, off, E, weights=w, forced=forced, kernel=kernel)
    both = cv.loglik_grad_emissions(h, off, E, weights=w, forced=forced, kernel=kernel, workspace_bytes=ws)
    h.set_tuning(xi_part_rows=0)
    worst = 0.0
    for name, got in (("chunked", chunked), ("parts", parts), ("both", both)):
        same_bits((got[0], got[3], got[4]), (whole[0], whole[3], whole[4]), name + ": per-sequence outputs")
        worst = max(worst, check(got, ref, off, N, w, a))
    print(f"{kernel}: chunks and parts, error / (2 x bound) = {worst:.4f}")


# ---- 6. statuses: flagged sequences contribute nothing, whatever their weights ---------------------
@pytest.mark.parametrize("kernel", ["auto", "generic"])
def test_statuses_and_zero_weight(gpu, kernel):
    N = 17
    pi, a, b0 = random_model(N, 2, seed=9417)
    zi, zj = [int(x[0]) for x in np.nonzero(np.isinf(a))]
    lengths = [6, 4, 0, 5, 1, 7, 3]
    k_nan, k_dead, k_empty = 1, 3, 2
    off = offsets_of(lengths)
    rng = np.random.default_rng(9418)
    E = rng.normal(0.0, 2.0, size=(int(off[-1]), N))
    E[off[k_nan] + 2, 5] = np.nan
    forced = np.full(len(E), -1, np.int32)
    forced[off[k_dead] + 1], forced[off[k_dead] + 2] = zi, zj  # tags through a zero arc
    w = np.array([1.5, np.nan, np.nan, np.inf, -0.75, 2.0, -1.25])
    h = cv.HMM(pi, a, b0, device=gpu)
    got = cv.loglik_grad_emissions(h, off, E, weights=w, forced=forced, kernel=kernel)
    assert list(got[4]) == [L.SEQ_OK, L.SEQ_BADOBS, L.SEQ_EMPTY, L.SEQ_INFEASIBLE, L.SEQ_OK, L.SEQ_OK, L.SEQ_OK]
    assert all(np.all(np.isfinite(x)) for x in got[1:4])
    for k in (k_nan, k_dead):
        assert not got[3][off[k]:off[k + 1]].any()
    dev = on_device(h, off, torch.from_numpy(E).to(f"cuda:{gpu}"), w, forced=forced, kernel=kernel)  # CV_OK
    same_bits(dev, got, "device")
    # the batch without them
    keep = [0, 4, 5, 6]
    koff = offsets_of([lengths[k] for k in keep])
    kE = np.concatenate([E[off[k]:off[k + 1]] for k in keep])
    kf = np.concatenate([forced[off[k]:off[k + 1]] for k in keep])
    clean = cv.loglik_grad_emissions(h, koff, kE, weights=w[keep], forced=kf, kernel=kernel)
    ref = np_grad(pi, a, kE, koff, w[keep], kf)
    rows = np.concatenate([np.arange(off[k], off[k + 1]) for k in keep])
    same_bits((got[0][keep], got[3][rows]), (clean[0], clean[3]), "per-sequence outputs")
    worst = max(grad_ratios(got[1], got[2], got[3][rows], ref, koff, N, w[keep], 2.0))
    # each is within its bound of the exact sums, so the two are within twice the bound of each other
    both = dict(ref, pi=clean[1], a=clean[2], e=clean[3])
    worst = max(worst, *grad_ratios(got[1], got[2], got[3][rows], both, koff, N, w[keep], 2.0))
    assert worst <= 1.0, worst
    # an OK sequence with weight 0: every term it adds is +-0.  As the last sequence its rows come
    # after everybody's in every sum, so the sums are those of the batch without it, bit for bit ...
    w0 = np.append(w[keep], 0.0)
    off0 = offsets_of([lengths[k] for k in keep] + [5])
    E0 = np.concatenate([kE, rng.normal(0.0, 2.0, size=(5, N))])
    f0 = np.concatenate([kf, np.full(5, -1, np.int32)])
    zero = cv.loglik_grad_emissions(h, off0, E0, weights=w0, forced=f0, kernel=kernel)
    assert zero[4][-1] == L.SEQ_OK and not zero[3][koff[-1]:].any()
    same_bits((zero[1] + 0.0, zero[2] + 0.0), (clean[1] + 0.0, clean[2] + 0.0), "weight 0, last")
    # ... and in the middle they are those of the same batch with that sequence flagged
    wmid, Ebad = w.copy(), E.copy()
    wmid[5] = 0.0
    Ebad[off[5], 0] = np.nan
    mid = cv.loglik_grad_emissions(h, off, E, weights=wmid, forced=forced, kernel=kernel)
    flagged = cv.loglik_grad_emissions(h, off, Ebad, weights=w, forced=forced, kernel=kernel)
    assert flagged[4][5] == L.SEQ_BADOBS and mid[4][5] == L.SEQ_OK
    same_bits((mid[1] + 0.0, mid[2] + 0.0, mid[3] + 0.0), (flagged[1] + 0.0, flagged[2] + 0.0, flagged[3] + 0.0),
              "weight 0, in the middle")
    # an OK sequence with a non-finite weight: documented to make what it touches non-finite
    wnan = w.copy()
    wnan[0] = np.nan
    poisoned = cv.loglik_grad_emissions(h, off, E, weights=wnan, forced=forced, kernel=kernel)
    assert np.isnan(poisoned[3][:off[1]]).any() and np.isnan(poisoned[1]).any()
    same_bits((poisoned[0], poisoned[4], poisoned[3][off[1]:]), (got[0], got[4], got[3][off[1]:]), "the others' rows")
    print(f"{kernel}: with the flagged sequences against without, error / (2 x bound) = {worst:.4f}")


def test_empty_batch_and_argument_errors(gpu):
    pi, a, b0 = random_model(5, 2, seed=9)
    h = cv.HMM(pi, a, b0, device=gpu)
    got = cv.loglik_grad_emissions(h, np.zeros(1, np.int64), np.zeros((0, 5)))
    assert got[1].shape == (5,) and not got[1].any() and not got[2].any() and got[3].shape == (0, 5)
    dev = torch.device("cuda", gpu)
    E = torch.zeros((3, 5), dtype=torch.float64, device=dev)
    narrow = torch.zeros((3, 4), dtype=torch.float64, device=dev)
    with pytest.raises(ValueError):
        on_device(h, np.array([0, 3]), E, grad_view=narrow)
    with pytest.raises(cv.CVError) as e:
        cv.loglik_grad_emissions(h, np.array([0, 3]), np.zeros((3, 5)), kernel="trellis")
    assert e.value.status == L.CV_EINVAL


# ---- 7. autograd -----------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [3, 65])
def test_autograd_against_the_torch_oracle(gpu, N):
    pi, a, b0 = random_model(N, 2, seed=9500 + N)
    if not np.isinf(a).any():
        a[0, N - 1] = -np.inf
    lengths = [9, 1, 4, 2, 12]
    off = offsets_of(lengths)
    E = feasible_scores(N, lengths, seed=9600 + N, ninf_frac=0.05)
    dev = torch.device("cuda", gpu)
    f = cv.autograd.sequence_loglik
    worst = 0.0
    for w in (np.ones(5), np.array([1.5, -2.0, 0.25, -0.5, 3.0])):
        ref, tg = np_grad(pi, a, E, off, w), torch_grad(pi, a, E, off, w)
        assert np.all(ref["status"] == L.SEQ_OK)
        em = torch.from_numpy(E).to(dev).requires_grad_(True)
        lp = torch.tensor(pi, requires_grad=True)  # on the CPU
        la = torch.tensor(a, device=dev, requires_grad=True)
        ll = f(em, off, lp, la)
        assert ll.shape == (5,) and ll.device == em.device and ll.requires_grad
        (ll.sum() if np.all(w == 1.0) else (ll * torch.from_numpy(w).to(dev)).sum()).backward()
        assert em.grad.shape == em.shape and lp.grad.device.type == "cpu" and la.grad.device == dev
        g = (lp.grad.numpy(), la.grad.cpu().numpy(), em.grad.cpu().numpy())
        both = dict(ref, pi=tg["pi"], a=tg["a"], e=tg["e"])  # the torch oracle's values, the bounds' |w| statistics
        ratios = grad_ratios(*g, both, off, N, w, 2.0) + grad_ratios(*g, ref, off, N, w, 2.0)
        assert max(ratios) <= 1.0, ratios
        worst = max(worst, *ratios)
        assert np.all(g[1][np.isinf(a)] == 0.0) and np.all(g[0][np.isinf(pi)] == 0.0) and np.all(g[2][np.isinf(E)] == 0.0)
        assert np.allclose(ll.detach().cpu().numpy(), tg["loglik"], rtol=1e-11, atol=1e-11)
    print(f"N={N}: autograd against the torch oracle, error / (2 x bound) = {worst:.4f}")


def test_autograd_plumbing(gpu):
    N = 65
    pi, a, b0 = random_model(N, 2, seed=9565)
    lengths = [9, 1, 4, 0, 12]
    off = offsets_of(lengths)
    E = feasible_scores(N, lengths, seed=9665, ninf_frac=0.05)
    E[off[2] + 1, 3] = np.nan  # BADOBS: its loglik is score_emissions', its gradient 0
    dev = torch.device("cuda", gpu)
    f = cv.autograd.sequence_loglik
    h = cv.HMM(pi, a, b0, device=gpu)
    lp, la = torch.tensor(pi), torch.tensor(a)
    # no input requires grad, and under no_grad: the scoring mode, no backward kernels
    em = torch.from_numpy(E).to(dev)
    for ctx_em in (em, em.clone().requires_grad_(True)):
        with torch.no_grad():
            ll = f(ctx_em, off, lp, la, hmm=h)
        torch.cuda.synchronize(dev)
        t = cv.last_timing(h)
        assert not ll.requires_grad and t["bt_ms"] == 0 and t["fwd_ms"] > 0, t
    ll0 = f(em, off, lp, la, hmm=h)
    assert not ll0.requires_grad and cv.last_timing(h)["bt_ms"] == 0
    score, status = cv.score_emissions(h, off, E)
    assert np.array_equal(bits(ll0.cpu().numpy()), bits(score))
    assert list(status) == [L.SEQ_OK, L.SEQ_OK, L.SEQ_BADOBS, L.SEQ_EMPTY, L.SEQ_OK]
    # inputs that do not require grad get None; flagged sequences a zero gradient whatever comes in
    em = torch.from_numpy(E).to(dev).requires_grad_(True)
    la_g = torch.tensor(a, requires_grad=True)
    ll, st = f(em, off, lp, la_g, hmm=h, return_status=True)
    assert np.array_equal(st.cpu().numpy(), status)
    upstream = torch.tensor([1.0, -2.0, float("nan"), float("inf"), 0.5], dtype=torch.float64, device=dev)
    ll.backward(upstream)
    assert lp.grad is None and la_g.grad is not None and cv.last_timing(h)["bt_ms"] > 0
    ge = em.grad.cpu().numpy()
    assert np.all(np.isfinite(ge)) and np.all(np.isfinite(la_g.grad.numpy())) and not ge[off[2]:off[3]].any()
    raw = cv.loglik_grad_emissions(h, off, E, weights=upstream.cpu().numpy())
    same_bits((ge, la_g.grad.numpy()), (raw[3], raw[2]), "backward is the raw call")
    only_pi = torch.tensor(pi, requires_grad=True)
    f(torch.from_numpy(E).to(dev), off, only_pi, la, hmm=h).sum().backward()
    same_bits((only_pi.grad.numpy(),), (cv.loglik_grad_emissions(h, off, E)[1],), "pi alone")
    # wider rows than N: the gradient has emis's shape, 0 beyond the N scores
    wide = torch.zeros((len(E), N + 2), dtype=torch.float64, device=dev)
    wide[:, :N] = torch.from_numpy(E).to(dev)
    wide.requires_grad_(True)
    f(wide, off, lp, la, hmm=h).backward(upstream)
    gw = wide.grad.cpu().numpy()
    assert gw.shape == (len(E), N + 2) and not gw[:, N:].any() and np.array_equal(bits(gw[:, :N]), bits(ge))
    # wrong arguments raise before any launch
    with pytest.raises(ValueError):
        f(em.detach().float(), off, lp, la)
    with pytest.raises(ValueError):
        f(em.detach()[:, :N - 1], off, lp, la)
    with pytest.raises(ValueError):
        f(em.detach(), [0, len(E) + 1], lp, la)
    with pytest.raises(ValueError):
        f(em.detach(), off, torch.tensor(pi[:3]), torch.tensor(a[:3, :3]), hmm=h)


def test_one_ascent_step_on_the_scores_does_not_lower_the_likelihood(gpu):
    N = 65
    pi, a, b0 = random_model(N, 2, seed=9765)
    lengths = [9, 1, 4, 2, 12]
    off = offsets_of(lengths)
    E = feasible_scores(N, lengths, seed=9865, ninf_frac=0.05)
    dev = torch.device("cuda", gpu)
    h = cv.HMM(pi, a, b0, device=gpu)
    lp, la = torch.tensor(pi), torch.tensor(a)
    em = torch.from_numpy(E).to(dev).requires_grad_(True)
    before = cv.autograd.sequence_loglik(em, off, lp, la, hmm=h).sum()
    before.backward()
    gain = 1e-3 * float((em.grad ** 2).sum())  # first order; the curvature term is of order 1e-6
    assert gain > 1e-4
    with torch.no_grad():
        after = cv.autograd.sequence_loglik(em + 1e-3 * em.grad, off, lp, la, hmm=h).sum()
    before, after = float(before.detach()), float(after)
    assert after > before and abs(after - before - gain) < 0.1 * gain, (before, after, gain)


# ---- 8. workspaces ---------------------------------------------------------------------------------
def test_release_workspaces_frees_everything(gpu):
    N = 65
    pi, a, b0, off, E, w, forced, _, _ = grad_case(N)
    h = cv.HMM(pi, a, b0, device=gpu)
    first = cv.posterior_emissions(h, off, E, gamma=True)  # builds the tables
    h.release_workspaces()
    before = cv.device_memory()["current"]
    h.set_tuning(xi_part_rows=8)
    cv.loglik_grad_emissions(h, off, E, weights=w, forced=forced)
    held = cv.device_memory()["current"]
    total = int(off[-1])
    assert held - before >= total * (3 * 128 * 8 + 12) + 128 * 128 * 8 * ((total + 7) // 8) + 70 * 128 * 8
    h.release_workspaces()
    assert cv.device_memory()["current"] == before
    again = cv.posterior_emissions(h, off, E, gamma=True)
    for u, v in zip(first, again):
        assert np.array_equal(bits(u), bits(v))
    h.release_workspaces()
