"""GPU: cv_gauss_emissions*, cv_expected_counts_gauss* and fit_gauss against tests/gauss_ref.py at
the bounds of include/cviterbi.h (u = 2^-53):
  |E - exact| <= (D + 8) u (kappa q + c_abs_j) + u |E|,
  |g_cnt - exact| <= (4 T (N + 8) + L + 1) u g_abs + 1e-290 L max(1, |w|max) max(1, |y|max^2),
  m1 with + 3 and m1_abs, m2 with + 5 and m2_abs,
"exact" for the statistics being exact sums for the scores E as cv_gauss_emissions returns them, so
the reference runs on those.  Beyond accuracy: the bit identities with gauss_emissions followed by
loglik_grad_emissions, host = device = repeat, NaN / inf rows, sentinel columns, chunk plans and
part sizes (tuning key gm_part_rows), nseq = 0, and EM's monotone likelihood.  Each test prints its
largest error-to-bound ratio (pytest -s)."""
import functools

import numpy as np
import pytest
import torch

import cviterbi as cv
import gauss_ref as G
from cviterbi import _lib as L
from grad_ref import a_grad_bound, emis_grad_bound, pi_grad_bound, row_weights
from test_posterior import loglik_bound, np_forward_backward, random_model

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F64 = dict(dtype=torch.float64, device=DEV)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


def same_bits(x, y, what=""):
    assert x.shape == y.shape and x.dtype == y.dtype, (what, x.shape, y.shape)
    assert np.array_equal(bits(x), bits(y)), (what, np.argwhere(~((x == y) | (np.isnan(x) & np.isnan(y))))[:5])


# ---- density -------------------------------------------------------------------------------------
def density_case(N, D, rows, seed):
    rng = np.random.default_rng(seed)
    mean = rng.normal(0.0, 2.0, size=(N, D))
    var = rng.uniform(0.3, 3.0, size=(N, D)) ** 2
    xw = np.full((rows, D + 2), 55.0)  # ldx = D + 2
    xw[:, :D] = rng.normal(0.0, 3.0, size=(rows, D))
    return xw[:, :D], mean, var


def density_device(h, x, mean, var, pad=3):
    """The _device variant on strided torch tensors -> (E [rows, N], the sentinel columns)."""
    rows, D, N = x.shape[0], x.shape[1], h.nstates()
    xw = torch.full((max(rows, 1), D + 2), 55.0, **F64)
    xw[:rows, :D] = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    out = torch.full((max(rows, 1), N + pad), 77.0, **F64)
    torch.cuda.synchronize(DEV)
    cv.gauss_emissions_device(h, xw[:, :D], mean, var, out[:, :N] if pad == 0 else out, rows=rows)
    torch.cuda.synchronize(DEV)
    o = out.cpu().numpy()
    return o[:rows, :N], o[:, N:]


@pytest.mark.parametrize("D", [1, 2, 16, 17, 33, 100])
@pytest.mark.parametrize("N", [1, 3, 64, 65, 257])
def test_density_within_bound(gpu, N, D):
    """Against 60-digit arithmetic where that is quick (N <= 3), else against the numpy restatement;
    L = 0, 1, 70; ldx > D and ld > N with the sentinel columns left alone; host = device = repeat."""
    rng = np.random.default_rng(N * 1000 + D)
    pi, a, _ = random_model(N, 1, seed=N + D)
    h = cv.gauss_hmm(pi, a, device=gpu)
    worst = 0.0
    for rows in (0, 1, 70):
        x, mean, var = density_case(N, D, rows, seed=rng.integers(1 << 30))
        assert rows == 0 or x.strides[0] == 8 * (D + 2)
        out = np.full((rows, N + 3), 77.0)
        E = cv.gauss_emissions(h, x, mean, var, out=out)[:, :N].copy()
        assert np.all(out[:, N:] == 77.0), "columns [N, ld) were written"
        Ed, sentinel = density_device(h, x, mean, var)
        assert np.all(sentinel == 77.0), "columns [N, ld) were written (device)"
        same_bits(E, Ed, "host vs device")
        same_bits(E, cv.gauss_emissions(h, x, mean, var), "repeat, ld = N")
        if rows == 0:
            continue
        exact = G.mp_density(x, mean, var) if N <= 3 else G.np_density(x, mean, var)
        worst = max(worst, G.within(E, exact, G.density_bound(x, mean, var, exact)))
    print(f"N={N} D={D}: error / bound = {worst:.3f}")
    assert worst <= 1.0


def test_density_hard_ranges(gpu):
    """An offset of 1e8 with sigma = 1e3, and sigma = 1e-150, against 60-digit arithmetic."""
    pi, a, _ = random_model(3, 1, seed=5)
    h = cv.gauss_hmm(pi, a, device=gpu)
    for D, offset, sigma in ((3, 1e8, 1e3), (17, 1e8, 1e3), (3, 0.0, 1e-150), (17, 0.0, 1e-150)):
        rng = np.random.default_rng(D)
        mean = offset + sigma * rng.normal(size=(3, D))
        var = (sigma * rng.uniform(1.0, 2.0, size=(3, D))) ** 2  # inside [1e-300, 1e300] at sigma = 1e-150
        x = offset + sigma * 2.0 * rng.normal(size=(5, D))
        E = cv.gauss_emissions(h, x, mean, var)
        exact = G.mp_density(x, mean, var)
        ratio = G.within(E, exact, G.density_bound(x, mean, var, exact))
        print(f"D={D} offset={offset} sigma={sigma}: error / bound = {ratio:.3f}")
        assert ratio <= 1.0


def test_density_bad_rows_and_overflow(gpu):
    N, D = 65, 17
    pi, a, _ = random_model(N, 1, seed=6)
    h = cv.gauss_hmm(pi, a, device=gpu)
    x, mean, var = density_case(N, D, 40, seed=7)
    clean = cv.gauss_emissions(h, x, mean, var)
    for bad in (np.nan, np.inf, -np.inf):
        xb = x.copy()
        xb[3, D - 1], xb[37, 0] = bad, bad
        E = cv.gauss_emissions(h, xb, mean, var)
        assert np.isnan(E[[3, 37]]).all(), bad
        keep = np.ones(40, bool)
        keep[[3, 37]] = False
        same_bits(E[keep], clean[keep], f"rows beside a {bad} row")
        same_bits(density_device(h, xb, mean, var)[0], E, "device")
    xo = x.copy()
    xo[5, 2] = mean[0, 2] + 1e200  # |x - mean| = 1e200: q overflows, -inf is a legal score
    E = cv.gauss_emissions(h, xo, mean, var)
    assert np.all(E[5] == -np.inf)
    keep = np.arange(40) != 5
    same_bits(E[keep], clean[keep], "rows beside the overflow")


def test_density_feeds_decode(gpu):
    """End to end: the two E agree within the bound, then decode_emissions on the library's E gives
    the paths and statuses of decode_emissions on the reference's E, and the scores agree to the
    sum of the bounds along a path."""
    N, D = 64, 16
    pi, a, _ = random_model(N, 1, seed=8)
    h = cv.gauss_hmm(pi, a, device=gpu)
    lens = [17, 1, 0, 33, 29]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    x, mean, var = density_case(N, D, int(off[-1]), seed=9)
    E = cv.gauss_emissions(h, x, mean, var)
    ref = G.np_density(x, mean, var)
    bound = G.density_bound(x, mean, var, ref)
    assert G.within(E, ref, bound) <= 1.0
    p1, s1, st1 = cv.decode_emissions(h, off, E)
    p2, s2, st2 = cv.decode_emissions(h, off, ref)
    assert np.array_equal(st1, st2) and np.array_equal(p1, p2)
    ok = st1 == L.SEQ_OK
    assert np.all(np.abs(s1 - s2)[ok] <= max(lens) * bound.max())


# ---- counts --------------------------------------------------------------------------------------
B = 70
NAN_SEQ, DEAD = 10, 30  # the sequence whose x holds a NaN; the infeasible one (a row of -inf scores)


def lengths70():
    """0 .. 40, every small length among them."""
    return [(7 * k + 3) % 41 for k in range(B)]


@functools.lru_cache(maxsize=None)
def case(N, D):
    """dict(pi, a, mean, var, off, x, w, forced, center), built once, shared, never modified: 70
    ragged sequences (an empty one among them) drawn around the means, one with a NaN in x, one
    infeasible, signed weights with a NaN on a sequence that is not OK, tags on a quarter."""
    pi, a, _ = random_model(N, 1, seed=5100 + 7 * N + D)
    rng = np.random.default_rng(5200 + 7 * N + D)
    lengths = lengths70()
    assert 0 in lengths and min(lengths[NAN_SEQ], lengths[DEAD]) >= 3
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    total = int(off[-1])
    # the means closer together at large D: the scores of a row stay within some tens of decades
    # of each other (an entry 300 decades below its row's largest is outside the contract of the
    # *_emissions entries)
    mean = rng.normal(0.0, 3.0 / np.sqrt(max(D / 8.0, 1.0)), size=(N, D))
    var = rng.uniform(0.5, 2.0, size=(N, D)) ** 2
    # a path the model allows per sequence (pi and A hold zeros): the tags below lie along it
    P, A = 10.0 ** pi, 10.0 ** a
    states = np.zeros(total, np.int64)
    for lo, hi in zip(off[:-1], off[1:]):
        z = rng.choice(N, p=P)
        for e in range(lo, hi):
            states[e] = z
            z = rng.choice(N, p=A[z])
    xw = np.full((total, D + 1), 55.0)  # ldx = D + 1
    xw[:, :D] = mean[states] + np.sqrt(var[states]) * rng.normal(size=(total, D)) + 10.0
    mean = mean + 10.0  # |mean| well above sigma: the centre matters
    x = xw[:, :D]
    center = x.mean(axis=0)
    x[off[NAN_SEQ] + 1, D // 2] = np.nan
    x[off[DEAD] + 2, 0] = 1e200
    forced = np.full(total, -1, np.int32)
    tag = rng.random(total) < 0.25
    forced[tag] = states[tag]
    w = rng.normal(0.0, 2.0, size=B)
    w[:2] = (-1.75, 0.5)
    w[DEAD] = np.nan
    for v in (pi, a, mean, var, off, xw, w, forced, center):
        v.setflags(write=False)
    return dict(pi=pi, a=a, mean=mean, var=var, off=off, x=x, w=w, forced=forced, center=center)


def reference(c, h, w=None, forced=None, center=None):
    """np_gauss_counts on the scores the library returns for the case's x."""
    E = cv.gauss_emissions(h, c["x"], c["mean"], c["var"])
    ref = G.np_gauss_counts(c["pi"], c["a"], E, c["off"], c["x"], w=w, forced=forced, center=center)
    st = ref["status"]
    assert st[NAN_SEQ] == G.SEQ_BADOBS and st[DEAD] == G.SEQ_INFEASIBLE and (st == G.SEQ_OK).sum() >= 50, st
    return E, ref


def check(got, ref, c, w=None):
    """(loglik, pi, a, g, m1, m2, gamma, status) against the reference's dict; the largest ratio."""
    off, N = c["off"], len(c["pi"])
    lens = np.diff(off)
    T, Ltot, nseq = int(lens.max()), int(lens.sum()), len(lens)
    wv = np.ones(nseq) if w is None else np.where(np.isfinite(w), w, 0.0)
    assert np.array_equal(got[7], ref["status"])
    for k in (1, 2, 3, 4, 5):
        assert np.isfinite(got[k]).all(), k
    bg, b1, b2 = G.moment_bounds(off, N, ref, wv)
    ratios = [G.within(got[3], ref["g"], bg), G.within(got[4], ref["m1"], b1), G.within(got[5], ref["m2"], b2),
              G.within(got[1], ref["pi"], pi_grad_bound(T, N, nseq, ref["pi_abs"])),
              G.within(got[2], ref["a"], a_grad_bound(T, N, Ltot, ref["a_abs"]))]
    if got[6] is not None:
        assert np.isfinite(got[6]).all()
        ratios.append(G.within(got[6], ref["gamma"], emis_grad_bound(T, N, ref["gamma_abs"], row_weights(off, wv))))
    assert max(ratios) <= 1.0, ratios
    return max(ratios)


def on_device(h, c, w=None, forced=None, center=None, gamma=True, nseq=None, **kw):
    """The _device variant on torch tensors (x strided) -> numpy results like the host wrapper's."""
    off = c["off"] if nseq is None else c["off"][:nseq + 1]
    nseq, total, N, D = len(off) - 1, int(off[-1]), h.nstates(), c["mean"].shape[1]
    xw = torch.full((max(total, 1), D + 1), 55.0, **F64)
    xw[:total, :D] = torch.from_numpy(np.ascontiguousarray(c["x"][:total])).to(DEV)
    off_d = torch.from_numpy(np.array(off, np.int64)).to(DEV)
    ll = torch.full((max(nseq, 1),), 77.0, **F64)
    st = torch.full((max(nseq, 1),), 9, dtype=torch.uint8, device=DEV)
    pg, ag, gg = torch.full((N,), 7.0, **F64), torch.full((N, N), 7.0, **F64), torch.full((N,), 7.0, **F64)
    m1, m2 = torch.full((N, D), 7.0, **F64), torch.full((N, D), 7.0, **F64)
    gm = torch.full((max(total, 1), N), 7.0, **F64) if gamma else None
    if forced is not None:
        kw["forced_dev"] = torch.from_numpy(np.array(forced, np.int32)).to(DEV)
    w_d = None if w is None else torch.from_numpy(np.array(w[:nseq], np.float64)).to(DEV)
    torch.cuda.synchronize(DEV)
    cv.expected_counts_gauss_device(h, off_d, xw[:, :D], c["mean"], c["var"], ll, pg, ag, gg, m1, m2, st, weight_dev=w_d,
                                    center=center, gamma_dev=gm, offsets_host=off, **kw)
    torch.cuda.synchronize(DEV)
    return (ll.cpu().numpy()[:nseq], pg.cpu().numpy(), ag.cpu().numpy(), gg.cpu().numpy(), m1.cpu().numpy(),
            m2.cpu().numpy(), gm.cpu().numpy()[:total] if gamma else None, st.cpu().numpy()[:nseq])


def all_same(x, y, what):
    for k, (u, v) in enumerate(zip(x, y)):
        if u is None or v is None:
            assert u is None and v is None, (what, k)
        else:
            same_bits(u, v, f"{what} [{k}]")


@pytest.mark.parametrize("D", [7, 8, 63, 64])
@pytest.mark.parametrize("N", [3, 64, 130, 300])
def test_counts_accuracy_and_bit_identities(gpu, N, D):
    c = case(N, D)
    h = cv.gauss_hmm(c["pi"], c["a"], device=gpu)
    args = (h, c["off"], c["x"], c["mean"], c["var"])
    # unit weights, no center, no tags
    E, ref = reference(c, h)
    plain = cv.expected_counts_gauss(*args, gamma=True)
    worst = check(plain, ref, c)
    # the definition: gauss_emissions, then loglik_grad_emissions (default workspace: one chunk each)
    pair = cv.loglik_grad_emissions(h, c["off"], E)
    all_same((plain[0], plain[1], plain[2], plain[6], plain[7]), pair, "the pair, unit weights")
    # signed weights (a NaN on a sequence that is not OK), a center, tags
    _, ref_w = reference(c, h, w=c["w"], forced=c["forced"], center=c["center"])
    kw = dict(weight=c["w"], center=c["center"], forced=c["forced"])
    full = cv.expected_counts_gauss(*args, gamma=True, **kw)
    worst = max(worst, check(full, ref_w, c, c["w"]))
    pair = cv.loglik_grad_emissions(h, c["off"], E, weights=c["w"], forced=c["forced"])
    all_same((full[0], full[1], full[2], full[6], full[7]), pair, "the pair, weights and tags")
    assert np.all(full[6][c["off"][NAN_SEQ]:c["off"][NAN_SEQ + 1]] == 0.0)
    assert np.all(full[6][c["off"][DEAD]:c["off"][DEAD + 1]] == 0.0)
    # repeats, the device variant, and without gamma (the rows go through the workspace, stride NP)
    all_same(cv.expected_counts_gauss(*args, gamma=True, **kw), full, "repeat")
    all_same(on_device(h, c, c["w"], c["forced"], c["center"]), full, "device")
    nog = cv.expected_counts_gauss(*args, **kw)
    assert nog[6] is None
    worst = max(worst, check(nog, ref_w, c, c["w"]))
    all_same(on_device(h, c, c["w"], c["forced"], c["center"], gamma=False), nog, "device, no gamma")
    all_same((nog[0], nog[7]), (full[0], full[7]), "loglik and status without gamma")
    print(f"N={N} D={D}: worst error / bound = {worst:.3g}")


def test_generic_kernels_below_257(gpu):
    c = case(64, 8)
    h = cv.gauss_hmm(c["pi"], c["a"], device=gpu)
    _, ref_w = reference(c, h, w=c["w"], forced=c["forced"], center=c["center"])
    got = cv.expected_counts_gauss(h, c["off"], c["x"], c["mean"], c["var"], weight=c["w"], center=c["center"],
                                   forced=c["forced"], gamma=True, kernel="generic")
    print(f"generic N=64: {check(got, ref_w, c, c['w']):.3g}")


def test_nan_sequence_equals_the_run_without_it(gpu):
    """The sequence whose x holds a NaN is BADOBS and counts nothing: every output is finite, the
    other sequences' loglik, status and gamma rows are those of the batch without it bit for bit,
    and the sums are within their bounds of that batch's reference."""
    N, D = 64, 8
    c = case(N, D)
    h = cv.gauss_hmm(c["pi"], c["a"], device=gpu)
    lo, hi = int(c["off"][NAN_SEQ]), int(c["off"][NAN_SEQ + 1])
    keep_seq = np.arange(B) != NAN_SEQ
    keep_row = np.ones(int(c["off"][-1]), bool)
    keep_row[lo:hi] = False
    lens = np.diff(c["off"])[keep_seq]
    c2 = dict(c, off=np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), x=c["x"][keep_row], w=c["w"][keep_seq],
              forced=c["forced"][keep_row])
    kw = lambda d: dict(weight=d["w"], center=d["center"], forced=d["forced"], gamma=True)  # noqa: E731
    got = cv.expected_counts_gauss(h, c["off"], c["x"], c["mean"], c["var"], **kw(c))
    assert got[7][NAN_SEQ] == G.SEQ_BADOBS and np.isnan(got[0][NAN_SEQ])
    without = cv.expected_counts_gauss(h, c2["off"], c2["x"], c2["mean"], c2["var"], **kw(c2))
    same_bits(got[0][keep_seq], without[0], "loglik")
    same_bits(got[7][keep_seq], without[7], "status")
    same_bits(got[6][keep_row], without[6], "gamma")
    E2 = cv.gauss_emissions(h, c2["x"], c2["mean"], c2["var"])
    ref2 = G.np_gauss_counts(c2["pi"], c2["a"], E2, c2["off"], c2["x"], w=c2["w"], forced=c2["forced"], center=c2["center"])
    got2 = tuple(g[keep_seq] if k in (0, 7) else g[keep_row] if k == 6 else g for k, g in enumerate(got))
    print(f"with the NaN sequence vs the reference without it: {check(got2, ref2, c2, c2['w']):.3g}")


@pytest.mark.parametrize("N,D", [(64, 8), (130, 63), (300, 7)])
def test_chunks_and_parts(gpu, N, D):
    """Several chunks (a small workspace_bytes) and several parts (gm_part_rows 4 and 7): within the
    bounds, repeated bit for bit; loglik, status and gamma bit-identical to the one-chunk run."""
    c = case(N, D)
    h = cv.gauss_hmm(c["pi"], c["a"], device=gpu)
    args = (h, c["off"], c["x"], c["mean"], c["var"])
    kw = dict(weight=c["w"], center=c["center"], forced=c["forced"], gamma=True)
    _, ref_w = reference(c, h, w=c["w"], forced=c["forced"], center=c["center"])
    base = cv.expected_counts_gauss(*args, **kw)
    np_ = (N + 63) // 64 * 64
    # a quarter of the cap is left to the rows: about 100 elements of (5 rows of NP + 16 bytes)
    small = 4 * 100 * (5 * 8 * np_ + 16)
    worst = 0.0
    for label, ws, key in (("chunks", small, 0), ("parts of 4", 0, 4), ("parts of 7", 0, 7), ("both", small, 7)):
        with h.tuned(gm_part_rows=key):
            got = cv.expected_counts_gauss(*args, workspace_bytes=ws, **kw)
            launches = cv.last_timing(h)["launches"]
            again = cv.expected_counts_gauss(*args, workspace_bytes=ws, **kw)
        assert (launches > 4) == (ws > 0), (label, launches)
        worst = max(worst, check(got, ref_w, c, c["w"]))
        all_same(again, got, f"repeat, {label}")
        all_same((got[0], got[6], got[7]), (base[0], base[6], base[7]), f"loglik, gamma, status, {label}")
        nog = cv.expected_counts_gauss(*args, workspace_bytes=ws, **dict(kw, gamma=False))
        worst = max(worst, check(nog, ref_w, c, c["w"]))
    assert h.tuning("gm_part_rows") == 0
    # a value the header does not list: negative is "by rule" (harmless), beyond int32 is rejected
    with h.tuned(gm_part_rows=-5):
        all_same(cv.expected_counts_gauss(*args, **kw), base, "gm_part_rows = -5")
    with pytest.raises(cv.CVError, match="EINVAL"):
        h.set_tuning(gm_part_rows=1 << 40)
    print(f"N={N} D={D}: worst error / bound over plans = {worst:.3g}")


def test_empty_batch_writes_zeros(gpu):
    c = case(3, 7)
    h = cv.gauss_hmm(c["pi"], c["a"], device=gpu)
    got = on_device(h, c, nseq=0)
    for k in (1, 2, 3, 4, 5):
        assert np.all(got[k] == 0.0), k
    host = cv.expected_counts_gauss(h, np.zeros(1, np.int64), np.zeros((0, 7)), c["mean"], c["var"])
    for k in (1, 2, 3, 4, 5):
        assert np.all(host[k] == 0.0), k


def test_release_frees_the_new_workspaces(gpu):
    c = case(64, 8)
    h = cv.gauss_hmm(c["pi"], c["a"], device=gpu)
    cv.expected_counts_gauss(h, c["off"], c["x"], c["mean"], c["var"])  # the model's own tables are built
    h.release_workspaces()
    idle = cv.device_memory()["current"]
    cv.expected_counts_gauss(h, c["off"], c["x"], c["mean"], c["var"])
    assert cv.device_memory()["current"] > idle
    h.release_workspaces()
    assert cv.device_memory()["current"] <= idle  # the tables, the partial tiles, the accumulator, the flags


# ---- EM ------------------------------------------------------------------------------------------
def test_fit_gauss_five_rounds(gpu):
    """N = 4, D = 2, 64 sequences of T = 50 from a known model: every round's statistics within the
    bounds of the reference on that round's own parameters, and the total log-likelihood never
    drops by more than the sum of posterior_batch's loglik bounds over the batch."""
    N, D, nseq, T = 4, 2, 64, 50
    rng = np.random.default_rng(77)
    pi_t = np.full(N, 1.0 / N)
    a_t = np.full((N, N), 0.1 / (N - 1)) + np.eye(N) * (0.9 - 0.1 / (N - 1))
    mean_t = np.array([[0.0, 0.0], [4.0, 0.0], [0.0, 4.0], [4.0, 4.0]]) + 20.0
    var_t = np.array([[0.5, 1.0], [1.0, 0.5], [0.8, 0.8], [1.5, 0.4]])
    off = np.arange(nseq + 1, dtype=np.int64) * T
    x = np.zeros((nseq * T, D))
    for s in range(nseq):
        z = rng.choice(N, p=pi_t)
        for t in range(T):
            x[s * T + t] = mean_t[z] + np.sqrt(var_t[z]) * rng.normal(size=D)
            z = rng.choice(N, p=a_t[z])
    pi0 = np.log10(rng.dirichlet(np.ones(N) * 5))
    a0 = np.log10(rng.dirichlet(np.ones(N) * 5, size=N))
    mean0 = x[rng.choice(len(x), N, replace=False)]
    var0 = np.tile(x.var(axis=0), (N, 1))
    history = []
    pi, a, mean, var, lls = cv.fit_gauss(pi0, a0, mean0, var0, off, x, rounds=5, device=gpu, history=history)
    assert len(lls) == 5 and len(history) == 5
    worst, tol = 0.0, []
    for r in history:
        h = cv.gauss_hmm(r["pi"], r["a"], device=gpu)
        E = cv.gauss_emissions(h, x, r["mean"], r["var"])
        ref = G.np_gauss_counts(r["pi"], r["a"], E, off, x, center=r["center"])
        assert np.all(r["status"] == G.SEQ_OK) and np.array_equal(ref["status"], r["status"])
        bg, b1, b2 = G.moment_bounds(off, N, ref)
        worst = max(worst, G.within(r["g_cnt"], ref["g"], bg), G.within(r["m1"], ref["m1"], b1),
                    G.within(r["m2"], ref["m2"], b2),
                    G.within(r["pi_cnt"], ref["pi"], pi_grad_bound(T, N, nseq, ref["pi_abs"])),
                    G.within(r["a_cnt"], ref["a"], a_grad_bound(T, N, nseq * T, ref["a_abs"])))
        S = [np_forward_backward(r["pi"], r["a"], E[lo:hi].T, np.arange(hi - lo))[2] for lo, hi in zip(off[:-1], off[1:])]
        tol.append(sum(loglik_bound(T, N, s) for s in S))
    print(f"EM: worst error / bound = {worst:.3g}; loglik per round {lls}; tolerances {tol}")
    assert worst <= 1.0
    for r in range(1, 5):
        assert lls[r] >= lls[r - 1] - tol[r], (r, lls, tol)
    assert lls[-1] > lls[0]
    assert np.isfinite(pi).any() and np.isfinite(a).any() and np.isfinite(mean).all() and np.all(var >= 1e-6)
