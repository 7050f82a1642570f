"""GPU: cv_sample_batch / cv_sample_batch_device (posterior path sampling, FFBS).  The main check
walks every GPU path backwards and conditions the numpy f64 oracle's CDF (tests/sample_ref.py) on
the GPU's own next state: the uniform of the pick must lie inside the picked state's CDF interval
within 2 eps(T, N) = 2 x 4 (T + 1) (N + 8) 2^-53 -- the GPU's bound plus the oracle's -- and the
picked state must have a positive weight.  Beyond it: scores equal to the f64 fold bit for bit,
draws keyed on (seed, sequence, draw) only, bit-identical variants and chunkings, tags, statuses
that disturb no neighbour, timing, release, and one handle shared with the other entries.
Each accuracy test prints its largest distance-to-bound ratio (pytest -s)."""
import ctypes
import functools

import numpy as np
import pytest

import cviterbi as cv
import handle_ops as ops
import sample_ref as sr
from cviterbi import _lib as L
from kbest_ref import fold_score
from test_gpu_posterior import covering_tags, kernels_of, offsets_of, tag_classes
from test_posterior import np_forward_backward, random_model

pytestmark = pytest.mark.gpu

RAGGED = (1, 2, 7, 33, 64)


def ragged(B):
    return [RAGGED[(3 * k + k // 5) % 5] for k in range(B)]


@functools.lru_cache(maxsize=None)
def case(N, B, V=6, lengths=None):
    """(pi, a, b, off, obs, rows) of a seeded model and batch: built once, shared, never modified.
    rows[k] = the numpy f64 forward rows of sequence k."""
    pi, a, b = random_model(N, V, seed=6100 + N)
    lengths = list(lengths) if lengths else ragged(B)
    off = offsets_of(lengths)
    obs = sr.model_sequences(pi, a, b, lengths, seed=N + B)
    P, A, Bm = sr.prob_tables(pi, a, b)
    rows = [sr.forward_rows(P, A, Bm, obs[off[k]:off[k + 1]]) for k in range(len(lengths))]
    for x in (pi, a, b, off, obs, A):
        x.setflags(write=False)
    return pi, a, b, off, obs, rows, A


def fold_scores(pi, a, b, obs, paths):
    """The reference's fold along each of paths[R, T], vectorised over the draws (f64)."""
    with np.errstate(invalid="ignore"):
        d = pi[paths[:, 0]] + b[paths[:, 0], obs[0]]
        for t in range(1, paths.shape[1]):
            d = (d + a[paths[:, t - 1], paths[:, t]]) + b[paths[:, t], obs[t]]
    return d


def check_draws(model, got, seed, seq_base=0, rows=None, forced=None):
    """Every draw of every sequence: the interval check at 2 eps, finite scores equal to the fold
    bit for bit.  Returns the largest distance / (2 eps)."""
    pi, a, b, off, obs, base_rows, A = model
    paths, scores, loglik, status = got
    R = paths.shape[0]
    N = len(pi)
    worst = 0.0
    for k in range(len(off) - 1):
        lo, hi = int(off[k]), int(off[k + 1])
        T = hi - lo
        if T == 0:
            continue
        assert status[k] == L.SEQ_OK, (k, status[k])
        alpha = (rows or base_rows)[k]
        us = cv.sample.uniform(seed, seq_base + k, np.arange(R, dtype=np.uint64)[:, None],
                               np.arange(T, dtype=np.uint64)[None, :])
        p = paths[:, lo:hi]
        if forced is not None:
            tagged = forced[lo:hi] >= 0
            assert np.all(p[:, tagged] == forced[lo:hi][tagged][None, :]), k
        d = sr.interval_ratio(alpha, A, p, us) / (2 * sr.eps(T, N))
        assert d <= 1.0, (k, T, N, d)
        worst = max(worst, d)
        if scores is not None:
            ref = fold_scores(pi, a, b, obs[lo:hi], p)
            assert np.all(np.isfinite(scores[:, k])), (k, scores[:, k])
            assert np.array_equal(scores[:, k].view(np.int64), ref.view(np.int64)), k
    return worst


def test_vectorised_fold_is_the_reference_fold(gpu):
    pi, a, b, off, obs, _, _ = case(20, 33)
    h = cv.HMM(pi, a, b, device=gpu)
    paths, scores, _, _ = cv.sample_batch(h, off, obs, 3, seed=1)
    for k in (0, 4, 32):
        lo, hi = int(off[k]), int(off[k + 1])
        for r in range(3):
            assert scores[r, k] == fold_score(pi, a, b, obs[lo:hi], paths[r, lo:hi])


# ---- the interval test -------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["auto", "generic"])
@pytest.mark.parametrize("N", [1, 3, 64, 65, 130, 192, 193, 256])
def test_interval_one_wave_sizes(gpu, N, kernel):
    worst = 0.0
    h = None
    for B, R in ((1, 64), (33, 8), (70, 1)):
        model = case(N, B)
        h = h or cv.HMM(*model[:3], device=gpu)
        got = cv.sample_batch(h, model[3], model[4], R, seed=40 + R, kernel=kernel)
        t = cv.last_timing(h)
        assert t["kernel"] == ("generic" if kernel == "generic" else "none"), t
        assert (t["seqs_per_wave"] == 32) == (kernel == "auto"), t
        worst = max(worst, check_draws(model, got, 40 + R))
    print(f"N={N} {kernel}: distance / (2 eps) = {worst:.5f}")


@pytest.mark.parametrize("N", [257, 300, 1030])
def test_interval_plain_kernel(gpu, N):
    worst = 0.0
    h = None
    for B, R in ((33, 8), (1, 64), (70, 1)):
        model = case(N, B)
        h = h or cv.HMM(*model[:3], device=gpu)
        got = cv.sample_batch(h, model[3], model[4], R, seed=7)
        assert cv.last_timing(h)["kernel"] == "generic"
        worst = max(worst, check_draws(model, got, 7))
    print(f"N={N}: distance / (2 eps) = {worst:.5f}")


@pytest.mark.parametrize("N", [3073, 4096])
def test_interval_at_the_state_limit(gpu, N):
    model = case(N, 2, 3, (6, 6))
    h = cv.HMM(*model[:3], device=gpu)
    got = cv.sample_batch(h, model[3], model[4], 8, seed=N)
    print(f"N={N}: distance / (2 eps) = {check_draws(model, got, N):.5f}")


# ---- feasibility ---------------------------------------------------------------------------------------
def test_draws_are_feasible_where_the_max_marginal_path_is_not(gpu):
    """A model (60% zeros, found on the CPU with the numpy oracle) whose per-element argmax of gamma
    crosses a zero transition: posterior_batch's path folds to -inf, all 64 sampled paths are finite."""
    pi, a, b = random_model(6, 3, 7006, zero_frac=0.6)
    obs = sr.model_sequences(pi, a, b, [14], 7006)
    off = offsets_of([14])
    ll, gm, _ = np_forward_backward(pi, a, b, obs)
    assert np.isfinite(ll)
    with np.errstate(invalid="ignore"):
        assert fold_score(pi, a, b, obs, gm.argmax(axis=1)) == -np.inf
    h = cv.HMM(pi, a, b, device=gpu)
    _, ppath, _, st = cv.posterior_batch(h, off, obs)
    assert st[0] == L.SEQ_OK and np.array_equal(ppath, gm.argmax(axis=1))
    for kernel in ("auto", "generic"):
        paths, scores, loglik, st = cv.sample_batch(h, off, obs, 64, seed=5, kernel=kernel)
        assert st[0] == L.SEQ_OK and np.all(np.isfinite(scores))
        assert abs(loglik[0] - ll) < 1e-9
        assert np.all(scores[:, 0] <= loglik[0] + 1e-9)  # a path's joint never exceeds the total
        assert np.array_equal(scores[:, 0], fold_scores(pi, a, b, obs, paths))
        assert len({p.tobytes() for p in paths}) > 1


def test_zero_weights_are_never_picked(gpu):
    """The first states have weight 0 at the last element (no emission of the last observation),
    and the tag j at the last-but-one element has A[i][j] = 0 for the first states i: a scan whose
    prefix starts at 0 must not return them, however small u is."""
    N, V, T = 70, 4, 9
    pi, a, b = random_model(N, V, seed=77, zero_frac=0.0)
    b[:5, V - 1] = -np.inf  # states 0..4 never emit the last observation
    j = 66
    a[:7, j] = -np.inf      # states 0..6 never move to j
    rng = np.random.default_rng(3)
    lengths = [T] * 4 + [1]
    obs = rng.integers(0, V - 1, size=sum(lengths)).astype(np.int32)
    off = offsets_of(lengths)
    obs[off[1:] - 1] = V - 1
    forced = np.full(len(obs), -1, np.int32)
    forced[off[:4] + T - 2] = j
    h = cv.HMM(pi, a, b, device=gpu)
    for kernel in ("auto", "generic"):
        paths, scores, _, st = cv.sample_batch(h, off, obs, 64, seed=9, forced=forced, kernel=kernel)
        assert np.all(st == L.SEQ_OK) and np.all(np.isfinite(scores))
        assert np.all(paths[:, off[1:] - 1] >= 5)
        assert np.all(paths[:, off[:4] + T - 2] == j) and np.all(paths[:, off[:4] + T - 3] >= 7)


# ---- exact cases ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [17, 130, 256, 300])
def test_all_tags_forced_gives_the_tags(gpu, N):
    pi, a, b = random_model(N, 5, seed=5)
    lengths = [33, 5, 1]
    off = offsets_of(lengths)
    obs = sr.model_sequences(pi, a, b, lengths, seed=5)
    h = cv.HMM(pi, a, b, device=gpu)
    path, score, st = cv.decode_batch(h, off, obs, dtype="f64")  # score: the f64 fold along the path
    assert np.all(st == L.SEQ_OK)
    for kernel in kernels_of(N):
        paths, scores, _, s = cv.sample_batch(h, off, obs, 8, seed=N, forced=path, kernel=kernel)
        assert np.all(s == L.SEQ_OK)
        assert np.array_equal(paths, np.broadcast_to(path, paths.shape))
        assert np.array_equal(scores, np.broadcast_to(score, scores.shape))


@pytest.mark.parametrize("N", [5, 200, 300])
def test_permutation_model_has_one_path(gpu, N):
    rng = np.random.default_rng(N)
    perm, emit = rng.permutation(N), rng.permutation(N)
    pi = np.full(N, -np.inf)
    pi[3] = 0.0
    a = np.full((N, N), -np.inf)
    a[np.arange(N), perm] = 0.0
    b = np.full((N, N), -np.inf)
    b[np.arange(N), emit] = 0.0
    lengths = [40, 1, 7]
    states = []
    for T in lengths:
        s = [3]
        for _ in range(T - 1):
            s.append(perm[s[-1]])
        states.append(np.array(s, np.int32))
    truth = np.concatenate(states)
    obs = emit[truth].astype(np.int32)
    off = offsets_of(lengths)
    h = cv.HMM(pi, a, b, device=gpu)
    for kernel in kernels_of(N):
        paths, scores, loglik, st = cv.sample_batch(h, off, obs, 8, seed=1, kernel=kernel)
        assert np.all(st == L.SEQ_OK)
        assert np.array_equal(paths, np.broadcast_to(truth, paths.shape))
        assert np.all(scores == 0.0) and np.all(np.abs(loglik) < 1e-12)


# ---- keying --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [20, 256, 300])
def test_draws_are_keyed_on_seed_sequence_and_draw_only(gpu, N):
    pi, a, b, off, obs, _, _ = case(N, 33)
    h = cv.HMM(pi, a, b, device=gpu)
    p8, s8, _, _ = cv.sample_batch(h, off, obs, 8, seed=12, seq_base=100)
    for R in (1, 2, 3):  # one, two, four (of which three used) and eight draws a wave
        pr, srr, _, _ = cv.sample_batch(h, off, obs, R, seed=12, seq_base=100)
        assert np.array_equal(pr, p8[:R]) and np.array_equal(srr, s8[:R])
    p64, s64, _, _ = cv.sample_batch(h, off, obs, 64, seed=12, seq_base=100)
    assert np.array_equal(p64[:8], p8) and np.array_equal(s64[:8], s8)
    for k in (0, 7, 32):
        lo, hi = int(off[k]), int(off[k + 1])
        p1, s1, _, _ = cv.sample_batch(h, [0, hi - lo], obs[lo:hi], 8, seed=12, seq_base=100 + k)
        assert np.array_equal(p1, p8[:, lo:hi]) and np.array_equal(s1[:, 0], s8[:, k])
    other, _, _, _ = cv.sample_batch(h, off, obs, 8, seed=13, seq_base=100)
    assert not np.array_equal(other, p8)
    shifted, _, _, _ = cv.sample_batch(h, off, obs, 8, seed=12, seq_base=101)
    assert not np.array_equal(shifted, p8)
    assert len({p.tobytes() for p in p8}) > 1


# ---- bit identity: variants, repeats, chunks ---------------------------------------------------------------
@pytest.mark.parametrize("N", [20, 130, 256])
def test_variants_repeats_and_chunks_are_bit_identical(gpu, N):
    import torch

    model = case(N, 33)
    pi, a, b, off, obs = model[:5]
    h = cv.HMM(pi, a, b, device=gpu)
    R = 5
    first = cv.sample_batch(h, off, obs, R, seed=3)
    assert cv.last_timing(h)["launches"] == 1
    check_draws(model, first, 3)
    again = cv.sample_batch(h, off, obs, R, seed=3)
    NP = (N + 63) // 64 * 64
    chunked = cv.sample_batch(h, off, obs, R, seed=3, workspace_bytes=NP * 8 * 150)
    assert cv.last_timing(h)["launches"] >= 3
    for other in (again, chunked):
        for x, y in zip(first, other):
            assert x.tobytes() == y.tobytes()
    dev = torch.device("cuda", gpu)
    total, B = int(off[-1]), len(off) - 1
    d_off, d_obs = torch.from_numpy(off.copy()).to(dev), torch.from_numpy(obs.copy()).to(dev)
    d_path = torch.full((R, total), -7, dtype=torch.int32, device=dev)
    d_score = torch.full((R, B), 7.5, dtype=torch.float64, device=dev)
    d_ll = torch.zeros(B, dtype=torch.float64, device=dev)
    d_st = torch.full((B,), 9, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    for host_off, ll in ((off, d_ll), (None, None)):
        cv.sample_batch_device(h, d_off, d_obs, R, d_path, d_st, d_score, ll, seed=3, offsets_host=host_off,
                               stream=stream.cuda_stream)
        stream.synchronize()
        assert np.array_equal(d_path.cpu().numpy(), first[0])
        assert d_score.cpu().numpy().tobytes() == first[1].tobytes()
        assert np.array_equal(d_ll.cpu().numpy(), first[2])
        assert np.array_equal(d_st.cpu().numpy(), first[3])
        d_path.fill_(-7), d_score.fill_(7.5)
        torch.cuda.synchronize(dev)
    # without scores: the same paths
    nos = cv.sample_batch(h, off, obs, R, seed=3, scores=False)
    assert nos[1] is None and np.array_equal(nos[0], first[0])


# ---- partial tags beyond the first tile / stride -----------------------------------------------------------
@pytest.mark.parametrize("N", [130, 256, 300])
def test_partial_tags_hold_in_every_draw(gpu, N):
    pi, a, b = random_model(N, 4, seed=4000 + N)
    lengths = [12, 1, 5, 2]
    off = offsets_of(lengths)
    obs = sr.model_sequences(pi, a, b, lengths, seed=N)
    h = cv.HMM(pi, a, b, device=gpu)
    path, _, st = cv.decode_batch(h, off, obs, dtype="f64")
    assert np.all(st == L.SEQ_OK)
    forced = covering_tags(pi, a, b, off, obs, path, tag_classes(N))
    tagged = np.nonzero(forced >= 0)[0]
    P, A, Bm = sr.prob_tables(pi, a, b)
    rows = [sr.forward_rows(P, A, Bm, obs[off[k]:off[k + 1]], forced[off[k]:off[k + 1]]) for k in range(len(lengths))]
    model = (pi, a, b, off, obs, rows, A)
    for kernel in kernels_of(N):
        got = cv.sample_batch(h, off, obs, 16, seed=N, forced=forced, kernel=kernel)
        assert np.array_equal(got[0][:, tagged], np.broadcast_to(forced[tagged], (16, len(tagged)))), kernel
        check_draws(model, got, N, forced=forced)
        assert (got[0][:, forced < 0] != path[forced < 0]).any()  # the free elements do vary


# ---- statuses ----------------------------------------------------------------------------------------------
def test_statuses_and_neighbours(gpu):
    N, V, R = 5, 4, 6
    pi, a, b = random_model(N, V, seed=9, zero_frac=0.0)
    b[2, 1] = -np.inf  # state 2 never emits observation 1: a tag of 2 there is infeasible
    good = [np.array([0, 1, 2, 1, 0], np.int32), np.array([2], np.int32), np.array([1, 1, 0, 2, 2, 0, 1], np.int32)]
    seqs = [good[0], np.array([0, 1, 3], np.int32), good[1], np.zeros(0, np.int32), np.array([1, 99, 0, -4], np.int32),
            good[2]]
    off = offsets_of([len(s) for s in seqs])
    obs = np.concatenate(seqs)
    forced = np.full(len(obs), -1, np.int32)
    forced[off[1] + 1] = 2
    h = cv.HMM(pi, a, b, device=gpu)
    expect = [L.SEQ_OK, L.SEQ_INFEASIBLE, L.SEQ_OK, L.SEQ_EMPTY, L.SEQ_BADOBS, L.SEQ_OK]
    for kernel in ("auto", "generic"):
        paths, scores, ll, st = cv.sample_batch(h, off, obs, R, seed=2, seq_base=10, forced=forced, kernel=kernel)
        assert list(st) == expect
        assert ll[1] == -np.inf and ll[3] == 0.0 and np.isnan(ll[4])
        assert np.all(paths[:, off[1]:off[2]] == -1) and np.all(scores[:, 1] == -np.inf)
        assert np.all(paths[:, off[4]:off[5]] == -1) and np.all(np.isnan(scores[:, 4]))
        for k in (0, 2, 5):  # the neighbours: the same sequence alone under its own global index
            alone = cv.sample_batch(h, [0, len(seqs[k])], seqs[k], R, seed=2, seq_base=10 + k, kernel=kernel)
            assert np.all(alone[3] == L.SEQ_OK)
            assert np.array_equal(alone[0], paths[:, off[k]:off[k + 1]])
            assert np.array_equal(alone[1][:, 0], scores[:, k]) and alone[2][0] == ll[k]
    # the C call reports the infeasible sequence after writing every output; the slots of the empty
    # sequence are left alone
    o = L.opts(L.DTYPE_F64)
    o.forced = forced.ctypes.data
    pc = np.full((R, len(obs)), -7, np.int32)
    sc, llc, stc = np.full((R, 6), 7.5), np.full(6, 7.5), np.full(6, 9, np.uint8)
    rc = L.lib().cv_sample_batch(h.handle, 6, off.ctypes.data, obs.ctypes.data, R, 2, 10, ctypes.byref(o),
                                 pc.ctypes.data, sc.ctypes.data, llc.ctypes.data, stc.ctypes.data)
    assert rc == L.CV_EINFEASIBLE and list(stc) == expect
    assert np.all(sc[:, 3] == 7.5) and np.all(sc[:, 1] == -np.inf) and np.all(np.isfinite(sc[:, [0, 2, 5]]))
    assert not (pc == -7).any() and llc[3] == 0.0


def test_statuses_of_the_device_variant(gpu):
    import torch

    N, V, R = 5, 4, 3
    pi, a, b = random_model(N, V, seed=9, zero_frac=0.0)
    seqs = [np.array([0, 1, 2], np.int32), np.zeros(0, np.int32), np.array([1, 99], np.int32), np.array([2, 2], np.int32)]
    off = offsets_of([len(s) for s in seqs])
    obs = np.concatenate(seqs)
    dev = torch.device("cuda", gpu)
    h = cv.HMM(pi, a, b, device=gpu)
    d_off, d_obs = torch.from_numpy(off).to(dev), torch.from_numpy(obs).to(dev)
    d_path = torch.full((R, len(obs)), -7, dtype=torch.int32, device=dev)
    d_score = torch.full((R, 4), 7.5, dtype=torch.float64, device=dev)
    d_st = torch.full((4,), 9, dtype=torch.uint8, device=dev)
    cv.sample_batch_device(h, d_off, d_obs, R, d_path, d_st, d_score, seed=4, offsets_host=off)
    torch.cuda.synchronize(dev)
    st, sc, pt = d_st.cpu().numpy(), d_score.cpu().numpy(), d_path.cpu().numpy()
    assert list(st) == [L.SEQ_OK, L.SEQ_EMPTY, L.SEQ_BADOBS, L.SEQ_OK]
    assert np.all(sc[:, 1] == 7.5) and np.all(np.isnan(sc[:, 2])) and np.all(np.isfinite(sc[:, [0, 3]]))
    assert np.all(pt[:, off[2]:off[3]] == -1) and np.all(pt[:, :3] >= 0) and np.all(pt[:, 5:] >= 0)
    host = cv.sample_batch(h, off, obs, R, seed=4)
    assert np.array_equal(host[0], pt) and np.array_equal(host[3], st)


# ---- timing, release, one handle across entries --------------------------------------------------------------
def test_timing_and_release_workspaces(gpu):
    pi, a, b, off, obs, _, _ = case(20, 33)
    h = cv.HMM(pi, a, b, device=gpu)
    cv.sample_batch(h, off, obs, 4, seed=1)  # builds the tables, which stay
    h.release_workspaces()
    level = cv.device_memory()["current"]
    cv.sample_batch(h, off, obs, 4, seed=1)
    t = cv.last_timing(h)
    assert t["fwd_ms"] > 0 and t["bt_ms"] > 0 and t["total_ms"] >= t["fwd_ms"] and t["launches"] == 1
    assert t["seqs_per_wave"] == 32 and t["padded_states"] == 64
    rows_bytes = int(off[-1]) * 64 * 8
    assert cv.device_memory()["current"] - level >= rows_bytes
    h.release_workspaces()
    assert cv.device_memory()["current"] == level
    again = cv.sample_batch(h, off, obs, 4, seed=1)  # the handle still works
    assert np.all(again[3] == L.SEQ_OK)
    h.release_workspaces()


@pytest.mark.parametrize("name", ["n40", "n256", "n300"])
def test_one_handle_interleaved_with_other_entries(gpu, name):
    """Sampling between the other entries of one handle changes neither their results nor its own."""
    x = ops.inputs(name, "small")
    h = ops.new_handle(name)
    fresh = {op: ops.run(name, op, ops.new_handle(name), "small") for op in ("f64_viterbi", "posterior_gamma", "kbest3")}

    def sample():
        return tuple(v for v in cv.sample_batch(h, x.off, x.obs_ok, 8, seed=21, seq_base=5))

    ref = sample()
    for op in ("f64_viterbi", "posterior_gamma", "kbest3", "posterior_gamma", "f64_viterbi"):
        assert ops.first_difference(ops.run(name, op, h, "small"), fresh[op]) is None, op
        assert ops.first_difference(sample(), ref) is None, op
    h.release_workspaces()
    assert ops.first_difference(sample(), ref) is None
    assert ops.first_difference(ops.run(name, "posterior_gamma", h, "small"), fresh["posterior_gamma"]) is None
