"""GPU: cv_kbest_batch / cv_kbest_batch_device (K-best list Viterbi, exact f64) against the
numpy specification of tests/kbest_ref.py bit for bit, against cv_decode_batch (rank 0), and
against exhaustive enumeration.  The shapes are the kernels' edges (a wave, more than one wave,
every list width KT = 2 / 4 / 8 / 16, 1 / 2 / 4 sequences per workgroup), not the workload."""
import ctypes
import functools

import numpy as np
import pytest

import cviterbi as cv
from conftest import load_golden
from cviterbi import _lib as L
from kbest_ref import brute_force, fold_score, kbest_ref, quantised_model
from test_kbest import check_against_brute_force
from test_posterior import random_model

pytestmark = pytest.mark.gpu

LENGTHS = [33, 1, 2, 5, 0]


def offsets_of(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def ref_batch(pi, a, b, off, obs, K, forced=None):
    """kbest_ref per sequence in cv_kbest_batch's layout: (paths[K, L], scores[B, K], count, status)."""
    B, total = len(off) - 1, int(off[-1])
    paths = np.full((K, total), -1, np.int32)
    scores = np.full((B, K), -np.inf)
    count = np.zeros(B, np.int32)
    status = np.zeros(B, np.uint8)
    for s in range(B):
        lo, hi = int(off[s]), int(off[s + 1])
        p, sc, c = kbest_ref(pi, a, b, obs[lo:hi], K, None if forced is None else forced[lo:hi])
        paths[:, lo:hi], scores[s], count[s] = p, sc, c
        status[s] = L.SEQ_EMPTY if hi == lo else (L.SEQ_OK if c else L.SEQ_INFEASIBLE)
    return paths, scores, count, status


def assert_same(got, ref, what=""):
    for name, x, y in zip(("paths", "scores", "count", "status"), got, ref):
        assert x.shape == y.shape and x.dtype == y.dtype, (what, name, x.shape, y.shape, x.dtype, y.dtype)
        assert np.array_equal(x, y, equal_nan=True), (what, name, np.argwhere(x != y)[:5])


@functools.lru_cache(maxsize=None)
def model(kind, n, v=4):
    if kind == "zeros10":
        return random_model(n, v, seed=3000 + n)
    return quantised_model(n, v, seed=4000 + n)


def case(kind, n, lengths, v=4):
    pi, a, b = model(kind, n, v)
    off = offsets_of(lengths)
    obs = np.random.default_rng(n).integers(0, v, size=int(off[-1])).astype(np.int32)
    return pi, a, b, off, obs


# ---- against the specification, bit for bit ---------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 3, 5, 8, 16])
@pytest.mark.parametrize("N", [1, 2, 3, 17, 63, 64, 65, 130, 256, 257])
@pytest.mark.parametrize("kind", ["zeros10", "ties"])
def test_matches_the_specification(gpu, kind, N, K):
    pi, a, b, off, obs = case(kind, N, LENGTHS)
    ref = ref_batch(pi, a, b, off, obs, K)
    h = cv.HMM(pi, a, b, device=gpu)
    for kernel in ("auto", "generic"):
        got = cv.kbest_batch(h, off, obs, K, kernel=kernel)
        assert_same(got, ref, f"{kind} N={N} K={K} {kernel}")
        t = cv.last_timing(h)
        assert t["kernel"] == "generic" and t["launches"] == 1, t
    assert ref[3][4] == L.SEQ_EMPTY and ref[2][4] == 0


@pytest.mark.parametrize("K", [1, 8])
@pytest.mark.parametrize("kind", ["zeros10", "ties"])
def test_matches_the_specification_at_1024_states(gpu, kind, K):
    pi, a, b, off, obs = case(kind, 1024, [5, 1])
    ref = ref_batch(pi, a, b, off, obs, K)
    h = cv.HMM(pi, a, b, device=gpu)
    for kernel in ("auto", "generic"):
        assert_same(cv.kbest_batch(h, off, obs, K, kernel=kernel), ref, f"{kind} N=1024 K={K} {kernel}")


# ---- 2 and 4 sequences per workgroup (batches from 1,024 / 2,048 sequences on) ------------------------
@pytest.mark.parametrize("K,B,S", [(2, 2050, 4), (2, 1030, 2), (3, 2050, 2), (4, 1030, 2), (8, 1030, 2), (8, 2050, 2),
                                   (16, 2050, 1)])
def test_sequences_per_workgroup(gpu, K, B, S):
    """A workgroup's S sequences have different lengths (ragged, the last workgroup partly empty),
    an empty and an out-of-range one among them; equal to the same sequences in batches small
    enough for one sequence per workgroup, and the first ones to the specification."""
    N, V = 65, 4
    pi, a, b = model("ties", N, V)
    lengths = [(7 * k) % 6 for k in range(B)]
    off = offsets_of(lengths)
    obs = np.random.default_rng(B).integers(0, V, size=int(off[-1])).astype(np.int32)
    obs[off[11] + 1] = V  # sequence 11 (length 5): BADOBS
    h = cv.HMM(pi, a, b, device=gpu)
    got = cv.kbest_batch(h, off, obs, K)
    assert cv.last_timing(h)["seqs_per_wave"] == S
    assert got[3][11] == L.SEQ_BADOBS and got[3][0] == L.SEQ_EMPTY
    for lo in range(0, B, 500):
        hi = min(lo + 500, B)
        e0, e1 = int(off[lo]), int(off[hi])
        part = cv.kbest_batch(h, off[lo:hi + 1] - e0, obs[e0:e1], K)
        assert cv.last_timing(h)["seqs_per_wave"] == 1
        assert_same(part, (got[0][:, e0:e1], got[1][lo:hi], got[2][lo:hi], got[3][lo:hi]), f"batch from {lo}")
    n = 10
    ref = ref_batch(pi, a, b, off[:n + 1], obs[:int(off[n])], K)
    assert_same((got[0][:, :int(off[n])], got[1][:n], got[2][:n], got[3][:n]), ref, "first sequences")


# ---- rank 0 is the decode ---------------------------------------------------------------------------
def assert_rank0_is_decode(h, off, obs, got, forced=None):
    path, score, st = cv.decode_batch(h, off, obs, dtype="f64", forced=forced)
    n_ok = 0
    for s in range(len(off) - 1):
        lo, hi = int(off[s]), int(off[s + 1])
        if st[s] != L.SEQ_OK:
            assert got[3][s] == st[s], (s, got[3][s], st[s])
            continue
        n_ok += 1
        assert got[3][s] == L.SEQ_OK and got[2][s] >= 1, s
        assert np.array_equal(got[0][0, lo:hi], path[lo:hi]), s
        assert got[1][s, 0] == score[s], (s, got[1][s, 0], score[s])
    return n_ok


@pytest.mark.parametrize("name", ["golden_small.npz", "golden_ties.npz", "golden_inf.npz"])
def test_rank0_is_the_decode_on_golden(gpu, name):
    g = load_golden(name)
    h = cv.HMM(g["pi"], g["a"], g["b"], device=gpu)
    ok = g["f64_viterbi_status"].repeat(np.diff(g["offsets"])) == L.SEQ_OK  # per element
    for K in (1, 4):
        got = cv.kbest_batch(h, g["offsets"], g["obs"], K)
        assert assert_rank0_is_decode(h, g["offsets"], g["obs"], got) > 0
        assert np.array_equal(got[0][0][ok], g["f64_viterbi_path"][ok])  # the recorded oracle path too


def test_rank0_is_the_decode_on_a_ragged_forced_batch(gpu):
    N, V = 40, 6
    pi, a, b = random_model(N, V, seed=21)
    rng = np.random.default_rng(21)
    lengths = [1 + (29 * k) % 50 for k in range(37)]
    off = offsets_of(lengths)
    obs = rng.integers(0, V, size=int(off[-1])).astype(np.int32)
    forced = np.where(rng.random(int(off[-1])) < 0.1, rng.integers(0, N, size=int(off[-1])), -1).astype(np.int32)
    h = cv.HMM(pi, a, b, device=gpu)
    for frc in (None, forced):
        got = cv.kbest_batch(h, off, obs, 5, forced=frc)
        assert assert_rank0_is_decode(h, off, obs, got, frc) >= 3


# ---- exhaustive enumeration on the device -----------------------------------------------------------
def test_brute_force_on_the_device(gpu):
    K, V = 8, 3
    rng = np.random.default_rng(5)
    saw_short = saw_infeasible = False
    for N in (1, 2, 3, 4):
        for inf_arcs in (False, True):
            pi, a, b = quantised_model(N, V, seed=50 + N, inf_arcs=inf_arcs)
            b[:, 2] = -np.inf  # observation 2 cannot be emitted: an infeasible sequence
            lengths = [6, 1, 3, 2, 5, 4]
            off = offsets_of(lengths)
            obs = rng.integers(0, 2, size=int(off[-1])).astype(np.int32)
            obs[off[2] + 1] = 2
            h = cv.HMM(pi, a, b, device=gpu)
            paths, scores, count, status = cv.kbest_batch(h, off, obs, K)
            assert status[2] == L.SEQ_INFEASIBLE and count[2] == 0
            assert np.all(scores[2] == -np.inf) and np.all(paths[:, off[2]:off[3]] == -1)
            saw_infeasible = True
            for s in (0, 1, 3, 4, 5):
                lo, hi = int(off[s]), int(off[s + 1])
                check_against_brute_force(pi, a, b, obs[lo:hi], K, (paths[:, lo:hi], scores[s], int(count[s])))
                n_paths = len(brute_force(pi, a, b, obs[lo:hi])[0])
                assert status[s] == (L.SEQ_OK if n_paths else L.SEQ_INFEASIBLE)
                saw_short |= 0 < n_paths < K
            # the C call reports the infeasible sequence after writing every output
            o = L.opts(L.DTYPE_F64)
            p2, s2 = np.zeros_like(paths), np.zeros_like(scores)
            c2, st2 = np.zeros_like(count), np.zeros_like(status)
            rc = L.lib().cv_kbest_batch(h.handle, len(lengths), off.ctypes.data, obs.ctypes.data, K, ctypes.byref(o),
                                        p2.ctypes.data, s2.ctypes.data, c2.ctypes.data, st2.ctypes.data)
            assert rc == L.CV_EINFEASIBLE
            assert_same((p2, s2, c2, st2), (paths, scores, count, status))
    assert saw_short and saw_infeasible


# ---- the K' < K result is a prefix ------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["zeros10", "ties"])
def test_prefix_property(gpu, kind):
    pi, a, b, off, obs = case(kind, 65, LENGTHS)
    h = cv.HMM(pi, a, b, device=gpu)
    p8, s8, c8, st8 = cv.kbest_batch(h, off, obs, 8)
    for K in (3, 5):
        p, s, c, st = cv.kbest_batch(h, off, obs, K)
        assert np.array_equal(p, p8[:K]) and np.array_equal(s, s8[:, :K])
        assert np.array_equal(c, np.minimum(c8, K)) and np.array_equal(st, st8)


# ---- forced tags ------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [3, 65])
def test_forced_tags(gpu, N):
    pi, a, b, off, obs = case("ties", N, [9, 4, 1, 6])
    pi, a, b = pi.copy(), a.copy(), b.copy()
    b[N - 1, :] = -np.inf  # the last state emits nothing: forcing it makes a sequence infeasible
    rng = np.random.default_rng(N)
    forced = np.full(int(off[-1]), -1, np.int32)
    forced[off[0] + 3] = rng.integers(0, N - 1)
    forced[off[0] + 7] = rng.integers(0, N - 1)
    forced[off[1] + 2] = N - 1  # infeasible
    forced[off[2]] = 0
    h = cv.HMM(pi, a, b, device=gpu)
    for K in (2, 8):
        ref = ref_batch(pi, a, b, off, obs, K, forced)
        assert ref[3][1] == L.SEQ_INFEASIBLE and ref[3][0] == L.SEQ_OK and ref[3][3] == L.SEQ_OK
        got = cv.kbest_batch(h, off, obs, K, forced=forced)
        assert_same(got, ref, f"forced N={N} K={K}")
        for r in range(got[2][0]):
            assert got[0][r, off[0] + 3] == forced[off[0] + 3] and got[0][r, off[0] + 7] == forced[off[0] + 7]
    with pytest.raises(cv.CVError) as e:
        cv.kbest_batch(h, off, obs, 2, forced=np.full(int(off[-1]), N, np.int32))
    assert e.value.status == L.CV_EINVAL


# ---- statuses: out-of-range and empty sequences disturb nobody -----------------------------------------
def test_badobs_and_empty_in_the_middle(gpu):
    N, V, K = 17, 4, 4
    pi, a, b = model("ties", N, V)
    good = [np.array([0, 1, 2, 1, 0, 3, 3], np.int32), np.array([2], np.int32), np.array([1, 1, 0, 2, 2], np.int32)]
    seqs = [good[0], np.array([1, 99, 0, -4], np.int32), good[1], np.zeros(0, np.int32), np.array([V], np.int32), good[2]]
    off, goff = offsets_of([len(s) for s in seqs]), offsets_of([len(s) for s in good])
    obs = np.concatenate(seqs)
    h = cv.HMM(pi, a, b, device=gpu)
    for kernel in ("auto", "generic"):
        paths, scores, count, status = cv.kbest_batch(h, off, obs, K, kernel=kernel)
        assert list(status) == [L.SEQ_OK, L.SEQ_BADOBS, L.SEQ_OK, L.SEQ_EMPTY, L.SEQ_BADOBS, L.SEQ_OK]
        for s in (1, 4):
            assert count[s] == 0 and np.all(np.isnan(scores[s])) and np.all(paths[:, off[s]:off[s + 1]] == -1)
        assert count[3] == 0 and np.all(scores[3] == -np.inf)
        p2, s2, c2, st2 = cv.kbest_batch(h, goff, np.concatenate(good), K, kernel=kernel)
        assert np.all(st2 == L.SEQ_OK)
        for k2, s in enumerate((0, 2, 5)):
            assert np.array_equal(scores[s], s2[k2]) and count[s] == c2[k2]
            assert np.array_equal(paths[:, off[s]:off[s + 1]], p2[:, goff[k2]:goff[k2 + 1]])
        assert_same((p2, s2, c2, st2), ref_batch(pi, a, b, goff, np.concatenate(good), K))


# ---- workspace chunks -------------------------------------------------------------------------------
def test_chunked_workspace(gpu):
    N, K, V = 64, 4, 4
    pi, a, b = model("zeros10", N, V)
    lengths = [1 + (23 * k) % 40 for k in range(40)]
    assert max(lengths) == 40 and min(lengths) == 1
    off = offsets_of(lengths)
    obs = np.random.default_rng(7).integers(0, V, size=int(off[-1])).astype(np.int32)
    h = cv.HMM(pi, a, b, device=gpu)
    whole = cv.kbest_batch(h, off, obs, K)
    assert cv.last_timing(h)["launches"] == 1
    need = 40 * N * 4 * 2  # the longest sequence's u16 back-pointers at KT = 4
    chunked = cv.kbest_batch(h, off, obs, K, workspace_bytes=need + 64)
    assert cv.last_timing(h)["launches"] > 1
    assert_same(chunked, whole, "chunked")
    with pytest.raises(cv.CVError) as e:
        cv.kbest_batch(h, off, obs, K, workspace_bytes=need - 2)
    assert e.value.status == L.CV_ENOMEM
    assert_same(cv.kbest_batch(h, off, obs, K), whole, "after the error")


# ---- self-consistency at a larger shape -------------------------------------------------------------
def test_self_consistency_n256_k8(gpu):
    N, K, V, B, T = 256, 8, 8, 64, 64
    pi, a, b = model("zeros10", N, V)
    off = offsets_of([T] * B)
    obs = np.random.default_rng(9).integers(0, V, size=B * T).astype(np.int32)
    h = cv.HMM(pi, a, b, device=gpu)
    got = cv.kbest_batch(h, off, obs, K)
    paths, scores, count, status = got
    assert assert_rank0_is_decode(h, off, obs, got) > B // 2
    for s in range(B):
        lo, hi = s * T, (s + 1) * T
        c = int(count[s])
        assert np.all(np.diff(scores[s, :c]) <= 0) and np.all(scores[s, c:] == -np.inf)
        assert len({tuple(paths[r, lo:hi]) for r in range(c)}) == c
        for r in range(c):
            assert fold_score(pi, a, b, obs[lo:hi], paths[r, lo:hi]) == scores[s, r], (s, r)
    ref = ref_batch(pi, a, b, off[:3], obs[:2 * T], K)
    assert np.array_equal(paths[:, :2 * T], ref[0]) and np.array_equal(scores[:2], ref[1])
    assert np.array_equal(count[:2], ref[2]) and np.array_equal(status[:2], ref[3])


# ---- the device variant, repeats --------------------------------------------------------------------
def test_device_variant_and_repeat_are_bit_identical(gpu):
    import torch

    N, K, V = 65, 5, 4
    pi, a, b = model("ties", N, V)
    lengths = [1 + (37 * k) % 30 for k in range(33)]
    off = offsets_of(lengths)
    obs = np.random.default_rng(3).integers(0, V, size=int(off[-1])).astype(np.int32)
    h = cv.HMM(pi, a, b, device=gpu)
    first = cv.kbest_batch(h, off, obs, K)
    assert_same(cv.kbest_batch(h, off, obs, K), first, "repeat")
    dev = torch.device("cuda", gpu)
    total, B = int(off[-1]), len(lengths)
    d_off, d_obs = torch.from_numpy(off).to(dev), torch.from_numpy(obs).to(dev)
    d_path = torch.zeros(K, total, dtype=torch.int32, device=dev)
    d_score = torch.zeros(B, K, dtype=torch.float64, device=dev)
    d_count = torch.zeros(B, dtype=torch.int32, device=dev)
    d_st = torch.zeros(B, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    for host_off in (off, None):
        cv.kbest_batch_device(h, d_off, d_obs, K, d_path, d_score, d_count, d_st, offsets_host=host_off,
                              stream=stream.cuda_stream)
        stream.synchronize()
        got = (d_path.cpu().numpy(), d_score.cpu().numpy(), d_count.cpu().numpy(), d_st.cpu().numpy())
        assert_same(got, first, "device variant")
        d_path.zero_(), d_score.zero_(), d_count.zero_()
        torch.cuda.synchronize(dev)
    t = cv.last_timing(h)
    assert t["fwd_ms"] > 0 and t["bt_ms"] > 0 and t["launches"] == 1 and t["kernel"] == "generic", t


# ---- limits -----------------------------------------------------------------------------------------
def test_limits(gpu):
    pi, a, b = model("ties", 4, 3)
    h = cv.HMM(pi, a, b, device=gpu)
    off, obs = [0, 3], np.array([0, 1, 2], np.int32)

    def status_of(hh, k=2, **kw):
        with pytest.raises(cv.CVError) as e:
            cv.kbest_batch(hh, off, obs, k, **kw)
        return e.value.status

    assert status_of(h, dtype="f32") == L.CV_EUNSUPPORTED
    assert status_of(h, assoc="cp") == L.CV_EINVAL
    assert status_of(h, kernel="trellis") == L.CV_EINVAL
    assert status_of(h, kernel="trellis_f64") == L.CV_EINVAL
    assert status_of(h, k=0) == L.CV_EINVAL and status_of(h, k=17) == L.CV_EINVAL

    def flat(n):
        return cv.HMM(np.full(n, -np.log10(n)), np.full((n, n), -np.log10(n)), np.zeros((n, 3)), device=gpu)

    assert status_of(flat(1024), k=16) == L.CV_EUNSUPPORTED  # N * KT = 16,384
    assert status_of(flat(1025), k=1) == L.CV_EUNSUPPORTED
    paths, scores, count, status = cv.kbest_batch(h, off, obs, 2)  # the handle still works after the errors
    assert status[0] == L.SEQ_OK and count[0] == 2


# ---- workspace release ------------------------------------------------------------------------------
def test_release_workspaces(gpu):
    N, K, V = 64, 8, 4
    pi, a, b = model("zeros10", N, V)
    off = offsets_of([50] * 20)
    obs = np.random.default_rng(1).integers(0, V, size=1000).astype(np.int32)
    h = cv.HMM(pi, a, b, device=gpu)
    cv.decode_batch(h, off, obs, dtype="f64", kernel="generic")  # the f64 tables are up before the baseline
    h.release_workspaces()
    before = cv.device_memory()["current"]
    cv.kbest_batch(h, off, obs, K)
    during = cv.device_memory()["current"]
    assert during - before >= 1000 * N * K * 2 + 20 * N * K * 8  # back-pointers and last lists
    h.release_workspaces()
    assert cv.device_memory()["current"] == before
