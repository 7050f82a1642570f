"""GPU: the certified fixed-point first pass of the plain f64 batch decode (tuning key
t64_fixed_first, DESIGN.md "Certified fixed-point first pass").

With the key at 1 (every batch of two or more sequences takes the pass) a decode must equal, bit
for bit -- paths, score bits, statuses -- the same decode with the key at 0 (the f64 kernels
alone: the earlier behaviour), and the C oracle where the oracle covers the input.  The counters
(cv_last_fixed_first_stats) say which sequences the integer pass kept, and on equal-length
batches they must be the numpy model's (tools/probe_fixed_first.py), which the kernels follow
step by step.
"""
import importlib.util
import os

import numpy as np
import pytest

import c_oracle as O
import cviterbi as cv
from conftest import load_golden
from cviterbi import _lib as L
from cviterbi import synth

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location(
    "probe_fixed_first", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools",
                                      "probe_fixed_first.py"))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)

N, V = 256, 16


def _same(got, ref, what):
    for x, y, name in zip(got, ref, ("path", "score", "status")):
        x, y = np.asarray(x), np.asarray(y)
        if name == "score":
            x, y = x.view(np.uint64), y.view(np.uint64)
        bad = np.nonzero(x != y)[0]
        assert bad.size == 0, f"{what}: {name} differs at {bad[:8]}"


def _decode_device(h, off, obs):
    """The device entry (observations are range-checked on the device, not by the host)."""
    import torch

    dev = torch.device("cuda", 0)
    off_d, obs_d = torch.from_numpy(np.asarray(off, np.int64)).to(dev), torch.from_numpy(obs).to(dev)
    p_d = torch.full((len(obs),), -9, dtype=torch.int32, device=dev)
    s_d = torch.full((len(off) - 1,), np.nan, dtype=torch.float64, device=dev)
    st_d = torch.full((len(off) - 1,), 77, dtype=torch.uint8, device=dev)
    cv.decode_batch_device(h, off_d, obs_d, p_d, s_d, st_d, offsets_host=np.asarray(off, np.int64), dtype="f64")
    torch.cuda.synchronize(dev)
    return p_d.cpu().numpy(), s_d.cpu().numpy(), st_d.cpu().numpy()


def _on_off(h, off, obs, what, device=False):
    """The decode with the pass and without it; they agree.  Returns (result, the pass's stats)."""
    run = (lambda: _decode_device(h, off, obs)) if device else (
        lambda: cv.decode_batch(h, off, obs, dtype="f64", rescore_f64=False))
    h.set_tuning(t64_fixed_first=1)
    on = run()
    st = cv.last_fixed_first_stats(h)
    assert cv.last_timing(h)["kernel"] == "trellis_f64"
    h.set_tuning(t64_fixed_first=0)
    ref = run()
    st0 = cv.last_fixed_first_stats(h)
    assert st0["engaged"] == 0 and st0["certified"] == 0 and st0["fallback"] == 0, st0
    _same(on, ref, f"{what}: key 1 vs 0")
    return on, st


@pytest.fixture(scope="module")
def model():
    return synth.random_hmm(N, V, seed=11)


@pytest.mark.parametrize("T", [1, 2, 3, 64])
def test_equal_lengths_and_batch_sizes(gpu, model, T):
    """B = 1 (not the pass's), 7 and 9 (an unpaired sequence), 8, 520 (more than one round of
    workgroups on any device is not needed: the grid is one workgroup per pair)."""
    pi, a, b = model
    for B in (1, 7, 8, 9, 520):
        off = np.arange(B + 1, dtype=np.int64) * T
        obs = synth.iid_obs(V, B * T, seed=100 * T + B)
        got, st = _on_off(cv.HMM(pi, a, b), off, obs, f"T={T} B={B}")
        _same(got, O.decode_batch(pi, a, b, off, obs, O.VITERBI, np.float64, nthreads=8), f"T={T} B={B} vs the oracle")
        if B == 1:
            assert st["engaged"] == 0, st
            continue
        _, cert, _ = M.decode(pi, a, b, obs.reshape(B, T).astype(np.int64)[: B - B % 2])
        assert st["engaged"] == 1 and st["certified"] + st["fallback"] == B, st
        assert st["certified"] == int(cert.sum()), (st, int(cert.sum()))
        assert st["fallback"] >= B % 2


def test_ragged_lengths(gpu, model):
    """Lengths 1..40 and an empty sequence, 75 sequences: equal-length neighbours of the
    longest-first order are paired, the others take the f64 kernels."""
    pi, a, b = model
    rng = np.random.default_rng(3)
    lengths = np.concatenate([[0, 1, 1, 2, 2, 3, 40, 40, 40], rng.integers(1, 41, size=66)])
    rng.shuffle(lengths)
    off = synth.offsets_from_lengths(lengths)
    obs = rng.integers(0, V, size=int(off[-1])).astype(np.int32)
    got, st = _on_off(cv.HMM(pi, a, b), off, obs, "ragged")
    _same(got, O.decode_batch(pi, a, b, off, obs, O.VITERBI, np.float64), "ragged vs the oracle")
    assert st["engaged"] == 1 and st["certified"] + st["fallback"] == len(lengths), st
    assert st["certified"] > 0 and st["fallback"] > 0, st


def test_inf_model_infeasible_and_bad_observation(gpu):
    """golden_inf.npz's 20 states inside a 256-state model whose other states are unreachable,
    plus one observation no state emits: the recorded f64 decode; then one sequence made
    infeasible (it ends in that observation) and one given an out-of-range observation, whose
    neighbours stay bit-identical."""
    g = load_golden("golden_inf.npz")
    n, v = g["b"].shape
    pi = np.full(N, -np.inf)
    a = np.full((N, N), -np.inf)
    b = np.full((N, v + 1), -np.inf)
    pi[:n], a[:n, :n], b[:n, :v] = g["pi"], g["a"], g["b"]
    off, obs = g["offsets"], g["obs"].copy()
    ref = (g["f64_viterbi_path"], g["f64_viterbi_score"], g["f64_viterbi_status"])
    got, st = _on_off(cv.HMM(pi, a, b), off, obs, "golden_inf")
    _same(got, ref, "golden_inf vs the recorded decode")
    assert st["engaged"] == 1 and st["certified"] + st["fallback"] == len(off) - 1, st
    long_ok = np.nonzero((ref[2] == L.SEQ_OK) & (np.diff(off) > 4))[0]
    k, m = int(long_ok[0]), int(long_ok[-1])
    obs[off[k] + 2] = v + 1  # out of range
    obs[off[m + 1] - 1] = v  # impossible
    bad, st = _on_off(cv.HMM(pi, a, b), off, obs, "golden_inf, bad observation", device=True)
    assert bad[2][k] == L.SEQ_BADOBS and bad[2][m] == L.SEQ_INFEASIBLE and k != m
    keep = ~np.isin(np.arange(len(off) - 1), [k, m])
    assert np.array_equal(bad[2][keep], ref[2][keep])
    assert np.array_equal(bad[1][keep].view(np.uint64), ref[1][keep].view(np.uint64))
    ek = np.ones(len(obs), bool)
    ek[off[k]:off[k + 1]] = False
    ek[off[m]:off[m + 1]] = False
    assert np.array_equal(bad[0][ek], ref[0][ek])


def test_banded_inf_model_at_256(gpu):
    """-inf transitions, emissions and initial states at N = 256 (banded a, half of b and pi)."""
    pi, a, b = synth.random_hmm(N, 8, seed=13)
    i, j = np.indices((N, N))
    a[(j - i) % N > 3] = -np.inf
    rng = np.random.default_rng(13)
    b[rng.random((N, 8)) < 0.5] = -np.inf
    pi[::2] = -np.inf
    b[:, 7] = -np.inf  # observation 7 is impossible: it ends every sixth sequence
    B, T = 64, 24
    off = np.arange(B + 1, dtype=np.int64) * T
    obs = rng.integers(0, 7, size=B * T).astype(np.int32)
    obs[off[1::6] - 1] = 7
    got, st = _on_off(cv.HMM(pi, a, b), off, obs, "banded -inf")
    ref = O.decode_batch(pi, a, b, off, obs, O.VITERBI, np.float64)
    _same(got, ref, "banded -inf vs the oracle")
    assert (ref[2] == L.SEQ_INFEASIBLE).any() and (ref[2] == L.SEQ_OK).any()
    assert st["certified"] + st["fallback"] == B and st["fallback"] >= int((ref[2] != L.SEQ_OK).sum()), st


def test_identical_states_fall_back_and_pin(gpu, model):
    """States 0 and 1 identical and dominant: an exact tie at every step, so no sequence
    certifies, the results are the f64 kernels', and the handle is pinned to them."""
    pi, a, b = (x.copy() for x in model)
    a[1, :], b[1, :], pi[1] = a[0, :], b[0, :], pi[0]
    a[:, :2] = np.log10(0.45)
    b[:2, :] = np.log10(0.9)
    B, T = 64, 16
    off = np.arange(B + 1, dtype=np.int64) * T
    obs = synth.iid_obs(V, B * T, seed=5)
    h = cv.HMM(pi, a, b)
    got, st = _on_off(h, off, obs, "identical states")
    _same(got, O.decode_batch(pi, a, b, off, obs, O.VITERBI, np.float64), "identical states vs the oracle")
    assert st == dict(engaged=1, certified=0, fallback=B, pinned=1), st
    h.set_tuning(t64_fixed_first=1)
    again = cv.decode_batch(h, off, obs, dtype="f64", rescore_f64=False)
    st2 = cv.last_fixed_first_stats(h)
    assert st2 == dict(engaged=0, certified=0, fallback=0, pinned=1), st2
    _same(again, got, "identical states, after the guard")
    assert h.tuning("t64_fixed_first") == 1  # the key is the caller's; the guard is the handle's


@pytest.mark.parametrize("scale,mixed", [(1e-3, True), (1e-4, False)])
def test_small_margins(gpu, model, scale, mixed):
    """The model scaled down until margins meet the certificate's threshold.  1e-3: a few of 96
    sequences fail, so certified and f64-decoded sequences share the call and each must land in
    its own slot.  1e-4: about half fail, which is above 1 in 8: the guard."""
    pi, a, b = (x * scale for x in model)
    B, T = 96, 48
    off = np.arange(B + 1, dtype=np.int64) * T
    obs = synth.iid_obs(V, B * T, seed=11)
    _, cert, _ = M.decode(pi, a, b, obs.reshape(B, T).astype(np.int64))
    nc = int(cert.sum())
    got, st = _on_off(cv.HMM(pi, a, b), off, obs, f"scale {scale}")
    _same(got, O.decode_batch(pi, a, b, off, obs, O.VITERBI, np.float64), f"scale {scale} vs the oracle")
    if mixed:
        assert 0 < B - nc <= B // 8
        assert st == dict(engaged=1, certified=nc, fallback=B - nc, pinned=0), (st, nc)
    else:
        assert B // 4 < B - nc < 3 * B // 4
        assert st == dict(engaged=1, certified=0, fallback=B, pinned=1), (st, nc)


def test_positive_entry_keeps_the_f64_kernels(gpu, model):
    pi, a, b = (x.copy() for x in model)
    b[3, 2] = 0.25  # a density above 1: not a log-probability model
    B, T = 16, 12
    off = np.arange(B + 1, dtype=np.int64) * T
    obs = synth.iid_obs(V, B * T, seed=2)
    got, st = _on_off(cv.HMM(pi, a, b), off, obs, "positive entry")
    assert st == dict(engaged=0, certified=0, fallback=0, pinned=0), st
    _same(got, O.decode_batch(pi, a, b, off, obs, O.VITERBI, np.float64), "positive entry vs the oracle")


def test_counters_are_consistent_and_length_checked(gpu, model):
    """certified + fallback = B, and the stats call is length-checked."""
    import ctypes

    pi, a, b = model
    B, T = 130, 20
    off = np.arange(B + 1, dtype=np.int64) * T
    obs = synth.iid_obs(V, B * T, seed=9)
    h = cv.HMM(pi, a, b)
    got, st = _on_off(h, off, obs, "counters")
    assert st["engaged"] == 1 and st["certified"] + st["fallback"] == B and st["pinned"] == 0, st
    out = (ctypes.c_int64 * 6)(*([-7] * 6))
    assert L.lib().cv_last_fixed_first_stats(h.handle, out, 2) == 4 and list(out[2:]) == [-7] * 4
    assert L.lib().cv_last_fixed_first_stats(h.handle, out, 6) == 4 and list(out[4:]) == [-7] * 2
    assert L.lib().cv_last_fixed_first_stats(h.handle, None, 0) == 4
