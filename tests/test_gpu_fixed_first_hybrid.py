"""The integer forward of the certified fixed-point first pass (trellis_fwd2_i32, DESIGN.md "The
integer mix's issue roof") on the shapes and table entries at which its inner loop can go wrong.

The hybrid the file is named after -- integer sums, the maximum taken with v_max3_f32 on biased bit
patterns -- was measured and not built (it does not co-issue: profiles/i32_mix_rates.txt), so no
bias and no second floor exist and the CPU check of their bounds has nothing to check.  What was
built is the order of the loop's instructions (each 8-row block: 16 sums, then 8 maxima, each
maximum taking one sum of either half of the block).  These tests hold whatever the loop's order:

  * with the pass on (t64_fixed_first=1) paths, score bits and statuses equal the same handle's
    decode with the pass off, and
  * the number of sequences the pass certified is the numpy model's (tools/probe_fixed_first.py),
    counted over the sequences the host pairs: equal-length neighbours of the longest-first order.
"""
import importlib.util
import os

import numpy as np
import pytest

import cviterbi as cv
from cviterbi import synth

_spec = importlib.util.spec_from_file_location(
    "probe_fixed_first", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools",
                                      "probe_fixed_first.py"))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)

V = 12
# table entries on both sides of the pass's floor (-16 decades) and of the floor the hybrid would
# have needed (-15.75), beside ordinary ones
EDGE = np.array([-np.inf, -15.7, -15.8, -15.99, -16.5, -40.0])
FLOORS_SEED = 0  # of floors_model: chosen with the numpy model, which certifies 14 of its 16 sequences


def _same(got, ref, what):
    for x, y, name in zip(got, ref, ("path", "score", "status")):
        x, y = np.asarray(x), np.asarray(y)
        if name == "score":
            x, y = x.view(np.uint64), y.view(np.uint64)
        bad = np.nonzero(x != y)[0]
        assert bad.size == 0, f"{what}: {name} differs at {bad[:8]}"


def model_certified(pi, a, b, off, obs):
    """The model's count over the sequences the host pairs: per length, in index order, all but
    the odd one out."""
    lengths = np.diff(off)
    n = 0
    for length in np.unique(lengths[lengths > 0]):
        idx = np.nonzero(lengths == length)[0]
        idx = idx[: len(idx) - len(idx) % 2]
        if len(idx) == 0:
            continue
        o = np.stack([obs[off[i]:off[i + 1]] for i in idx]).astype(np.int64)
        n += int(M.decode(pi, a, b, o)[1].sum())
    return n


def on_off_and_count(pi, a, b, off, obs, what):
    """Both assertions; returns the pass's stats and the model's count."""
    h = cv.HMM(pi, a, b)
    h.set_tuning(t64_fixed_first=1)
    on = cv.decode_batch(h, off, obs, dtype="f64", rescore_f64=False)
    st = cv.last_fixed_first_stats(h)
    h.set_tuning(t64_fixed_first=0)
    ref = cv.decode_batch(h, off, obs, dtype="f64", rescore_f64=False)
    assert cv.last_fixed_first_stats(h)["engaged"] == 0
    _same(on, ref, f"{what}: key 1 vs 0")
    want = model_certified(pi, a, b, off, obs)
    print(f"{what}: stats {st}, model certifies {want}")
    assert st["certified"] == want, (what, st, want)
    return st, want


def ragged_lengths(B, T, rng):
    """B = 2: one pair of length T.  Otherwise lengths from {T, T - 1, T // 2} (those >= 1), so
    several lengths pair and some leave an odd sequence out."""
    if B == 2:
        return np.array([T, T])
    pool = sorted({x for x in (T, T - 1, T // 2) if x >= 1})
    lengths = rng.choice(pool, size=B)
    lengths[:2] = T
    return lengths


def floors_model(seed, n=256):
    """The ordinary entries scaled down until some margins meet the certificate's threshold (as in
    test_gpu_fixed_first.py's small margins), three in ten entries replaced by the edge values."""
    pi, a, b = (x * 1e-3 for x in synth.random_hmm(n, V, seed=seed))
    rng = np.random.default_rng(seed)
    for m in (pi, a, b):
        hit = rng.random(m.shape) < 0.3
        m[hit] = rng.choice(EDGE, size=int(hit.sum()))
    return pi, a, b


def floors_batch(seed, B=16, T=48):
    off = np.arange(B + 1, dtype=np.int64) * T
    return off, synth.iid_obs(V, B * T, seed=seed + 1000)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 2, 3, 64])
@pytest.mark.parametrize("n", [256, 225])
def test_random_models(gpu, n, T):
    """N = 256 and N = 225 (padded to 256 states), B = 2, 6 and 64, ragged lengths."""
    pi, a, b = synth.random_hmm(n, V, seed=17 + n)
    rng = np.random.default_rng(1000 * n + T)
    total = 0
    for B in (2, 6, 64):
        lengths = ragged_lengths(B, T, rng)
        off = synth.offsets_from_lengths(lengths)
        obs = rng.integers(0, V, size=int(off[-1])).astype(np.int32)
        st, want = on_off_and_count(pi, a, b, off, obs, f"N={n} T={T} B={B}")
        assert st["engaged"] == 1, st
        total += want
    assert total > 0  # the pass kept something: the model and the kernel did not agree on nothing


@pytest.mark.gpu
def test_entries_around_both_floors(gpu):
    """-inf, -15.7, -15.8, -15.99, -16.5 and -40 in three of ten entries of pi, A and B."""
    pi, a, b = floors_model(FLOORS_SEED)
    off, obs = floors_batch(FLOORS_SEED)
    st, want = on_off_and_count(pi, a, b, off, obs, "both floors")
    assert 0 < want < len(off) - 1, want
    assert st["engaged"] == 1 and st["pinned"] == 0 and st["fallback"] == len(off) - 1 - want, st


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["zeros", "floored", "one_column"])
def test_extremes(gpu, kind):
    """Every finite entry 0 (every sum at the top of the range, all ties); every entry at or below
    the floor (every sum at the bottom); one column at 0 and the rest at the floor (both ends in
    every maximum)."""
    n, B, T = 256, 4, 8
    rng = np.random.default_rng(5)
    low = np.array([-16.0, -16.5, -40.0, -np.inf])
    if kind == "zeros":
        pi, a, b = np.zeros(n), np.zeros((n, n)), np.zeros((n, V))
    else:
        pi, a, b = (rng.choice(low[:3] if kind == "one_column" else low, size=s) for s in ((n,), (n, n), (n, V)))
        if kind == "one_column":
            pi[7], a[:, 7], b[7, :] = 0.0, 0.0, 0.0
    off = np.arange(B + 1, dtype=np.int64) * T
    obs = rng.integers(0, V, size=B * T).astype(np.int32)
    st, want = on_off_and_count(pi, a, b, off, obs, kind)
    assert want == (B if kind == "one_column" else 0), want


@pytest.mark.gpu
def test_sliding_floor(gpu):
    """T = 2,048 with rows spread over 12 decades: an entry floored in one row re-enters the next
    row's window as F - mu, for two thousand rows."""
    n, B, T = 256, 4, 2048
    rng = np.random.default_rng(23)
    pi, a, b = (-rng.uniform(0.0, 12.0, size=s) for s in ((n,), (n, n), (n, V)))
    off = np.arange(B + 1, dtype=np.int64) * T
    obs = rng.integers(0, V, size=B * T).astype(np.int32)
    st, want = on_off_and_count(pi, a, b, off, obs, "sliding floor")
    assert st["engaged"] == 1 and want > 0, (st, want)
