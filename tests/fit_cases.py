"""Shared pieces of the fitting tests (tests/test_fit.py, tests/test_gpu_fit_sparse.py,
tests/test_gpu_fit_chunks.py, tests/golden/make_fit_golden.py): the comparison of two
(pi, a, b) triples, the sparse model / corpus families S1-S4, a corpus of thousands of short
sequences, and cv_hmm_fit_train's host-side splitting rules restated (chunks, pairs per wave).

  S1  fallback-heavy: banded A, half of B zero, every other pi zero, random observations
      and 30% random tags -- alpha, beta, gamma and xi all hit normalize()'s zero-sum
      branch (hmm.rs:279, 311) many times per iteration.
  S2  zeros preserved: the same A and pi, B strictly positive, the corpus sampled from the
      model and tagged with 30% of the sampled path -- no fallback can fire (the sampled
      state is in the support of every alpha_t and beta_t), the zeros of A and pi stay.
  S3  dead state: dense, but state N-1 has pi = 0 and a zero column of A, no tags -- no
      gamma ever visits it, so a_den = b_den = 0 there: NaN rows of A and B.
  S4  S2's model with a 1e-306 and a subnormal arc that tagged runs force through: the
      E-step on A 2^K beside exact zeros.
"""
import functools

import numpy as np

import fit_oracle as FO


def assert_params_match(got, ref, atol, rtol=0.0):
    """(pi, a, b) against the reference's: NaN, +inf and -inf at the same positions, every
    other entry within atol / rtol."""
    for g, r, what in zip(got, ref, ("pi", "a", "b")):
        g = np.asarray(g)
        r = np.asarray(r)
        assert g.shape == r.shape, what
        for name, f in (("nan", np.isnan), ("+inf", np.isposinf), ("-inf", np.isneginf)):
            gm, rm = f(g), f(r)
            assert np.array_equal(gm, rm), (f"{what}: {name} at {np.argwhere(gm != rm)[:8].tolist()} "
                                            f"(got {int(gm.sum())}, reference {int(rm.sum())})")
        fin = np.isfinite(r)
        np.testing.assert_allclose(g[fin], r[fin], rtol=rtol, atol=atol, err_msg=what)


def ragged_offsets(rng, nseq, tmax):
    """Lengths in 1..tmax with T = 1, T = 2 and T = tmax among them; sequence 2 has >= 3."""
    lengths = rng.integers(1, tmax + 1, size=nseq)
    lengths[0], lengths[1], lengths[2], lengths[-1] = 1, 2, max(3, tmax // 2), tmax
    off = np.zeros(nseq + 1, np.int64)
    np.cumsum(lengths, out=off[1:])
    return off


def banded_a(rng, n):
    """Arc i -> j kept when (j - i) mod n <= 3 (dense below n = 5), rows normalised."""
    a = rng.random((n, n))
    i, j = np.indices((n, n))
    a[(j - i) % n > 3] = 0.0
    return a / a.sum(axis=1, keepdims=True)


def sparse_pi(rng, n):
    pi = rng.random(n)
    pi[::2] = 0.0
    return pi / pi.sum()


def s1(n, v, nseq, tmax, seed):
    """-> (pi, a, b, offsets, obs, tags)"""
    rng = np.random.default_rng(seed)
    a = banded_a(rng, n)
    b = rng.random((n, v))
    b[rng.random((n, v)) < 0.5] = 0.0
    b[:, 0] += 0.1
    b /= b.sum(axis=1, keepdims=True)
    pi = sparse_pi(rng, n)
    off = ragged_offsets(rng, nseq, tmax)
    total = int(off[-1])
    obs = rng.integers(0, v, size=total).astype(np.int32)
    tags = rng.integers(0, n, size=total).astype(np.int32)
    tags = np.where(rng.random(total) < 0.3, tags, -1).astype(np.int32)
    return pi, a, b, off, obs, tags


def _sample(rng, pi, a, b, off):
    total = int(off[-1])
    n, v = b.shape
    path = np.zeros(total, np.int32)
    obs = np.zeros(total, np.int32)
    for s in range(len(off) - 1):
        for e in range(int(off[s]), int(off[s + 1])):
            path[e] = rng.choice(n, p=pi if e == off[s] else a[path[e - 1]])
            obs[e] = rng.choice(v, p=b[path[e]])
    return path, obs


def s2(n, v, nseq, tmax, seed):
    """-> (pi, a, b, offsets, obs, tags).  Sequences 0 (T = 1) and 2 (T >= 3) stay untagged:
    their alpha and beta have full support (pi's at t = 0), so every state and every arc of
    the band gets a positive count and the -inf of the result are the zeros of the start."""
    rng = np.random.default_rng(seed)
    a = banded_a(rng, n)
    b = rng.random((n, v)) + 0.05
    b /= b.sum(axis=1, keepdims=True)
    pi = sparse_pi(rng, n)
    off = ragged_offsets(rng, nseq, tmax)
    path, obs = _sample(rng, pi, a, b, off)
    tags = np.where(rng.random(len(path)) < 0.3, path, -1).astype(np.int32)
    tags[off[0]:off[1]] = -1
    tags[off[2]:off[3]] = -1
    return pi, a, b, off, obs, tags


def s3(n, v, nseq, tmax, seed):
    """-> (pi, a, b, offsets, obs, tags): state n-1 unreachable, no tags."""
    rng = np.random.default_rng(seed)
    a = rng.random((n, n))
    a[:, n - 1] = 0.0
    a /= a.sum(axis=1, keepdims=True)
    b = rng.random((n, v))
    b /= b.sum(axis=1, keepdims=True)
    pi = rng.random(n)
    pi[n - 1] = 0.0
    pi /= pi.sum()
    off = ragged_offsets(rng, nseq, tmax)
    obs = rng.integers(0, v, size=int(off[-1])).astype(np.int32)
    tags = np.full(int(off[-1]), -1, np.int32)
    return pi, a, b, off, obs, tags


S4_ARCS = ((1, 3), (5, 7))  # both inside the band


def s4(n, v, nseq, tmax, seed):
    """-> (pi, a, b, offsets, obs, tags): S2 with a[1, 3] = 1e-306 and a[5, 7] = 5e-320 (rows
    renormalised: still ~1e-306 and subnormal), followed by fully tagged sequences through
    each tiny arc p -> q: (p, q) and (p, q, q + 1), every step an arc of the band, so no xi
    is uniform and the zeros of A must survive the E-step on A 2^K."""
    pi, a, b, off, obs, tags = s2(n, v, nseq, tmax, seed)
    rng = np.random.default_rng(seed + 1)
    (p, q), (p2, q2) = S4_ARCS
    a = a.copy()
    a[p, q] = 1e-306
    a[p2, q2] = 5e-320
    a /= a.sum(axis=1, keepdims=True)
    forced = []
    for arc in S4_ARCS:
        forced += [np.array(arc)] * 8 + [np.array([arc[0], arc[1], arc[1] + 1])] * 4
    lengths = np.concatenate([np.diff(off), [len(x) for x in forced]])
    off2 = np.zeros(len(lengths) + 1, np.int64)
    np.cumsum(lengths, out=off2[1:])
    ftags = np.concatenate(forced).astype(np.int32)
    fobs = rng.integers(0, v, size=len(ftags)).astype(np.int32)
    return pi, a, b, off2, np.concatenate([obs, fobs]), np.concatenate([tags, ftags])


def dense(n, v, nseq, tmax, seed):
    """-> (pi, a, b, offsets, obs, tags): strictly positive parameters, 30% random tags."""
    rng = np.random.default_rng(seed)
    a = rng.random((n, n))
    a /= a.sum(axis=1, keepdims=True)
    b = rng.random((n, v))
    b /= b.sum(axis=1, keepdims=True)
    pi = rng.random(n)
    pi /= pi.sum()
    off = ragged_offsets(rng, nseq, tmax)
    total = int(off[-1])
    obs = rng.integers(0, v, size=total).astype(np.int32)
    tags = rng.integers(0, n, size=total).astype(np.int32)
    tags = np.where(rng.random(total) < 0.3, tags, -1).astype(np.int32)
    return pi, a, b, off, obs, tags


def short(n, v, nseq, tmax, seed):
    """-> (pi, a, b, offsets, obs, tags): strictly positive parameters, lengths uniform in
    1..tmax, 20% random tags -- thousands of sequences in a few elements each (more pairs of
    sequences than a device has backward waves)."""
    rng = np.random.default_rng(seed)
    a = rng.random((n, n))
    a /= a.sum(axis=1, keepdims=True)
    b = rng.random((n, v))
    b /= b.sum(axis=1, keepdims=True)
    pi = rng.random(n)
    pi /= pi.sum()
    off = np.zeros(nseq + 1, np.int64)
    np.cumsum(rng.integers(1, tmax + 1, size=nseq), out=off[1:])
    total = int(off[-1])
    obs = rng.integers(0, v, size=total).astype(np.int32)
    tags = rng.integers(0, n, size=total).astype(np.int32)
    tags = np.where(rng.random(total) < 0.2, tags, -1).astype(np.int32)
    return pi, a, b, off, obs, tags


FAMILIES = {"s1": s1, "s2": s2, "s3": s3, "s4": s4, "dense": dense, "short": short}


# ---- the host's splitting rules (cv_hmm_fit_train), restated for the tests that hook them -------
def greedy_chunks(off, cap):
    """The chunks [s0, s1) of sequences cv_hmm_fit_train forms under a cap of `cap` elements:
    greedily as many whole sequences as fit; a sequence longer than the cap is a chunk of its own."""
    off = np.asarray(off, np.int64)
    nseq = len(off) - 1
    chunks = []
    s0 = 0
    while s0 < nseq:
        s1 = s0 + 1
        while s1 < nseq and off[s1 + 1] - off[s0] <= cap:
            s1 += 1
        chunks.append((s0, s1))
        s0 = s1
    return chunks


def chunk_stats(off, cap):
    """-> (chunks, max_chunk_elems, most sequences in a chunk) of greedy_chunks."""
    ch = greedy_chunks(off, cap)
    return len(ch), max(int(off[s1] - off[s0]) for s0, s1 in ch), max(s1 - s0 for s0, s1 in ch)


def pair_steps(off):
    """L - 1 of every pair of sequences the N <= 64 backward kernel walks side by side: the
    sequences longest first (stable), two at a time, L the longer of the two (an odd count
    leaves the last one alone).  The kernel stages two steps per matrix-core update, so a pair
    with L - 1 odd ends in a flush of a half-filled stage."""
    lengths = np.diff(np.asarray(off, np.int64))
    srt = lengths[np.argsort(-lengths, kind="stable")]
    return [int(srt[k]) - 1 for k in range(0, len(srt), 2)]


def flush_then_full_stage(off, nwaves):
    """Whether some wave of `nwaves` (wave w walks pairs w, w + nwaves, ...) meets a pair with
    L - 1 odd and right after it a pair with L - 1 even and at least 2: the flush arm between
    two pairs of one wave, then a full stage that a leftover row would corrupt."""
    st = pair_steps(off)
    return any(st[p] % 2 == 1 and st[p + nwaves] % 2 == 0 and st[p + nwaves] >= 2
               for p in range(len(st) - nwaves))


@functools.lru_cache(maxsize=None)
def case(family, n, v, nseq, tmax, iters):
    """One corpus with everything the tests need of the oracle, computed once per session and
    shared (treat as read-only): inputs, fallback_counts of the first iteration, and the
    oracle's log-mapped result after `iters` iterations."""
    inputs = FAMILIES[family](n, v, nseq, tmax, seed=9000 + n)
    counts = FO.fallback_counts(*inputs)
    ref = FO.train(*inputs, iters, 0.0)[:3]
    for x in inputs + ref:
        x.setflags(write=False)
    return inputs, counts, ref
