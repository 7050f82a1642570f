"""CPU: a numpy model of the f64 trellis's sparse low-word planes (tuning key t64_lo_every).

The forward pass (trellis64.hip) stores every delta row as two planes of 32-bit words.  The
HIGH plane (the f64 truncated to a 20-bit mantissa) is written at every row; the LOW plane only
at rows r with r % K == 0 and at the last row ("full" rows).  The backtrack decides most steps
from the high plane alone (the NONPOS threshold test of bt_chain_f64); at a near tie it needs
the exact delta_{t-1}[i] of the few surviving candidates i, and where row t-1 is not a full
row the sparse resolver recomputes them:

  descend  for each needed (row r, state i) the same threshold scan runs over the high plane of
           row r-1 against the column a[:, i]; its survivors are the only states that can
           attain delta_r[i]'s maximum, so they become the need-set of row r-1 (a union over
           i, at most CAP = 8 states per row), down to the nearest full row c <= t-1;
  ascend   exact(c, k) is read from both planes; exact(r, i) = max_k (exact(r-1, k) + a[k, i])
           + b[i, o_r] over the need-set of row r-1 -- the forward pass's own association and
           f64 adds, and a maximum is order-free, so the value is the forward's bit for bit
           (self-check: its high word equals the stored one);
  choose   the first index among the step's survivors with the largest exact sum.

A need-set above the cap replays the rows c+1 .. t-1 densely (the plain forward recurrence
from the full row c), which is exact by construction.

The model below follows the kernel step by step -- same truncation, same f32 estimates and
threshold, same descend / ascend and cap, touching low words of full rows only -- and must
return the numpy oracle's paths and scores on every model class the GPU tests use.
"""
import numpy as np
import pytest

import np_oracle as NO

CAP = 8
F32 = np.float32


def _hi(x):
    """The f64 values whose low 32 bits are cleared: what the high plane alone holds."""
    return (np.asarray(x, np.float64).view(np.uint64) & np.uint64(0xFFFFFFFF00000000)).view(np.float64)


def _scan(hi_row, a32_col):
    """NONPOS threshold test: indices that can attain the exact maximum of delta + a[:, j]."""
    with np.errstate(over="ignore", invalid="ignore"):
        x = hi_row.astype(F32) + a32_col
        m = x.max()
        thr = F32(m * F32(1.0 + 3 * 2.0 ** -20)) - F32(2.0 ** -100)
    return np.nonzero(x >= thr)[0]


def sparse_backtrack(pi, a, b, obs, K, stats):
    """One feasible sequence: forward in f64, backtrack from the planes the kernel keeps."""
    T, n = len(obs), len(pi)
    delta = np.empty((T, n))
    delta[0] = pi + b[:, obs[0]]
    for t in range(1, T):
        delta[t] = (delta[t - 1][:, None] + a).max(axis=0) + b[:, obs[t]]
    hi = _hi(delta)
    full = np.array([r % K == 0 or r == T - 1 for r in range(T)])

    def exact_row(r):  # both planes: only a full row has them
        assert full[r], "the model read a low plane the forward pass never wrote"
        return delta[r]

    a32 = a.astype(F32)
    path = np.zeros(T, np.int32)
    cur = int(np.argmax(exact_row(T - 1)))
    score = exact_row(T - 1)[cur]
    path[T - 1] = cur
    for t in range(T - 1, 0, -1):
        surv = _scan(hi[t - 1], a32[:, cur])
        if len(surv) == 1:
            cur = int(surv[0])
        elif full[t - 1]:  # a near tie at a full row: both planes are there (not counted as an event)
            cur =int(np.argmax(exact_row(t - 1) + a[:, cur]))
        else:
            stats["events"] += 1
            c = (t - 1) - (t - 1) % K
            need = [surv]
            ok = len(surv) <= CAP
            stats["maxneed"] = max(stats["maxneed"], len(surv))
            r = t - 1
            while ok and r > c:  # descend
                nxt = set()
                for i in need[-1]:
                    stats["scans"] += 1
                    nxt.update(int(k) for k in _scan(hi[r - 1], a32[:, i]))
                stats["levels"] += 1
                stats["maxneed"] = max(stats["maxneed"], len(nxt))
                ok = len(nxt) <= CAP
                need.append(np.array(sorted(nxt)))
                r -= 1
            if ok:  # ascend from the full row c
                ex = exact_row(c)[need[-1]]
                for d in range(len(need) - 2, -1, -1):
                    r = t - 1 - d
                    ex = (ex[:, None] + a[np.ix_(need[d + 1], need[d])]).max(axis=0) + b[need[d], obs[r]]
                    assert np.array_equal(_hi(ex), hi[r][need[d]]), "self-check: high words differ"
                    assert np.array_equal(ex, delta[r][need[d]])
                cur = int(need[0][np.argmax(ex + a[need[0], cur])])
            else:  # dense replay of rows c+1 .. t-1
                stats["overflows"] += 1
                d = exact_row(c).copy()
                for r in range(c + 1, t):
                    d = (d[:, None] + a).max(axis=0) + b[:, obs[r]]
                cur = int(np.argmax(d + a[:, cur]))
        path[t - 1] = cur
    return path, score


def _decode(pi, a, b, off, obs, K):
    stats = dict(events=0, scans=0, levels=0, overflows=0, maxneed=0)
    ref = NO.decode_batch(pi, a, b, off, obs, NO.VITERBI, np.float64)
    with np.errstate(invalid="ignore"):
        for s in range(len(off) - 1):
            o = obs[off[s]:off[s + 1]]
            if ref[2][s] != 0:
                continue  # empty / infeasible: the backtrack writes zeros, no chain
            p, sc = sparse_backtrack(pi, a, b, o, K, stats)
            assert np.array_equal(p, ref[0][off[s]:off[s + 1]]), (s, K)
            assert sc == ref[1][s]
    return stats


def _batch(rng, v, K, nseq=10):
    lengths = np.concatenate([[1, 2, K, K + 1, 2 * K + 1, 40], rng.integers(1, 41, size=nseq)])
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return off, rng.integers(0, v, size=int(off[-1])).astype(np.int32)


def _dirichlet(rng, n, v):
    return (np.log10(rng.dirichlet(np.ones(n))), np.log10(rng.dirichlet(np.ones(n), size=n)),
            np.log10(rng.dirichlet(np.ones(v), size=n)))


def _near_ties(rng, n, v):
    q = lambda shape: np.round(rng.uniform(-2, 0, shape) * 4) / 4  # noqa: E731
    return q(n), q((n, n)) - rng.uniform(0, 1e-12, (n, n)), q((n, v)) - rng.uniform(0, 1e-12, (n, v))


def _dyadic(rng, n, v):
    q = lambda shape: -rng.integers(0, 3, size=shape) / 4.0  # noqa: E731
    return q(n), q((n, n)), q((n, v))


@pytest.mark.parametrize("K", [2, 8, 16])
def test_dirichlet_models_have_few_events(K):
    rng = np.random.default_rng(40 + K)
    pi, a, b = _dirichlet(rng, 24, 9)
    off, obs = _batch(rng, 9, K)
    st = _decode(pi, a, b, off, obs, K)
    assert st["events"] * 20 <= int(off[-1]) and st["overflows"] == 0, st


@pytest.mark.parametrize("K", [2, 8, 16])
def test_near_tie_models_descend(K):
    rng = np.random.default_rng(50 + K)
    pi, a, b = _near_ties(rng, 24, 7)
    off, obs = _batch(rng, 7, K)
    st = _decode(pi, a, b, off, obs, K)
    assert st["events"] > 0 and st["levels"] > 0 and st["scans"] >= st["levels"], st
    assert st["maxneed"] <= CAP or st["overflows"] > 0


@pytest.mark.parametrize("K", [2, 8])
def test_dyadic_models_overflow_into_the_dense_replay(K):
    """Exact ties: every state that attains a maximum survives every scan, the need-sets grow
    past the cap and the dense replay decides."""
    rng = np.random.default_rng(60 + K)
    pi, a, b = _dyadic(rng, 40, 5)
    off, obs = _batch(rng, 5, K)
    st = _decode(pi, a, b, off, obs, K)
    assert st["overflows"] > 0, st


def test_infinite_entries_and_infeasible_sequences():
    rng = np.random.default_rng(13)
    n, v = 20, 8
    pi, a, b = _dirichlet(rng, n, v)
    i, j = np.indices((n, n))
    a[(j - i) % n > 3] = -np.inf
    b[rng.random((n, v)) < 0.5] = -np.inf
    pi[::2] = -np.inf
    off, obs = _batch(rng, v, 8, nseq=20)
    ref = NO.decode_batch(pi, a, b, off, obs, NO.VITERBI, np.float64)
    assert (ref[2] == 1).any() and (ref[2] == 0).any()
    _decode(pi, a, b, off, obs, 8)
    _decode(pi, a, b, off, obs, 2)
