"""Probe (CPU, numpy): certified 32-bit fixed-point first pass for the exact f64 decode.

A numpy int64 model of the integer recurrence of DESIGN.md "Certified fixed-point first pass"
(every intermediate is asserted to fit int32), its backtrack with certificate, and the gate-1
measurement: on config 4's first B sequences, the share that certifies, and that every
certified path is the f64 decode's own path.

Model (q = 2^QLOG2 log10 units, floor F; every table entry is <= 0 or -inf):
  tables   x~ = max(rint(x / q), F), -inf -> F            (|x~ q - x| <= q/2 wherever x~ > F)
  row 0    v_0[j] = max(pi~[j] + b~[j,o_0], F)
  row t    m = max_i (v_{t-1}[i] + a~[i,j]);  x = max(m, F) + b~[j,o_t]
           v_t[j] = max(x - mu_{t-1}, F),  mu_{t-1} = max_j v_{t-1}[j]   (the PREVIOUS row's
           maximum: the kernel has it one barrier earlier than the current row's, and any
           shift that is uniform over the row leaves every comparison unchanged)
  end      j* = first argmax of v_{T-1}; certified if v[j*] > F and v[j*] - second >= 2T + 1 + x_T
  step t   w = first argmax_i s_i, s_i = v_{t-1}[i] + a~[i,cur]; certified if s_w > F and
           s_w - max_{i != w} s_i >= thr_t = 2t + 2 + floor(g (t+1)^2)
  tables   every pi / b entry on the path has x~ > F (the kernel checks this in the f64 re-score,
           which loads those entries anyway; a~ > F on the path follows from s_w > F)
with g = 1.01 * 2.02 * 2^-53 / q * (max|pi| + max|a| + max|b|) over the finite entries: the f64
recurrence's own rounding, which the threshold has to cover besides the quantisation.

Usage: python tools/probe_fixed_first.py [B] [chunk] [qlog2]
"""
import sys
import time

import numpy as np

QLOG2 = -26
FLOOR = -(1 << 30)
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


def quantise(x, qlog2=QLOG2, floor=FLOOR):
    """int64 array: max(rint(x / q), F); -inf -> F.  x / q is exact (q is a power of two)."""
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        r = np.rint(np.ldexp(x, -qlog2))
    r = np.where(np.isfinite(r) & (r > floor), r, float(floor))
    return r.astype(np.int64)


def rounding_gain(pi, a, b, qlog2=QLOG2):
    """g of the docstring; inf if the tables hold no finite entry."""
    w = 0.0
    for m in (pi, a, b):
        m = np.asarray(m, np.float64)
        f = np.isfinite(m)
        w += float(np.abs(m[f]).max()) if f.any() else 0.0
    return 1.01 * 2.02 * 2.0 ** -53 * 2.0 ** -qlog2 * w


def thresholds(T, g):
    """thr[t] for t = 1..T-1 (thr[0] unused) and the terminal threshold."""
    t = np.arange(T, dtype=np.float64)
    extra = np.minimum(np.floor(g * (t + 1.0) ** 2), float(1 << 29)).astype(np.int64)
    thr = 2 * np.arange(T, dtype=np.int64) + 2 + extra
    end = 2 * T + 1 + int(min(np.floor(g * (T + 1.0) ** 2), float(1 << 29)))
    return thr, end


def _chk32(x):
    assert x.min() >= I32_MIN and x.max() <= I32_MAX, "int32 overflow in the fixed-point recurrence"
    return x


def forward(pq, aq, bq, obs, floor=FLOOR):
    """obs [S, T] (all in range); returns rows [T, S, N] int64, every value in [F, 0]."""
    S, T = obs.shape
    N = aq.shape[0]
    rows = np.empty((T, S, N), np.int64)
    v = np.maximum(_chk32(pq[None, :] + bq[:, obs[:, 0]].T), floor)
    rows[0] = v
    for t in range(1, T):
        mu = v.max(axis=1)
        m = _chk32(v[:, :, None] + aq[None, :, :]).max(axis=1)
        x = _chk32(np.maximum(m, floor) + bq[:, obs[:, t]].T)
        v = np.maximum(_chk32(x - mu[:, None]), floor)
        assert v.max() <= 0
        rows[t] = v
    return rows


def _top2(x):
    """first argmax, its value, and the largest value among the other indices; x [S, N]."""
    S = x.shape[0]
    w = x.argmax(axis=1)
    v1 = x[np.arange(S), w]
    y = x.copy()
    y[np.arange(S), w] = I32_MIN
    return w, v1, y.max(axis=1)


def backtrack(rows, pq, aq, bq, obs, g, floor=FLOOR):
    """returns path [S, T] and cert [S] (bool)."""
    T, S, N = rows.shape
    thr, end = thresholds(T, g)
    path = np.empty((S, T), np.int64)
    cur, v1, v2 = _top2(rows[T - 1])
    cert = (v1 > floor) & (v2 <= v1 - end)
    path[:, T - 1] = cur
    ar = np.arange(S)
    for t in range(T - 1, 0, -1):
        cert &= bq[cur, obs[:, t]] > floor
        s = _chk32(rows[t - 1] + aq[:, cur].T)
        w, v1, v2 = _top2(s)
        cert &= (v1 > floor) & (v2 <= v1 - thr[t])
        path[:, t - 1] = w
        cur = w
    cert &= (bq[cur, obs[:, 0]] > floor) & (pq[cur] > floor)
    return path, cert


def decode(pi, a, b, obs, qlog2=QLOG2, floor=FLOOR):
    """The whole first pass for sequences of one length: path [S, T], cert [S], rows."""
    pq, aq, bq = (quantise(m, qlog2, floor) for m in (pi, a, b))
    rows = forward(pq, aq, bq, obs, floor)
    path, cert = backtrack(rows, pq, aq, bq, obs, rounding_gain(pi, a, b, qlog2), floor)
    return path, cert, rows


def decode64(pi, a, b, obs):
    """The f64 row-A0 decode (first-index argmax on the forward's own sums); path, margin."""
    S, T = obs.shape
    d = pi[None, :] + b[:, obs[:, 0]].T
    rows = np.empty((T, S, a.shape[0]))
    rows[0] = d
    for t in range(1, T):
        d = (d[:, :, None] + a[None, :, :]).max(axis=1) + b[:, obs[:, t]].T
        rows[t] = d
    path = np.empty((S, T), np.int64)
    srt = np.sort(rows[T - 1], axis=1)
    gap = srt[:, -1] - srt[:, -2]
    cur = rows[T - 1].argmax(axis=1)
    path[:, T - 1] = cur
    for t in range(T - 1, 0, -1):
        x = rows[t - 1] + a[:, cur].T
        xs = np.sort(x, axis=1)
        gap = np.minimum(gap, xs[:, -1] - xs[:, -2])
        cur = x.argmax(axis=1)
        path[:, t - 1] = cur
    return path, gap


def main():
    sys.path.insert(0, "consistent-viterbi_amd")
    from cviterbi import synth

    B = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    chunk = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    qlog2 = int(sys.argv[3]) if len(sys.argv) > 3 else QLOG2
    c = synth.config("c4", B)
    pi, a, b = c["pi"], c["a"], c["b"]
    T = 512
    obs = c["obs"].reshape(B, T)
    certs, same, gaps = [], [], []
    t0 = time.time()
    for s0 in range(0, B, chunk):
        o = obs[s0:s0 + chunk]
        p64, g64 = decode64(pi, a, b, o)
        pq, cert, _ = decode(pi, a, b, o, qlog2)
        eq = (pq == p64).all(axis=1)
        assert np.all(eq[cert]), "a certified fixed-point path differs from the f64 path"
        certs.append(cert); same.append(eq); gaps.append(g64)
        print(f"{s0 + len(o)}/{B} seqs, {time.time() - t0:.0f} s: certified {np.concatenate(certs).mean():.4f}"
              f", fixed path == f64 {np.concatenate(same).mean():.4f}", flush=True)
    cert = np.concatenate(certs); eq = np.concatenate(same); g = np.concatenate(gaps)
    thr, end = thresholds(T, rounding_gain(pi, a, b, qlog2))
    print(f"\nB={B} N=256 T=512 (config 4, first {B} sequences), q = 2^{qlog2}, F = {FLOOR}")
    print(f"rounding gain g = {rounding_gain(pi, a, b, qlog2):.3e}; thr_1 = {thr[1]}, thr_{T - 1} = {thr[T - 1]},"
          f" terminal = {end} units ({end * 2.0 ** qlog2:.3e} log10 units)")
    print(f"f64 path margin quantiles 1/5/10/50% = {np.quantile(g, [0.01, 0.05, 0.10, 0.5])}")
    print(f"fixed-point path == f64 path {eq.mean():.4f}; CERTIFIED {cert.mean():.4f} ({cert.sum()} of {B})")
    print(f"certified paths equal to the f64 path: {int((eq & cert).sum())} of {int(cert.sum())}")
    print(f"uncertified margins (f64): {np.sort(g[~cert])}")


if __name__ == "__main__":
    main()
