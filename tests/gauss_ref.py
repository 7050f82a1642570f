"""References for the Gaussian entries (DESIGN.md "Gaussian emissions"), plain numpy f64:
  np_density      E[e][j] = c_j - kappa sum_d (x - mean)^2 w in the kernel's operation order (one
                  rounding in the difference, one in the square, an fma per dimension in ascending
                  d -- emulated by error-free transformations -- then c_j - kappa q);
  mp_density      the same quantity in 60-digit mpmath, and density_bound, the header's bound;
  np_gauss_counts the statistics: grad_ref.np_grad's forward-backward on 10^E (the scaled rows of
                  bcnt_ref.np_model_counts under dense scores), then g.T @ [1 | y | y^2], the
                  abs-statistics and the header's bounds;
  enumerate_gauss_counts   every state path of a tiny model, which shares nothing with the recursions.
"""
import itertools

import numpy as np

import grad_ref

U = 2.0 ** -53
KAPPA = 0.21714724095162591  # 0.5 / ln 10
SEQ_OK, SEQ_INFEASIBLE, SEQ_EMPTY, SEQ_BADOBS = 0, 1, 2, 3


def _split(a):
    t = 134217729.0 * a
    hi = t - (t - a)
    return hi, a - hi


def fma(a, b, c):
    """round(a * b + c) with the product's rounding error added back before the sum is rounded
    (Dekker's product, Knuth's sum): a hardware fma's result except where that last addition
    meets a tie, and the plain a * b + c where an intermediate leaves the finite range."""
    with np.errstate(all="ignore"):
        p = a * b
        ah, al = _split(a)
        bh, bl = _split(b)
        e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
        h = p + c
        z = h - p
        l = (p - (h - z)) + (c - z)
        r = h + (l + e)
        return np.where(np.isfinite(r) & np.isfinite(e), r, p + c)


def tables(mean, var):
    """(w [N, D], c [N], c_abs [N]) as the host side of cv_gauss_emissions computes them."""
    var = np.asarray(var, np.float64)
    logs = np.log10(6.283185307179586 * var)
    c = np.zeros(var.shape[0])
    for d in range(var.shape[1]):  # ascending d, plain f64 sum
        c = c + logs[:, d]
    return 1.0 / var, -0.5 * c, 0.5 * np.abs(logs).sum(axis=1)


def np_density(x, mean, var):
    """E f64[rows, N]; a row of x with a NaN or +-inf gives NaNs."""
    x = np.asarray(x, np.float64)
    mean = np.asarray(mean, np.float64)
    w, c, _ = tables(mean, var)
    q = np.zeros((x.shape[0], mean.shape[0]))
    with np.errstate(all="ignore"):
        for d in range(mean.shape[1]):
            diff = x[:, d, None] - mean[None, :, d]
            s = diff * diff
            q = fma(s, np.broadcast_to(w[None, :, d], s.shape), q)
        E = c[None, :] - KAPPA * q
    E[~np.isfinite(x).all(axis=1)] = np.nan
    return E


def density_bound(x, mean, var, E):
    """The header's bound per entry, [rows, N]: (D + 8) u (kappa q + c_abs_j) + u |E|."""
    x, mean, var = (np.asarray(v, np.float64) for v in (x, mean, var))
    _, _, c_abs = tables(mean, var)
    D = mean.shape[1]
    with np.errstate(all="ignore"):
        q = (((x[:, None, :] - mean[None]) ** 2) / var[None]).sum(axis=2)
        return (D + 8) * U * (KAPPA * q + c_abs[None, :]) + U * np.abs(E)


def mp_density(x, mean, var, dps=60):
    """log10 N(x_e; mean_j, var_j) in dps-digit arithmetic, rounded to f64 at the end: [rows, N]."""
    import mpmath as mp

    x, mean, var = (np.asarray(v, np.float64) for v in (x, mean, var))
    out = np.zeros((x.shape[0], mean.shape[0]))
    with mp.workdps(dps):
        ln10 = mp.log(10)
        for j in range(mean.shape[0]):
            cj = -sum(mp.log10(2 * mp.pi * mp.mpf(float(v))) for v in var[j]) / 2
            for e in range(x.shape[0]):
                q = sum((mp.mpf(float(x[e, d])) - mp.mpf(float(mean[j, d]))) ** 2 / mp.mpf(float(var[j, d]))
                        for d in range(mean.shape[1]))
                out[e, j] = float(cj - q / (2 * ln10))
    return out


# ---- statistics ----------------------------------------------------------------------------------
def _phi(x, center):
    x = np.asarray(x, np.float64)
    y = x if center is None else x - np.asarray(center, np.float64)[None, :]
    with np.errstate(all="ignore"):
        return y, y * y


def _moments(g, g_abs, x, center, ok_rows):
    """g_cnt, m1, m2 and their abs-statistics over the rows of OK sequences (a select: the other
    rows may hold NaNs)."""
    y, y2 = _phi(x, center)
    idx = np.nonzero(ok_rows)[0]
    g, g_abs, y, y2 = g[idx], g_abs[idx], y[idx], y2[idx]
    return dict(g=g.sum(axis=0), m1=g.T @ y, m2=g.T @ y2, g_abs=g_abs.sum(axis=0), m1_abs=g_abs.T @ np.abs(y),
                m2_abs=g_abs.T @ y2, ymax=float(np.abs(y).max()) if y.size else 0.0)


def np_gauss_counts(pi, a, E, off, x, w=None, forced=None, center=None):
    """dict(pi, a, gamma [L, N] (the rows w_s gamma), g, m1, m2, their *_abs, status, ymax) for the
    scores E [L, N] (as cv_gauss_emissions returns them) of the observations x [L, D]."""
    off = np.asarray(off, np.int64)
    r = grad_ref.np_grad(pi, a, E, off, w=w, forced=forced)
    ok_rows = np.zeros(len(E), bool)
    ok_rows[int(off[0]):int(off[-1])] = np.repeat(r["status"] == SEQ_OK, np.diff(off))
    out = _moments(r["e"], r["e_abs"], x, center, ok_rows)
    out.update(pi=r["pi"], a=r["a"], pi_abs=r["pi_abs"], a_abs=r["a_abs"], gamma=r["e"], gamma_abs=r["e_abs"],
               status=r["status"])
    return out


def moment_bounds(off, N, ref, w=None):
    """(g, m1, m2) bounds of include/cviterbi.h from the reference's abs-statistics."""
    lens = np.diff(off)
    T, L = int(lens.max()) if len(lens) else 0, int(lens.sum())
    wmax = 1.0 if w is None else float(np.max(np.abs(np.asarray(w)[np.isfinite(w)]), initial=1.0))
    absolute = 1e-290 * L * max(1.0, wmax) * max(1.0, ref["ymax"] ** 2)
    base = 4 * T * (N + 8) + L
    return ((base + 1) * U * ref["g_abs"] + absolute, (base + 3) * U * ref["m1_abs"] + absolute,
            (base + 5) * U * ref["m2_abs"] + absolute)


def enumerate_gauss_counts(pi, a, E, off, x, w=None, forced=None, center=None):
    """The same dict (and loglik [B]) by summing over every state path: N^T terms per sequence."""
    with np.errstate(over="ignore"):
        P, A = 10.0 ** np.asarray(pi, np.float64), 10.0 ** np.asarray(a, np.float64)
    N, nseq = len(P), len(off) - 1
    E = np.asarray(E, np.float64)[:, :N]
    w = np.ones(nseq) if w is None else np.asarray(w, np.float64)
    g, g_abs = np.zeros((len(E), N)), np.zeros((len(E), N))
    pi_c, a_c = np.zeros(N), np.zeros((N, N))
    status = np.zeros(nseq, np.uint8)
    loglik = np.full(nseq, -np.inf)
    for s, (lo, hi) in enumerate(zip(off[:-1], off[1:])):
        T = int(hi - lo)
        if T == 0:
            status[s] = SEQ_EMPTY
            continue
        rows = E[lo:hi]
        if not np.all(np.isfinite(rows) | (rows == -np.inf)):
            status[s] = SEQ_BADOBS
            continue
        Bm = 10.0 ** rows
        total, g0, xi, gm = 0.0, np.zeros(N), np.zeros((N, N)), np.zeros((T, N))
        for path in itertools.product(range(N), repeat=T):
            if forced is not None and any(forced[lo + t] >= 0 and forced[lo + t] != path[t] for t in range(T)):
                continue
            p = P[path[0]]
            for t in range(T):
                p *= Bm[t, path[t]]
                if t > 0:
                    p *= A[path[t - 1], path[t]]
            if p == 0.0:
                continue
            total += p
            g0[path[0]] += p
            for t in range(T):
                gm[t, path[t]] += p
                if t > 0:
                    xi[path[t - 1], path[t]] += p
        if not total > 0:
            status[s] = SEQ_INFEASIBLE
            continue
        loglik[s] = np.log10(total)
        pi_c += g0 / total * w[s]
        a_c += xi / total * w[s]
        g[lo:hi], g_abs[lo:hi] = gm / total * w[s], gm / total * abs(w[s])
    ok_rows = np.zeros(len(E), bool)
    ok_rows[int(off[0]):int(off[-1])] = np.repeat(status == SEQ_OK, np.diff(off))
    out = _moments(g, g_abs, x, center, ok_rows)
    out.update(pi=pi_c, a=a_c, gamma=g, status=status, loglik=loglik)
    return out


def within(got, ref, bound):
    """Largest |got - ref| / bound (asserted <= 1 by the callers)."""
    return float(np.max(np.abs(got - ref) / bound)) if np.size(got) else 0.0
