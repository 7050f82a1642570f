"""References for cv_loglik_grad_emissions* (DESIGN.md "Likelihood gradients"), two of them and
independent of each other:
  np_grad      a plain numpy f64 restatement of the weighted expected-counts algorithm, in the style
               of counts_ref.np_counts (scaled forward rows, R^T U per sequence, the product with
               A), which also returns the |w| statistics the bounds are stated in;
  torch_grad   a pure-torch log-space forward algorithm whose autograd differentiates
               sum_s w_s loglik_s -- no backward recursion of its own.
-inf parameters and scores are masked out of the torch graph (their gradient is exactly 0).
The bounds are those of include/cviterbi.h."""
import numpy as np

U = 2.0 ** -53
SEQ_OK, SEQ_INFEASIBLE, SEQ_EMPTY, SEQ_BADOBS = 0, 1, 2, 3


def a_grad_bound(T, N, L, a_abs):
    """|a_grad - exact|: T the longest sequence of the call, L its elements; a_abs with |w_s|."""
    return (4 * T * (N + 8) + L + 9) * U * a_abs + 1e-290 * L


def pi_grad_bound(T, N, B, pi_abs):
    return (4 * T * (N + 8) + B + 1) * U * pi_abs + 1e-290 * B


def emis_grad_bound(T, N, e_abs, w_rows):
    """Per entry: e_abs = |w_s| gamma, w_rows [L, 1] the weight of each row's sequence."""
    return (4 * T * (N + 8) + 1) * U * e_abs + 1e-290 * np.maximum(1.0, np.abs(w_rows))


def row_weights(off, w):
    """[L, 1]: the weight of the sequence each element belongs to."""
    return np.repeat(np.asarray(w, np.float64), np.diff(off))[:, None]


def _bad_rows(rows):
    with np.errstate(invalid="ignore"):
        return bool(np.any(np.isnan(rows)) or np.any(rows == np.inf) or np.any(np.abs(rows[np.isfinite(rows)]) >= 2.0 ** 40))


def np_grad(pi, a, E, off, w=None, forced=None):
    """dict(pi, a, e: the gradients; pi_abs, a_abs, e_abs: the same with |w_s|; status [B]) of
    F = sum_s w_s log10 P(o_s) over the sequences of positive likelihood.  Tables and scores
    log10 (-inf = 0), forced -1 = free, w None = all 1.  A sequence with a NaN, +inf or huge score
    (BADOBS) counts nothing.  A row whose 10^E would underflow is scaled by its own maximum (the
    scale cancels in gamma and xi); every other row is 10^E as np_counts takes it."""
    with np.errstate(over="ignore"):
        P, A = 10.0 ** np.asarray(pi), 10.0 ** np.asarray(a)
    N, B = len(P), len(off) - 1
    E = np.asarray(E, np.float64)[:, :N]
    w = np.ones(B) if w is None else np.asarray(w, np.float64)
    pi_g, S, pi_abs, S_abs = np.zeros(N), np.zeros((N, N)), np.zeros(N), np.zeros((N, N))
    e_g, e_abs = np.zeros((len(E), N)), np.zeros((len(E), N))
    status = np.zeros(B, np.uint8)
    for s, (lo, hi) in enumerate(zip(off[:-1], off[1:])):
        T = int(hi - lo)
        if T == 0:
            status[s] = SEQ_EMPTY
            continue
        rows = E[lo:hi]
        if _bad_rows(rows):
            status[s] = SEQ_BADOBS
            continue
        with np.errstate(over="ignore", invalid="ignore"):
            Bm = 10.0 ** rows
            top = rows.max(axis=1)
            tiny = np.isfinite(top) & ((Bm.max(axis=1) < 1e-290) | ~np.isfinite(Bm.max(axis=1)))
            Bm[tiny] = 10.0 ** (rows[tiny] - top[tiny, None])
        mask = np.ones((T, N))
        if forced is not None:
            for t in np.nonzero(np.asarray(forced[lo:hi]) >= 0)[0]:
                mask[t] = 0.0
                mask[t, forced[lo + t]] = 1.0
        alpha = np.zeros((T, N))
        for t in range(T):
            y = (P if t == 0 else alpha[t - 1] @ A) * Bm[t] * mask[t]
            if not y.max() > 0:
                status[s] = SEQ_INFEASIBLE
                break
            alpha[t] = y / y.max()
        else:
            R, Us = np.zeros((T, N)), np.zeros((T, N))
            W = np.ones(N)
            for t in range(T - 1, -1, -1):
                rsum = alpha[t] @ W
                gamma = alpha[t] * W / rsum
                e_g[lo + t], e_abs[lo + t] = gamma * w[s], gamma * abs(w[s])
                if t == 0:
                    pi_g += gamma * w[s]
                    pi_abs += gamma * abs(w[s])
                if t < T - 1:
                    R[t] = alpha[t] / rsum
                if t > 0:
                    u = Bm[t] * mask[t] * (W / W.max())
                    Us[t - 1] = u
                    W = A @ u
            X = R.T @ Us
            S += X * w[s]
            S_abs += X * abs(w[s])
    return dict(pi=pi_g, a=A * S, e=e_g, pi_abs=pi_abs, a_abs=A * S_abs, e_abs=e_abs, status=status)


def _mlse10(torch, x, mask, dim):
    """log10 sum_{mask} 10^x along dim and whether anything was summed; x finite everywhere."""
    ln10 = float(np.log(10.0))
    neg = torch.where(mask, x.detach(), torch.full_like(x, -np.inf))
    m = neg.max(dim=dim, keepdim=True).values
    any_ = torch.isfinite(m)
    m = torch.where(any_, m, torch.zeros_like(m))
    s = torch.where(mask, torch.exp((x - m) * ln10), torch.zeros_like(x)).sum(dim=dim, keepdim=True)
    out = torch.log(torch.where(any_, s, torch.ones_like(s))) / ln10 + m
    return out.squeeze(dim), any_.squeeze(dim)


def torch_loglik(torch, emis, off, log_pi, log_a, forced=None):
    """Pure-torch log-space forward algorithm on tensors: [(loglik_s or None)] per sequence, None
    for a sequence that is empty, infeasible or holds a NaN / +inf score.  Differentiable in
    emis, log_pi and log_a; -inf entries are outside the graph."""
    N = log_pi.shape[0]
    fin_pi, fin_a = torch.isfinite(log_pi), torch.isfinite(log_a)
    lp = torch.where(fin_pi, log_pi, torch.zeros_like(log_pi))
    la = torch.where(fin_a, log_a, torch.zeros_like(log_a))
    out = []
    for lo, hi in zip(off[:-1], off[1:]):
        lo, hi = int(lo), int(hi)
        rows = emis[lo:hi, :N]
        if hi == lo or _bad_rows(rows.detach().cpu().numpy()):
            out.append(None)
            continue
        fin_e = torch.isfinite(rows)
        le = torch.where(fin_e, rows, torch.zeros_like(rows))
        val, msk = None, None
        for t in range(hi - lo):
            free = torch.ones(N, dtype=torch.bool)
            if forced is not None and forced[lo + t] >= 0:
                free = torch.zeros(N, dtype=torch.bool)
                free[int(forced[lo + t])] = True
            if t == 0:
                v, m = lp, fin_pi
            else:
                v, m = _mlse10(torch, val[:, None] + la, msk[:, None] & fin_a, 0)
            msk = m & fin_e[t] & free
            val = torch.where(msk, v + le[t], torch.zeros_like(v))
        ll, any_ = _mlse10(torch, val, msk, 0)
        out.append(ll if bool(any_) else None)
    return out


def torch_grad(pi, a, E, off, w=None, forced=None):
    """The second oracle: autograd of sum_s w_s loglik_s through torch_loglik (f64, CPU) ->
    dict(pi, a, e, loglik [B] with nan where the sequence has none)."""
    import torch

    N, B = len(pi), len(off) - 1
    w = np.ones(B) if w is None else np.asarray(w, np.float64)
    lp = torch.tensor(np.asarray(pi, np.float64), requires_grad=True)
    la = torch.tensor(np.asarray(a, np.float64), requires_grad=True)
    em = torch.tensor(np.asarray(E, np.float64)[:, :N].copy(), requires_grad=True)
    lls = torch_loglik(torch, em, off, lp, la, forced)
    loss = sum((ll * float(w[s]) for s, ll in enumerate(lls) if ll is not None), torch.zeros((), dtype=torch.float64))
    grads = [np.zeros(N), np.zeros((N, N)), np.zeros((len(E), N))]
    if loss.requires_grad:
        got = torch.autograd.grad(loss, (lp, la, em), allow_unused=True)
        grads = [z if g is None else g.numpy() for g, z in zip(got, grads)]
    loglik = np.array([np.nan if ll is None else float(ll.detach()) for ll in lls])
    return dict(pi=grads[0], a=grads[1], e=grads[2], loglik=loglik)


def within(got, ref, bound):
    """Largest |got - ref| / bound (asserted <= 1 by the callers)."""
    return float(np.max(np.abs(got - ref) / bound)) if np.size(got) else 0.0


def grad_ratios(got_pi, got_a, got_e, ref, off, N, w, factor=1.0):
    """(a, pi, e) error-to-bound ratios of gradients against np_grad's dict `ref` at `factor` times
    the bounds, T, L and B taken from `off`."""
    lens = np.diff(off)
    T, Lel, B = int(lens.max()), int(lens.sum()), len(lens)
    ra = within(got_a, ref["a"], factor * a_grad_bound(T, N, Lel, ref["a_abs"]))
    rp = within(got_pi, ref["pi"], factor * pi_grad_bound(T, N, B, ref["pi_abs"]))
    re_ = 0.0 if got_e is None else within(got_e, ref["e"], factor * emis_grad_bound(T, N, ref["e_abs"], row_weights(off, w)))
    return ra, rp, re_
