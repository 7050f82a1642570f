"""Diagonal-covariance Gaussian emissions on MI355X (cv_gauss_emissions*, cv_expected_counts_gauss*).

A Gaussian HMM on raw observation vectors x f64[sum T, D]: the handle holds (pi, A) -- gauss_hmm
gives it a one-symbol dummy b, which these entries ignore -- and every call takes mean f64[N, D]
and var f64[N, D].

    gauss_emissions(hmm, x, mean, var)        E[e, j] = log10 N(x_e; mean_j, var_j), f64[rows, N]

feeds decode_emissions, score_emissions, posterior_emissions, expected_counts_emissions and
loglik_grad_emissions.  expected_counts_gauss is, by definition, gauss_emissions followed by
loglik_grad_emissions, plus the statistics of the Gaussian M-step over the OK sequences, with
g_e = weight[s] * gamma_e and y = x - center:

    g_cnt[j] = sum_e g_e[j]     m1[j, d] = sum_e g_e[j] y[e, d]     m2[j, d] = sum_e g_e[j] y[e, d]^2

The whole EM loop (fit_gauss does this on device-resident x):

    for _ in range(rounds):
        ll, pi_cnt, a_cnt, g, m1, m2, _, _ = expected_counts_gauss(hmm, offsets, x, mean, var, center=c)
        pi, a = reestimate(pi_cnt, a_cnt, pi, a)
        mean, var = reestimate_gauss(g, m1, m2, c, mean, var)
        hmm = gauss_hmm(pi, a)

f64, deterministic (no atomic adds); see include/cviterbi.h for the definitions and the error
bounds.  As in posterior.py, CV_EINFEASIBLE is not raised: the statuses say which sequences.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib as L
from .counts import _dev_opts, _host_opts, reestimate
from .emissions import _dev_ld, _host_emis, _ptr
from .hmm import HMM
from .posterior import _p


def gauss_hmm(pi, a, device=0):
    """An HMM handle for the Gaussian entries: (pi, A) in log10 and a one-symbol dummy b."""
    pi = np.asarray(pi, np.float64)
    return HMM(pi, a, np.zeros((pi.shape[0], 1), np.float64), device=device)


class _Cols:
    """What _host_emis / _dev_ld ask of a handle, for an array of D columns instead of N."""

    def __init__(self, cols, device):
        self._cols, self.device = int(cols), device

    def nstates(self):
        return self._cols


def _params(hmm, mean, var):
    n = hmm.nstates()
    mean = np.ascontiguousarray(mean, np.float64)
    var = np.ascontiguousarray(var, np.float64)
    if mean.ndim != 2 or mean.shape[0] != n or var.shape != mean.shape:
        raise ValueError(f"mean {mean.shape} and var {var.shape} must both be [N = {n}, D]")
    return mean, var, mean.shape[1]


def _center(center, d):
    if center is None:
        return None
    center = np.ascontiguousarray(center, np.float64)
    if center.shape != (d,):
        raise ValueError(f"center must be [D = {d}], got {center.shape}")
    return center


def gauss_emissions(hmm: HMM, x, mean, var, out=None):
    """x f64[rows, >= D] (a row stride passes without a copy), mean and var f64[N, D] -> E
    f64[rows, N].  out (optional): a C-contiguous f64[rows, >= N] array to write into; its columns
    beyond N are left as they are."""
    mean, var, d = _params(hmm, mean, var)
    x = np.asarray(x)
    rows = x.shape[0] if x.ndim == 2 else 0
    _, x, ldx, _, _ = _host_emis(_Cols(d, hmm.device), np.array([0, rows], np.int64), x)
    n = hmm.nstates()
    if out is None:
        out = np.zeros((rows, n), np.float64)
    elif (not isinstance(out, np.ndarray) or out.dtype != np.float64 or out.ndim != 2 or not out.flags.c_contiguous
          or out.shape[0] != rows or out.shape[1] < n):
        raise ValueError(f"out must be a C-contiguous float64 array [{rows}, >= {n}]")
    L.check(L.lib().cv_gauss_emissions(hmm.handle, rows, _p(x), int(ldx), d, _p(mean), _p(var), _p(out), out.shape[1]))
    return out


def gauss_emissions_device(hmm: HMM, x_dev, mean, var, emis_dev, rows=None, D=None, stream=None):
    """Device-pointer variant: x_dev a 2-D float64 torch tensor [rows, >= D] with stride(1) == 1 (its
    stride(0) is the row stride) or a pointer to rows of exactly D doubles (then give rows);
    emis_dev likewise [rows, >= N].  mean and var are host arrays.  Enqueued on `stream`."""
    mean, var, d = _params(hmm, mean, var)
    ldx = _dev_ld(_Cols(d, hmm.device), x_dev)
    ld = _dev_ld(hmm, emis_dev)
    if rows is None:
        rows = x_dev.shape[0]
    o = L.opts(L.DTYPE_F64, stream=stream)
    L.check(L.lib().cv_gauss_emissions_device(hmm.handle, int(rows), _ptr(x_dev), int(ldx), d, _p(mean), _p(var),
                                              ctypes.byref(o), _ptr(emis_dev), int(ld)))


def expected_counts_gauss(hmm: HMM, offsets, x, mean, var, weight=None, center=None, forced=None, gamma=False,
                          kernel="auto", workspace_bytes=0):
    """CSR sequences (offsets[B+1]) of observation vectors x f64[sum T, >= D] -> (loglik f64[B],
    pi_cnt f64[N], a_cnt f64[N, N], g_cnt f64[N], m1 f64[N, D], m2 f64[N, D], gamma f64[sum T, N]
    or None (the rows weight[s] * gamma), status u8[B])."""
    mean, var, d = _params(hmm, mean, var)
    center = _center(center, d)
    offsets, x, ldx, nseq, total = _host_emis(_Cols(d, hmm.device), offsets, x)
    n = hmm.nstates()
    if weight is not None:
        weight = np.ascontiguousarray(weight, np.float64)
        if weight.shape != (max(nseq, 0),):
            raise ValueError(f"weight must be [B = {nseq}], got {weight.shape}")
    loglik = np.zeros(max(nseq, 0), np.float64)
    status = np.zeros(max(nseq, 0), np.uint8)
    pi_cnt, a_cnt, g_cnt = np.zeros(n, np.float64), np.zeros((n, n), np.float64), np.zeros(n, np.float64)
    m1, m2 = np.zeros((n, d), np.float64), np.zeros((n, d), np.float64)
    gamma_out = np.zeros((max(total, 0), n), np.float64) if gamma else None
    o, forced = _host_opts(forced, kernel, workspace_bytes)
    st = L.lib().cv_expected_counts_gauss(hmm.handle, nseq, _p(offsets), _p(x), int(ldx), d, _p(mean), _p(var),
                                          _p(weight), _p(center), ctypes.byref(o), _p(loglik), _p(pi_cnt), _p(a_cnt),
                                          _p(g_cnt), _p(m1), _p(m2), _p(gamma_out), _p(status))
    if st != L.CV_EINFEASIBLE:
        L.check(st)
    return loglik, pi_cnt, a_cnt, g_cnt, m1, m2, gamma_out, status


def expected_counts_gauss_device(hmm: HMM, offsets_dev, x_dev, mean, var, loglik_dev, pi_cnt_dev, a_cnt_dev, g_cnt_dev,
                                 m1_dev, m2_dev, status_dev, weight_dev=None, center=None, gamma_dev=None,
                                 offsets_host=None, forced_dev=None, kernel="auto", stream=None, workspace_bytes=0):
    """Device-pointer variant (ints or objects with data_ptr(), e.g. torch tensors): enqueued on
    `stream`, returns without synchronizing.  x_dev as in gauss_emissions_device; mean, var and
    center are host arrays; g_cnt_dev f64[N], m1_dev and m2_dev f64[N, D]."""
    mean, var, d = _params(hmm, mean, var)
    center = _center(center, d)
    ldx = _dev_ld(_Cols(d, hmm.device), x_dev)
    nseq, oh, o = _dev_opts(offsets_dev, offsets_host, forced_dev, kernel, stream, workspace_bytes)
    L.check(L.lib().cv_expected_counts_gauss_device(hmm.handle, nseq, _p(oh), _ptr(offsets_dev), _ptr(x_dev), int(ldx), d,
                                                    _p(mean), _p(var), _ptr(weight_dev), _p(center), ctypes.byref(o),
                                                    _ptr(loglik_dev), _ptr(pi_cnt_dev), _ptr(a_cnt_dev),
                                                    _ptr(g_cnt_dev), _ptr(m1_dev), _ptr(m2_dev), _ptr(gamma_dev),
                                                    _ptr(status_dev)))


def reestimate_gauss(g_cnt, m1, m2, center, mean_prev, var_prev, var_floor=1e-6):
    """The Gaussian M-step: mean = center + m1 / g, var = max(m2 / g - (m1 / g)^2, var_floor); a
    state with g <= 0 (never visited) keeps its previous row.  center None means 0."""
    g = np.asarray(g_cnt, np.float64)
    m1 = np.asarray(m1, np.float64)
    m2 = np.asarray(m2, np.float64)
    mean_prev = np.asarray(mean_prev, np.float64)
    var_prev = np.asarray(var_prev, np.float64)
    if m1.ndim != 2 or m2.shape != m1.shape or g.shape != (m1.shape[0],):
        raise ValueError(f"g_cnt {g.shape}, m1 {m1.shape}, m2 {m2.shape} must be [N], [N, D], [N, D]")
    if mean_prev.shape != m1.shape or var_prev.shape != m1.shape:
        raise ValueError("mean_prev / var_prev must have the shape of m1")
    c = np.zeros(m1.shape[1]) if center is None else np.asarray(center, np.float64)
    mean, var = mean_prev.copy(), var_prev.copy()
    live = g > 0
    mu = m1[live] / g[live, None]
    mean[live] = c + mu
    var[live] = np.maximum(m2[live] / g[live, None] - mu * mu, var_floor)
    return mean, var


def fit_gauss(pi, a, mean, var, offsets, x, rounds, tol=0.0, var_floor=1e-6, forced=None, device=0, history=None):
    """EM for the Gaussian HMM from (pi, a) in log10 and mean, var f64[N, D]: x f64[sum T, D] is
    uploaded once, center is the data's per-dimension mean, and every round is one
    expected_counts_gauss_device call followed by reestimate and reestimate_gauss.  Stops after
    `rounds` rounds or when the total log-likelihood gains less than tol (> 0).  Returns (pi, a,
    mean, var, logliks): logliks[r] is the total log10-likelihood of the OK sequences under round
    r's input parameters.  history (a list, optional) receives one dict per round: the input
    parameters and the statistics of that round."""
    import torch

    dev = torch.device("cuda", device)
    pi, a = np.asarray(pi, np.float64), np.asarray(a, np.float64)
    mean, var = np.array(mean, np.float64), np.array(var, np.float64)
    offsets = np.ascontiguousarray(offsets, np.int64)
    x = np.ascontiguousarray(x, np.float64)
    n, d = mean.shape
    nseq, total = len(offsets) - 1, int(offsets[-1])
    center = x[int(offsets[0]):total].mean(axis=0) if total > int(offsets[0]) else np.zeros(d)
    x_dev = torch.from_numpy(x).to(dev)
    off_dev = torch.from_numpy(offsets).to(dev)
    forced_dev = None if forced is None else torch.from_numpy(np.ascontiguousarray(forced, np.int32)).to(dev)
    f64 = dict(dtype=torch.float64, device=dev)
    ll_dev, st_dev = torch.zeros(max(nseq, 1), **f64), torch.zeros(max(nseq, 1), dtype=torch.uint8, device=dev)
    pi_dev, a_dev, g_dev = torch.zeros(n, **f64), torch.zeros(n, n, **f64), torch.zeros(n, **f64)
    m1_dev, m2_dev = torch.zeros(n, d, **f64), torch.zeros(n, d, **f64)
    logliks = []
    for _ in range(rounds):
        hmm = gauss_hmm(pi, a, device=device)
        expected_counts_gauss_device(hmm, off_dev, x_dev, mean, var, ll_dev, pi_dev, a_dev, g_dev, m1_dev, m2_dev,
                                     st_dev, center=center, offsets_host=offsets, forced_dev=forced_dev,
                                     stream=torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
        ll, status = ll_dev[:nseq].cpu().numpy(), st_dev[:nseq].cpu().numpy()
        stats = dict(pi_cnt=pi_dev.cpu().numpy(), a_cnt=a_dev.cpu().numpy(), g_cnt=g_dev.cpu().numpy(),
                     m1=m1_dev.cpu().numpy(), m2=m2_dev.cpu().numpy())
        logliks.append(float(ll[status == L.SEQ_OK].sum()))
        if history is not None:
            history.append(dict(pi=pi, a=a, mean=mean, var=var, center=center, loglik=ll, status=status, **stats))
        pi, a = reestimate(stats["pi_cnt"], stats["a_cnt"], pi, a)
        mean, var = reestimate_gauss(stats["g_cnt"], stats["m1"], stats["m2"], center, mean, var, var_floor)
        if tol > 0 and len(logliks) > 1 and logliks[-1] - logliks[-2] < tol:
            break
    return pi, a, mean, var, logliks
