"""Expected counts for EM on MI355X (cv_expected_counts*): the E-step's statistics of (pi, A),
and of the emission table b of the discrete model (cv_expected_counts_model*).

For the model as posterior_batch reads it, over the sequences with status SEQ_OK:
pi_cnt[i] = sum_s gamma_0[i] and a_cnt[i, j] = sum_s sum_t P(s_t = i, s_t+1 = j | o, tags),
together with loglik, gamma (optional) and status exactly as posterior_batch returns them.
The outputs are overwritten, not accumulated: a multi-GPU caller adds the arrays of its shards.
f64, deterministic (no atomic adds); see include/cviterbi.h for the definitions and the error
bound.  As in posterior.py, CV_EINFEASIBLE is not raised: the statuses say which sequences.

An EM loop for (pi, A) under fixed emissions is three lines:

    for _ in range(rounds):
        _, pi_cnt, a_cnt, _, _ = expected_counts(hmm, offsets, obs)
        pi, a = reestimate(pi_cnt, a_cnt, pi, a)
        hmm = HMM(pi, a, b)

Full EM for the discrete model (pi, A, b), with any M-step of the caller's in place of
reestimate_model (priors, smoothing, tied rows, the arrays of several shards added up):

    for _ in range(rounds):
        _, pi_cnt, a_cnt, b_cnt, _, _ = expected_counts_model(hmm, offsets, obs)
        pi, a, b = reestimate_model(pi_cnt, a_cnt, b_cnt, pi, a, b)
        hmm = HMM(pi, a, b)

With weight= the three arrays are the gradient of sum_s weight[s] * loglik[s] in log10 (pi, A, b).
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib as L
from .emissions import _dev_ld, _host_emis, _ptr
from .hmm import HMM
from .posterior import _opts, _p


def _outputs(hmm, nseq, total, gamma):
    n = hmm.nstates()
    return (np.zeros(max(nseq, 0), np.float64), np.zeros(n, np.float64), np.zeros((n, n), np.float64),
            np.zeros((max(total, 0), n), np.float64) if gamma else None, np.zeros(max(nseq, 0), np.uint8))


def _host_opts(forced, kernel, workspace_bytes):
    o = _opts(kernel, workspace_bytes)
    if forced is not None:
        forced = np.ascontiguousarray(forced, np.int32)
        o.forced = forced.ctypes.data
    return o, forced  # forced: kept alive by the caller until the call has returned


def expected_counts(hmm: HMM, offsets, obs, forced=None, gamma=False, kernel="auto", workspace_bytes=0):
    """CSR sequences (offsets[B+1], flat obs) -> (loglik f64[B], pi_cnt f64[N], a_cnt f64[N, N]
    from-major, gamma f64[sum T, N] or None, status u8[B]).  forced as in posterior_batch."""
    offsets = np.ascontiguousarray(offsets, np.int64)
    obs = np.ascontiguousarray(obs, np.int32)
    nseq = offsets.shape[0] - 1
    total = int(offsets[-1]) if nseq >= 0 else 0
    loglik, pi_cnt, a_cnt, gamma_out, status = _outputs(hmm, nseq, total, gamma)
    o, forced = _host_opts(forced, kernel, workspace_bytes)
    st = L.lib().cv_expected_counts(hmm.handle, nseq, _p(offsets), _p(obs), ctypes.byref(o), _p(loglik), _p(pi_cnt),
                                    _p(a_cnt), _p(gamma_out), _p(status))
    if st != L.CV_EINFEASIBLE:
        L.check(st)
    return loglik, pi_cnt, a_cnt, gamma_out, status


def expected_counts_emissions(hmm: HMM, offsets, emis, forced=None, gamma=False, kernel="auto", workspace_bytes=0):
    """The same under emission scores emis f64[sum T, >= N] (log10), read as posterior_emissions
    reads them; the handle's own b is ignored.  Array handling as in decode_emissions."""
    offsets, emis, ld, nseq, total = _host_emis(hmm, offsets, emis)
    loglik, pi_cnt, a_cnt, gamma_out, status = _outputs(hmm, nseq, total, gamma)
    o, forced = _host_opts(forced, kernel, workspace_bytes)
    st = L.lib().cv_expected_counts_emissions(hmm.handle, nseq, _p(offsets), _p(emis), int(ld), ctypes.byref(o),
                                              _p(loglik), _p(pi_cnt), _p(a_cnt), _p(gamma_out), _p(status))
    if st != L.CV_EINFEASIBLE:
        L.check(st)
    return loglik, pi_cnt, a_cnt, gamma_out, status


def expected_counts_model(hmm: HMM, offsets, obs, weight=None, forced=None, gamma=False, kernel="auto",
                          workspace_bytes=0):
    """CSR sequences -> (loglik f64[B], pi_cnt f64[N], a_cnt f64[N, N], b_cnt f64[N, V], gamma
    f64[sum T, N] or None, status u8[B]): expected_counts plus the expected emission counts
    b_cnt[j, v] = sum of gamma_e[j] over the elements e of OK sequences with obs[e] = v.  weight
    (optional, f64[B]) multiplies every term of sequence s, gamma's rows included: the arrays are
    then the gradient of sum_s weight[s] loglik[s] in log10 pi, log10 A and log10 b."""
    offsets = np.ascontiguousarray(offsets, np.int64)
    obs = np.ascontiguousarray(obs, np.int32)
    nseq = offsets.shape[0] - 1
    total = int(offsets[-1]) if nseq >= 0 else 0
    loglik, pi_cnt, a_cnt, gamma_out, status = _outputs(hmm, nseq, total, gamma)
    b_cnt = np.zeros((hmm.nstates(), hmm.nobs()), np.float64)
    if weight is not None:
        weight = np.ascontiguousarray(weight, np.float64)
        if weight.shape != (max(nseq, 0),):
            raise ValueError(f"weight must be [B = {nseq}], got {weight.shape}")
    o, forced = _host_opts(forced, kernel, workspace_bytes)
    st = L.lib().cv_expected_counts_model(hmm.handle, nseq, _p(offsets), _p(obs), _p(weight), ctypes.byref(o),
                                          _p(loglik), _p(pi_cnt), _p(a_cnt), _p(b_cnt), _p(gamma_out), _p(status))
    if st != L.CV_EINFEASIBLE:
        L.check(st)
    return loglik, pi_cnt, a_cnt, b_cnt, gamma_out, status


def _dev_opts(offsets_dev, offsets_host, forced_dev, kernel, stream, workspace_bytes):
    nseq = (len(offsets_host) if offsets_host is not None else offsets_dev.numel()) - 1
    oh = np.ascontiguousarray(offsets_host, np.int64) if offsets_host is not None else None
    o = _opts(kernel, workspace_bytes, stream)
    if forced_dev is not None:
        o.forced = _ptr(forced_dev)
    return nseq, oh, o


def expected_counts_device(hmm: HMM, offsets_dev, obs_dev, loglik_dev, pi_cnt_dev, a_cnt_dev, status_dev,
                           gamma_dev=None, offsets_host=None, forced_dev=None, kernel="auto", stream=None,
                           workspace_bytes=0):
    """Device-pointer variant (ints or objects with data_ptr(), e.g. torch tensors): enqueued on
    `stream`, returns without synchronizing.  pi_cnt_dev f64[N], a_cnt_dev f64[N, N]."""
    nseq, oh, o = _dev_opts(offsets_dev, offsets_host, forced_dev, kernel, stream, workspace_bytes)
    L.check(L.lib().cv_expected_counts_device(hmm.handle, nseq, _p(oh), _ptr(offsets_dev), _ptr(obs_dev), ctypes.byref(o),
                                              _ptr(loglik_dev), _ptr(pi_cnt_dev), _ptr(a_cnt_dev), _ptr(gamma_dev),
                                              _ptr(status_dev)))


def expected_counts_emissions_device(hmm: HMM, offsets_dev, emis_dev, loglik_dev, pi_cnt_dev, a_cnt_dev, status_dev,
                                     gamma_dev=None, offsets_host=None, forced_dev=None, kernel="auto", stream=None,
                                     workspace_bytes=0):
    """Device-pointer variant under emission scores; emis_dev as in decode_emissions_device."""
    ld = _dev_ld(hmm, emis_dev)
    nseq, oh, o = _dev_opts(offsets_dev, offsets_host, forced_dev, kernel, stream, workspace_bytes)
    L.check(L.lib().cv_expected_counts_emissions_device(hmm.handle, nseq, _p(oh), _ptr(offsets_dev), _ptr(emis_dev),
                                                        int(ld), ctypes.byref(o), _ptr(loglik_dev), _ptr(pi_cnt_dev),
                                                        _ptr(a_cnt_dev), _ptr(gamma_dev), _ptr(status_dev)))


def expected_counts_model_device(hmm: HMM, offsets_dev, obs_dev, loglik_dev, pi_cnt_dev, a_cnt_dev, b_cnt_dev,
                                 status_dev, weight_dev=None, gamma_dev=None, offsets_host=None, forced_dev=None,
                                 kernel="auto", stream=None, workspace_bytes=0):
    """Device-pointer variant of expected_counts_model: b_cnt_dev f64[N, V], weight_dev f64[B] or
    None, gamma_dev f64[sum T, N] or None (the rows weight[s] * gamma)."""
    nseq, oh, o = _dev_opts(offsets_dev, offsets_host, forced_dev, kernel, stream, workspace_bytes)
    L.check(L.lib().cv_expected_counts_model_device(hmm.handle, nseq, _p(oh), _ptr(offsets_dev), _ptr(obs_dev),
                                                    _ptr(weight_dev), ctypes.byref(o), _ptr(loglik_dev),
                                                    _ptr(pi_cnt_dev), _ptr(a_cnt_dev), _ptr(b_cnt_dev),
                                                    _ptr(gamma_dev), _ptr(status_dev)))


def reestimate(pi_cnt, a_cnt, pi_prev, a_prev):
    """The M-step for (pi, A): expected counts -> (pi, a) in log10, each row normalised to sum 1
    (a count of 0 gives -inf).  pi_prev, a_prev: the current log10 parameters; a row of a_cnt
    whose sum is 0 (a state never left) keeps a_prev's row, and pi_prev is kept if pi_cnt sums
    to 0 (no sequence counted)."""
    pi_cnt = np.asarray(pi_cnt, np.float64)
    a_cnt = np.asarray(a_cnt, np.float64)
    pi_prev = np.asarray(pi_prev, np.float64)
    a_prev = np.asarray(a_prev, np.float64)
    if a_cnt.ndim != 2 or a_cnt.shape[0] != a_cnt.shape[1] or pi_cnt.shape != (a_cnt.shape[0],):
        raise ValueError(f"pi_cnt {pi_cnt.shape} and a_cnt {a_cnt.shape} must be [N] and [N, N]")
    if pi_prev.shape != pi_cnt.shape or a_prev.shape != a_cnt.shape:
        raise ValueError("pi_prev / a_prev must have the shapes of pi_cnt / a_cnt")
    with np.errstate(divide="ignore"):
        total = pi_cnt.sum()
        pi = np.log10(pi_cnt / total) if total > 0 else pi_prev.copy()
        rows = a_cnt.sum(axis=1)
        a = a_prev.copy()
        live = rows > 0
        a[live] = np.log10(a_cnt[live] / rows[live, None])
    return pi, a


def reestimate_model(pi_cnt, a_cnt, b_cnt, pi_prev, a_prev, b_prev):
    """The M-step for (pi, A, b): reestimate's rules for pi and A, and each state's row of b_cnt
    [N, V] normalised to sum 1 (a count of 0 gives -inf); a row whose sum is 0 (a state never
    visited) keeps b_prev's row.  Returns (pi, a, b) in log10."""
    pi, a = reestimate(pi_cnt, a_cnt, pi_prev, a_prev)
    b_cnt = np.asarray(b_cnt, np.float64)
    b_prev = np.asarray(b_prev, np.float64)
    if b_cnt.ndim != 2 or b_cnt.shape[0] != pi.shape[0] or b_cnt.shape[1] < 1:
        raise ValueError(f"b_cnt {b_cnt.shape} must be [N = {pi.shape[0]}, V]")
    if b_prev.shape != b_cnt.shape:
        raise ValueError("b_prev must have the shape of b_cnt")
    with np.errstate(divide="ignore"):
        rows = b_cnt.sum(axis=1)
        b = b_prev.copy()
        live = rows > 0
        b[live] = np.log10(b_cnt[live] / rows[live, None])
    return pi, a, b
