"""Likelihood gradients under emission scores on MI355X (cv_loglik_grad_emissions*).

For F = sum_s weights[s] * log10 P(o_s | model, tags) over the sequences with status SEQ_OK, in
log10 units on both sides:

    emis_grad[e, j] = dF / d emis[e, j]     = weights[s] * gamma_e[j]
    pi_grad[i]      = dF / d log10 pi[i]    = sum_s weights[s] * gamma_0(s)[i]
    a_grad[i, j]    = dF / d log10 A[i, j]  = sum_s weights[s] * sum_t xi_t(s)(i, j)

that is expected_counts_emissions with a weight per sequence: loglik and status are that call's bit
for bit, and with weights None (all 1) so are pi_grad, a_grad and emis_grad.  A sequence that is
not SEQ_OK contributes nothing and its emis_grad rows are 0 whatever its weight holds; an OK
sequence with a non-finite weight makes the outputs it touches non-finite.  f64, deterministic (no
atomic adds); see include/cviterbi.h for the error bounds.  cviterbi.autograd.sequence_loglik puts
this behind torch's loss.backward().  As in posterior.py, CV_EINFEASIBLE is not raised.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib as L
from .counts import _dev_opts, _host_opts
from .emissions import _dev_ld, _host_emis, _ptr
from .hmm import HMM
from .posterior import _p


def loglik_grad_emissions(hmm: HMM, offsets, emis, weights=None, forced=None, emis_grad=True, kernel="auto",
                          workspace_bytes=0):
    """CSR sequences (offsets[B+1]) with emission scores emis f64[sum T, >= N] (log10) and weights
    f64[B] (None: all 1) -> (loglik f64[B], pi_grad f64[N], a_grad f64[N, N] from-major, emis_grad
    f64[sum T, N] or None, status u8[B]).  Array handling as in decode_emissions; forced as in
    posterior_batch."""
    offsets, emis, ld, nseq, total = _host_emis(hmm, offsets, emis)
    n = hmm.nstates()
    if weights is not None:
        weights = np.ascontiguousarray(weights, np.float64)
        if weights.shape != (max(nseq, 0),):
            raise ValueError(f"weights must have shape ({max(nseq, 0)},), got {weights.shape}")
    loglik = np.zeros(max(nseq, 0), np.float64)
    status = np.zeros(max(nseq, 0), np.uint8)
    pi_grad, a_grad = np.zeros(n, np.float64), np.zeros((n, n), np.float64)
    egrad = np.zeros((max(total, 0), n), np.float64) if emis_grad else None
    o, forced = _host_opts(forced, kernel, workspace_bytes)
    st = L.lib().cv_loglik_grad_emissions(hmm.handle, nseq, _p(offsets), _p(emis), int(ld), _p(weights), ctypes.byref(o),
                                          _p(loglik), _p(pi_grad), _p(a_grad), _p(egrad), n, _p(status))
    if st != L.CV_EINFEASIBLE:
        L.check(st)
    return loglik, pi_grad, a_grad, egrad, status


def loglik_grad_emissions_device(hmm: HMM, offsets_dev, emis_dev, loglik_dev, pi_grad_dev, a_grad_dev, status_dev,
                                 weight_dev=None, emis_grad_dev=None, offsets_host=None, forced_dev=None, kernel="auto",
                                 stream=None, workspace_bytes=0):
    """Device-pointer variant (ints or objects with data_ptr(), e.g. torch tensors): enqueued on
    `stream`, returns without synchronizing.  emis_dev as in decode_emissions_device; emis_grad_dev
    (optional) likewise: a 2-D float64 torch tensor with at least N columns and stride(1) == 1
    whose stride(0) is its row stride (the columns beyond N are never written), or a pointer to
    rows of exactly N doubles.  weight_dev f64[B] (None: all 1), pi_grad_dev f64[N], a_grad_dev
    f64[N, N]."""
    ld = _dev_ld(hmm, emis_dev)
    ld_grad = _dev_ld(hmm, emis_grad_dev) if emis_grad_dev is not None else hmm.nstates()
    nseq, oh, o = _dev_opts(offsets_dev, offsets_host, forced_dev, kernel, stream, workspace_bytes)
    L.check(L.lib().cv_loglik_grad_emissions_device(hmm.handle, nseq, _p(oh), _ptr(offsets_dev), _ptr(emis_dev), int(ld),
                                                    _ptr(weight_dev), ctypes.byref(o), _ptr(loglik_dev),
                                                    _ptr(pi_grad_dev), _ptr(a_grad_dev), _ptr(emis_grad_dev),
                                                    int(ld_grad), _ptr(status_dev)))
