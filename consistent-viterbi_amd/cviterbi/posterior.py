"""Sequence log-likelihood and posterior state marginals on MI355X (cv_posterior_batch*).

The evaluation problem of the standard HMM, on the model as decode_batch's "viterbi"
association reads it: loglik = log10 P(observations | model), gamma[t, j] =
P(state at t = j | observations), path[t] = the first index of max_j gamma[t, j] (posterior
decoding).  f64; see include/cviterbi.h for the numerics and the error bounds.

A sequence of likelihood 0 has status SEQ_INFEASIBLE, loglik -inf, path -1 and gamma rows 0;
the C call then reports CV_EINFEASIBLE, which these wrappers do not raise: the per-sequence
statuses say which sequences it was, and every other sequence's results are valid.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib as L
from .hmm import HMM

_KERNEL = {"auto": L.KERNEL_AUTO, "generic": L.KERNEL_GENERIC, "trellis": L.KERNEL_TRELLIS,
           "trellis_f64": L.KERNEL_TRELLIS_F64}


def _p(x):
    return x.ctypes.data_as(ctypes.c_void_p) if x is not None else None


def _opts(kernel, workspace_bytes, stream=None, dtype="f64"):
    dt = {"f64": L.DTYPE_F64, "f32": L.DTYPE_F32}.get(dtype, dtype)
    return L.opts(dt, L.ASSOC_VITERBI, _KERNEL.get(kernel, kernel), True, stream, workspace_bytes, 0)


def posterior_batch(hmm: HMM, offsets, obs, forced=None, gamma=False, kernel="auto", workspace_bytes=0, path=True,
                    dtype="f64"):
    """CSR sequences (offsets[B+1], flat obs) -> (loglik f64[B], path int32[sum T], gamma
    f64[sum T, N] or None, status u8[B]).  forced[sum T] (optional): -1 free, s >= 0 admits only
    state s at that element (loglik is then the joint with the tags, gamma conditioned on them).
    path=False with gamma=False is the scoring mode (forward pass only; path is None)."""
    offsets = np.ascontiguousarray(offsets, np.int64)
    obs = np.ascontiguousarray(obs, np.int32)
    nseq = offsets.shape[0] - 1
    total = int(offsets[-1]) if nseq >= 0 else 0
    n = hmm.nstates()
    loglik = np.zeros(max(nseq, 0), np.float64)
    status = np.zeros(max(nseq, 0), np.uint8)
    path_out = np.zeros(max(total, 0), np.int32) if path else None
    gamma_out = np.zeros((max(total, 0), n), np.float64) if gamma else None
    o = _opts(kernel, workspace_bytes, dtype=dtype)
    if forced is not None:
        forced = np.ascontiguousarray(forced, np.int32)
        o.forced = forced.ctypes.data
    st = L.lib().cv_posterior_batch(hmm.handle, nseq, _p(offsets), _p(obs), ctypes.byref(o), _p(loglik), _p(path_out),
                                    _p(gamma_out), _p(status))
    if st != L.CV_EINFEASIBLE:
        L.check(st)
    return loglik, path_out, gamma_out, status


def score_batch(hmm: HMM, offsets, obs, forced=None, kernel="auto"):
    """log10 P(observations | model) per sequence (forward pass only) -> (loglik f64[B], status u8[B])."""
    loglik, _, _, status = posterior_batch(hmm, offsets, obs, forced=forced, gamma=False, kernel=kernel, path=False)
    return loglik, status


def posterior_batch_device(hmm: HMM, offsets_dev, obs_dev, loglik_dev, status_dev, path_dev=None, gamma_dev=None,
                           offsets_host=None, forced_dev=None, kernel="auto", stream=None, workspace_bytes=0):
    """Device-pointer variant (ints or objects with data_ptr(), e.g. torch tensors); enqueued on
    `stream`, returns without synchronizing."""
    def ptr(x):
        if x is None:
            return None
        return x.data_ptr() if hasattr(x, "data_ptr") else int(x)

    nseq = (len(offsets_host) if offsets_host is not None else offsets_dev.numel()) - 1
    oh = np.ascontiguousarray(offsets_host, np.int64) if offsets_host is not None else None
    o = _opts(kernel, workspace_bytes, stream)
    if forced_dev is not None:
        o.forced = ptr(forced_dev)
    L.check(L.lib().cv_posterior_batch_device(hmm.handle, nseq, _p(oh), ptr(offsets_dev), ptr(obs_dev),
                                              ctypes.byref(o), ptr(loglik_dev), ptr(path_dev), ptr(gamma_dev),
                                              ptr(status_dev)))
