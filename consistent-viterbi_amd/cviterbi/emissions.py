"""Decode of caller-supplied emission scores on MI355X in exact f64 (cv_decode_emissions*).

For observations that are not symbols of the model's alphabet -- continuous densities, scores
of a neural tagger, back-off rows -- the caller holds E[e][j] = log10 p(observation of element
e | state j) and wants the decode of the handle's (pi, A) under it; the handle's own b is
ignored.  The result is, by definition and bit for bit, decode_batch(dtype="f64") of the
discrete model b = E[:, :N].T with obs = arange(len(E)): same associations, tie rule, statuses
and scores (the same kernels decode rows staged by emis_prepare_f64).  Values may be positive
or -inf; -0.0 reads as +0.0; a NaN or +inf makes its sequence SEQ_BADOBS and leaves every other
sequence alone.  See include/cviterbi.h.

posterior_emissions / score_emissions / posterior_emissions_device (cv_posterior_emissions*)
evaluate the same model: log10 P(observations | model), the state marginals and the posterior
path, as posterior_batch does for the discrete model b = E[:, :N].T, within its error bounds
(not bit for bit: each row is staged as 10^E 2^-k with its own integer k, so scores of any
finite magnitude below 2^40 work).  As in posterior.py, CV_EINFEASIBLE is not raised.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib as L
from .hmm import HMM

_ASSOC = {"viterbi": L.ASSOC_VITERBI, "cp": L.ASSOC_CP, "dp": L.ASSOC_DP, "decode": L.ASSOC_DECODE}
_KERNEL = {"auto": L.KERNEL_AUTO, "trellis": L.KERNEL_TRELLIS, "generic": L.KERNEL_GENERIC,
           "trellis_f64": L.KERNEL_TRELLIS_F64}


def _p(x):
    return x.ctypes.data_as(ctypes.c_void_p) if x is not None else None


def _opts(assoc, kernel, workspace_bytes, stream=None):
    return L.opts(L.DTYPE_F64, _ASSOC.get(assoc, assoc), _KERNEL.get(kernel, kernel), True, stream, workspace_bytes,
                  0)


def _host_emis(hmm, offsets, emis):
    """(offsets int64, emis as the library reads it, ld, nseq, total) of a host call."""
    offsets = np.ascontiguousarray(offsets, np.int64)
    emis = np.asarray(emis)
    if emis.ndim != 2:
        raise ValueError(f"emis must be 2-D [sum T, >= N], got shape {emis.shape}")
    if emis.shape[1] < hmm.nstates():
        raise ValueError(f"emis has {emis.shape[1]} columns, the model {hmm.nstates()} states")
    if (emis.dtype != np.float64 or not emis.flags.aligned or not emis.dtype.isnative
            or (emis.shape[1] > 1 and emis.strides[1] != 8)
            or (emis.shape[0] > 1 and (emis.strides[0] % 8 or emis.strides[0] < 8 * emis.shape[1]))):
        emis = np.ascontiguousarray(emis, np.float64)
    ld = emis.strides[0] // 8 if emis.shape[0] > 1 else emis.shape[1]
    nseq = offsets.shape[0] - 1
    total = int(offsets[-1]) if nseq >= 0 else 0
    if total > emis.shape[0]:
        raise ValueError(f"offsets cover {total} elements, emis has {emis.shape[0]} rows")
    return offsets, emis, ld, nseq, total


def _dev_ld(hmm, emis_dev):
    """The row stride of a device emission array (a checked torch tensor, or a bare pointer)."""
    ld = hmm.nstates()
    if hasattr(emis_dev, "stride") and hasattr(emis_dev, "dim"):
        if emis_dev.dim() != 2:
            raise ValueError(f"emis_dev must be 2-D [sum T, >= N], got {tuple(emis_dev.shape)}")
        if "float64" not in str(emis_dev.dtype):
            raise ValueError(f"emis_dev must be float64, got {emis_dev.dtype}")
        if emis_dev.shape[1] < hmm.nstates():
            raise ValueError(f"emis_dev has {emis_dev.shape[1]} columns, the model {hmm.nstates()} states")
        if emis_dev.shape[1] > 1 and emis_dev.stride(1) != 1:
            raise ValueError("emis_dev must have stride(1) == 1 (rows of consecutive scores)")
        dev = emis_dev.device
        if dev.type != "cuda" or (dev.index is not None and dev.index != hmm.device):
            raise ValueError(f"emis_dev is on {dev}, the handle on device {hmm.device}")
        ld = emis_dev.stride(0) if emis_dev.shape[0] > 1 else emis_dev.shape[1]
    return ld


def _ptr(x):
    if x is None:
        return None
    return x.data_ptr() if hasattr(x, "data_ptr") else int(x)


def decode_emissions(hmm: HMM, offsets, emis, assoc="viterbi", kernel="auto", forced=None, workspace_bytes=0):
    """CSR sequences (offsets[B+1]) with emission scores emis f64[sum T, >= N] (log10) ->
    (path int32[sum T], score f64[B], status u8[B]).  Columns beyond N are ignored; a row stride
    that is not the row length is passed on as it is (no copy), any other layout is copied.
    forced[sum T] (optional, assoc "viterbi"): -1 free, s >= 0 forces state s at that element."""
    offsets, emis, ld, nseq, total = _host_emis(hmm, offsets, emis)
    path = np.zeros(max(total, 0), np.int32)
    score = np.zeros(max(nseq, 0), np.float64)
    status = np.zeros(max(nseq, 0), np.uint8)
    o = _opts(assoc, kernel, workspace_bytes)
    if forced is not None:
        forced = np.ascontiguousarray(forced, np.int32)
        o.forced = forced.ctypes.data
    L.check(L.lib().cv_decode_emissions(hmm.handle, nseq, _p(offsets), _p(emis), int(ld), ctypes.byref(o), _p(path),
                                        _p(score), _p(status)))
    return path, score, status


def decode_emissions_device(hmm: HMM, offsets_dev, emis_dev, path_dev, score_dev, status_dev, offsets_host=None,
                            forced_dev=None, assoc="viterbi", kernel="auto", stream=None, workspace_bytes=0):
    """Device-pointer variant (ints or objects with data_ptr(), e.g. torch tensors): enqueued on
    `stream`, returns without synchronizing.  emis_dev: a 2-D float64 torch tensor on the
    handle's device with at least N columns and stride(1) == 1 (ld = its stride(0): a slice of a
    wider tensor passes without a copy), or a pointer to rows of exactly N doubles."""
    ptr = _ptr
    ld = _dev_ld(hmm, emis_dev)
    nseq = (len(offsets_host) if offsets_host is not None else offsets_dev.numel()) - 1
    oh = np.ascontiguousarray(offsets_host, np.int64) if offsets_host is not None else None
    o = _opts(assoc, kernel, workspace_bytes, stream)
    if forced_dev is not None:
        o.forced = ptr(forced_dev)
    L.check(L.lib().cv_decode_emissions_device(hmm.handle, nseq, _p(oh), ptr(offsets_dev), ptr(emis_dev), int(ld),
                                               ctypes.byref(o), ptr(path_dev), ptr(score_dev), ptr(status_dev)))


def posterior_emissions(hmm: HMM, offsets, emis, forced=None, gamma=False, path=True, kernel="auto",
                        workspace_bytes=0):
    """CSR sequences (offsets[B+1]) with emission scores emis f64[sum T, >= N] (log10, any finite
    magnitude below 2^40, or -inf) -> (loglik f64[B], path int32[sum T] or None, gamma
    f64[sum T, N] or None, status u8[B]), as posterior_batch returns them.  Array handling as in
    decode_emissions.  path=False with gamma=False is the scoring mode (forward pass only)."""
    offsets, emis, ld, nseq, total = _host_emis(hmm, offsets, emis)
    n = hmm.nstates()
    loglik = np.zeros(max(nseq, 0), np.float64)
    status = np.zeros(max(nseq, 0), np.uint8)
    path_out = np.zeros(max(total, 0), np.int32) if path else None
    gamma_out = np.zeros((max(total, 0), n), np.float64) if gamma else None
    o = _opts("viterbi", kernel, workspace_bytes)
    if forced is not None:
        forced = np.ascontiguousarray(forced, np.int32)
        o.forced = forced.ctypes.data
    st = L.lib().cv_posterior_emissions(hmm.handle, nseq, _p(offsets), _p(emis), int(ld), ctypes.byref(o), _p(loglik),
                                        _p(path_out), _p(gamma_out), _p(status))
    if st != L.CV_EINFEASIBLE:
        L.check(st)
    return loglik, path_out, gamma_out, status


def score_emissions(hmm: HMM, offsets, emis, forced=None, kernel="auto"):
    """log10 P(observations | model) per sequence under the scores emis -> (loglik f64[B], status u8[B])."""
    loglik, _, _, status = posterior_emissions(hmm, offsets, emis, forced=forced, gamma=False, path=False,
                                               kernel=kernel)
    return loglik, status


def posterior_emissions_device(hmm: HMM, offsets_dev, emis_dev, loglik_dev, status_dev, path_dev=None,
                               gamma_dev=None, offsets_host=None, forced_dev=None, kernel="auto", stream=None,
                               workspace_bytes=0):
    """Device-pointer variant (ints or objects with data_ptr(), e.g. torch tensors): enqueued on
    `stream`, returns without synchronizing.  emis_dev as in decode_emissions_device."""
    ld = _dev_ld(hmm, emis_dev)
    nseq = (len(offsets_host) if offsets_host is not None else offsets_dev.numel()) - 1
    oh = np.ascontiguousarray(offsets_host, np.int64) if offsets_host is not None else None
    o = _opts("viterbi", kernel, workspace_bytes, stream)
    if forced_dev is not None:
        o.forced = _ptr(forced_dev)
    L.check(L.lib().cv_posterior_emissions_device(hmm.handle, nseq, _p(oh), _ptr(offsets_dev), _ptr(emis_dev),
                                                  int(ld), ctypes.byref(o), _ptr(loglik_dev), _ptr(path_dev),
                                                  _ptr(gamma_dev), _ptr(status_dev)))
