"""K-best (list) Viterbi decoding on MI355X in exact f64 (cv_kbest_batch*).

The k best paths of every sequence under decode_batch's "viterbi" association in f64, with
their scores: rank 0 is decode_batch(dtype="f64")'s path and score bit for bit, every score is
the f64 fold along its path, and the first k' ranks of a k-best call are the k'-best call's
result.  See include/cviterbi.h for the recurrence and its tie rules.

A sequence with fewer than k paths of finite score reports how many it has in count; its unused
ranks hold score -inf and path -1.  A sequence with none has status SEQ_INFEASIBLE and count 0;
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
_ASSOC = {"viterbi": L.ASSOC_VITERBI, "cp": L.ASSOC_CP, "dp": L.ASSOC_DP, "decode": L.ASSOC_DECODE}


def _p(x):
    return x.ctypes.data_as(ctypes.c_void_p) if x is not None else None


def _opts(kernel, workspace_bytes, stream=None, dtype="f64", assoc="viterbi"):
    dt = {"f64": L.DTYPE_F64, "f32": L.DTYPE_F32}.get(dtype, dtype)
    return L.opts(dt, _ASSOC.get(assoc, assoc), _KERNEL.get(kernel, kernel), True, stream, workspace_bytes, 0)


def kbest_batch(hmm: HMM, offsets, obs, k, forced=None, kernel="auto", workspace_bytes=0, dtype="f64",
                assoc="viterbi"):
    """CSR sequences (offsets[B+1], flat obs) -> (paths int32[k, sum T], scores f64[B, k], count
    int32[B], status u8[B]).  paths[r] is rank r's path array in decode_batch's layout.
    forced[sum T] (optional): -1 free, s >= 0 admits only state s at that element."""
    offsets = np.ascontiguousarray(offsets, np.int64)
    obs = np.ascontiguousarray(obs, np.int32)
    k = int(k)
    nseq = offsets.shape[0] - 1
    total = int(offsets[-1]) if nseq >= 0 else 0
    rows = min(max(k, 0), 16)  # a bad k is reported by the library; no buffer is sized by it
    paths = np.zeros((rows, max(total, 0)), np.int32)
    scores = np.zeros((max(nseq, 0), rows), np.float64)
    count = np.zeros(max(nseq, 0), np.int32)
    status = np.zeros(max(nseq, 0), np.uint8)
    o = _opts(kernel, workspace_bytes, dtype=dtype, assoc=assoc)
    if forced is not None:
        forced = np.ascontiguousarray(forced, np.int32)
        o.forced = forced.ctypes.data
    st = L.lib().cv_kbest_batch(hmm.handle, nseq, _p(offsets), _p(obs), k, ctypes.byref(o), _p(paths), _p(scores),
                                _p(count), _p(status))
    if st != L.CV_EINFEASIBLE:
        L.check(st)
    return paths, scores, count, status


def kbest_batch_device(hmm: HMM, offsets_dev, obs_dev, k, path_dev, score_dev, count_dev, status_dev,
                       offsets_host=None, forced_dev=None, kernel="auto", stream=None, workspace_bytes=0):
    """Device-pointer variant (ints or objects with data_ptr(), e.g. torch tensors): path_dev
    int32[k, sum T], score_dev f64[B, k], count_dev int32[B], status_dev u8[B]; enqueued on
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
    L.check(L.lib().cv_kbest_batch_device(hmm.handle, nseq, _p(oh), ptr(offsets_dev), ptr(obs_dev), int(k),
                                          ctypes.byref(o), ptr(path_dev), ptr(score_dev), ptr(count_dev),
                                          ptr(status_dev)))
