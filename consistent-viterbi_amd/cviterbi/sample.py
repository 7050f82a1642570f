"""Posterior path sampling on MI355X (cv_sample_batch*): whole paths drawn from
P(path | observations, tags) by forward filtering, backward sampling, on the model as
posterior_batch reads it.  f64; see include/cviterbi.h for the pick rule, the generator and the
accuracy contract.

A draw depends on (seed, seq_base + s, r) and the sequence alone: the first R' planes of an
R-draw call are the R'-draw call, and sequence s of a batch is the same sequence sampled alone
with seq_base = s.  Every sampled path has a finite score.

As in posterior_batch, a sequence of likelihood 0 has status SEQ_INFEASIBLE (paths -1, scores
-inf) and the wrappers do not raise for it: the per-sequence statuses say which it was.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib as L
from .hmm import HMM
from .posterior import _opts, _p

MAX_DRAWS = 64
_G = 0x9E3779B97F4A7C15
_STEP = 0xD1B54A32D192ED03


def _mix(z):
    z = z ^ (z >> np.uint64(30))
    z = z * np.uint64(0xBF58476D1CE4E5B9)
    z = z ^ (z >> np.uint64(27))
    z = z * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _u64(x):
    """x mod 2^64 as numpy uint64 (arrays of any integer dtype, or Python integers of any size)."""
    if isinstance(x, (int, np.integer)):
        return np.uint64(int(x) & 0xFFFFFFFFFFFFFFFF)
    x = np.asarray(x)
    return x.astype(np.int64).astype(np.uint64) if x.dtype.kind == "i" else x.astype(np.uint64)


def uniform(seed, S, r, t):
    """The generator of cv_sample_batch in numpy uint64: u(seed, S, r, t) in [0, 1) as f64;
    S = seq_base + s, r the draw, t the position in the sequence.  Broadcasts over arrays."""
    with np.errstate(over="ignore"):
        g = np.uint64(_G)
        k = _mix(_u64(seed) + g)
        k = _mix(k ^ _u64(S))
        k = _mix(k + g * (_u64(r) + np.uint64(1)))
        z = _mix(k ^ (_u64(t) * np.uint64(_STEP)))
    return (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def sample_batch(hmm: HMM, offsets, obs, draws, seed=0, seq_base=0, forced=None, kernel="auto", workspace_bytes=0,
                 scores=True):
    """CSR sequences (offsets[B+1], flat obs) -> (paths int32[R, sum T], scores f64[R, B] or None,
    loglik f64[B], status u8[B]): R = draws paths per sequence, scores[r, s] the f64 log10 fold
    along paths[r] of sequence s (what kbest_batch reports for that path)."""
    offsets = np.ascontiguousarray(offsets, np.int64)
    obs = np.ascontiguousarray(obs, np.int32)
    nseq = offsets.shape[0] - 1
    total = int(offsets[-1]) if nseq >= 0 else 0
    R = int(draws)
    rows = min(max(R, 0), MAX_DRAWS)
    paths = np.zeros((rows, max(total, 0)), np.int32)
    score = np.zeros((rows, max(nseq, 0)), np.float64) if scores else None
    loglik = np.zeros(max(nseq, 0), np.float64)
    status = np.zeros(max(nseq, 0), np.uint8)
    o = _opts(kernel, workspace_bytes)
    if forced is not None:
        forced = np.ascontiguousarray(forced, np.int32)
        o.forced = forced.ctypes.data
    st = L.lib().cv_sample_batch(hmm.handle, nseq, _p(offsets), _p(obs), R, int(seed) & 0xFFFFFFFFFFFFFFFF,
                                 int(seq_base), ctypes.byref(o), _p(paths), _p(score), _p(loglik), _p(status))
    if st != L.CV_EINFEASIBLE:
        L.check(st)
    return paths, score, loglik, status


def sample_batch_device(hmm: HMM, offsets_dev, obs_dev, draws, path_dev, status_dev, score_dev=None, loglik_dev=None,
                        seed=0, seq_base=0, offsets_host=None, forced_dev=None, kernel="auto", stream=None,
                        workspace_bytes=0):
    """Device-pointer variant (ints or objects with data_ptr(), e.g. torch tensors): path_dev
    int32[R, sum T], score_dev f64[R, B] (optional), loglik_dev f64[B] (optional), status_dev
    u8[B]; enqueued on `stream`, returns without synchronizing."""
    def ptr(x):
        if x is None:
            return None
        return x.data_ptr() if hasattr(x, "data_ptr") else int(x)

    nseq = (len(offsets_host) if offsets_host is not None else offsets_dev.numel()) - 1
    oh = np.ascontiguousarray(offsets_host, np.int64) if offsets_host is not None else None
    o = _opts(kernel, workspace_bytes, stream)
    if forced_dev is not None:
        o.forced = ptr(forced_dev)
    L.check(L.lib().cv_sample_batch_device(hmm.handle, nseq, _p(oh), ptr(offsets_dev), ptr(obs_dev), int(draws),
                                           int(seed) & 0xFFFFFFFFFFFFFFFF, int(seq_base), ctypes.byref(o),
                                           ptr(path_dev), ptr(score_dev), ptr(loglik_dev), ptr(status_dev)))
