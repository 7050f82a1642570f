"""torch.autograd for the sequence log-likelihood: under emission scores (sequence_loglik,
cv_loglik_grad_emissions*) and of the discrete model with a learnable emission table
(discrete_loglik, cv_expected_counts_model*).

    loglik = cviterbi.autograd.sequence_loglik(emis, offsets, log_pi, log_a)   # [B], log10
    (-loglik.sum()).backward()          # gradients in emis, log_pi and log_a

Marginal-likelihood training of a tagger whose scores feed an HMM / linear-chain layer: the forward
pass is the scoring mode of posterior_emissions (what score_emissions runs), the backward pass one
loglik_grad_emissions_device call with the incoming gradient as the per-sequence weight, both in
the order of torch's current stream (on it; for the legacy default stream on a side stream tied
to it by events), in f64 on the matrix-core kernels.  Everything is log10: for natural-log
scores s and parameters (lp, la) use

    sequence_loglik(s / ln10, offsets, lp / ln10, la / ln10) * ln10        # ln10 = math.log(10)

whose gradients are then the natural-log ones (the two factors cancel).  Differentiable once
(no double backward); f64 only.

    loglik = cviterbi.autograd.discrete_loglik(obs, offsets, log_pi, log_a, log_b)   # [B], log10
    (-loglik.sum()).backward()          # gradients in log_pi, log_a and log_b

is the same for the discrete model: obs int32 [L] on the GPU, log_b [N, V]; the forward pass is the
scoring mode of posterior_batch_device, the backward pass one expected_counts_model_device call.
"""
from __future__ import annotations

import numpy as np

from .counts import expected_counts_model_device
from .emissions import _dev_ld, posterior_emissions_device
from .grad import loglik_grad_emissions_device
from .hmm import HMM
from .posterior import posterior_batch_device

_FN = None
_DFN = None
_SIDE = {}  # device index -> the stream that stands in for torch's legacy default stream


def _ordered(torch, dev, launch):
    """launch(stream handle) in the order of torch's current stream on `dev`.  A stream of its own
    is passed as it is.  The legacy default stream's handle is 0, which the C ABI reads as "the
    handle's own stream": then the work goes to a side stream that waits for the current stream
    and that the current stream waits for."""
    cur = torch.cuda.current_stream(dev)
    if cur.cuda_stream != 0:
        return launch(cur.cuda_stream)
    side = _SIDE.get(dev.index)
    if side is None:
        side = _SIDE[dev.index] = torch.cuda.Stream(device=dev)
    side.wait_stream(cur)
    try:
        return launch(side.cuda_stream)
    finally:
        cur.wait_stream(side)


def _function():
    """The torch.autograd.Function, built at first use (torch is imported only then)."""
    global _FN
    if _FN is not None:
        return _FN
    import torch
    from torch.autograd.function import once_differentiable

    class SequenceLoglik(torch.autograd.Function):
        @staticmethod
        def forward(ctx, emis, log_pi, log_a, call):
            ctx.call = call
            ctx.save_for_backward(emis)
            ctx.param_devices = (log_pi.device, log_a.device)
            nseq = len(call["offsets_host"]) - 1
            loglik = torch.empty(nseq, dtype=torch.float64, device=emis.device)
            status = torch.empty(nseq, dtype=torch.uint8, device=emis.device)
            _ordered(torch, emis.device, lambda stream: posterior_emissions_device(
                call["hmm"], call["offsets_dev"], emis, loglik, status, offsets_host=call["offsets_host"],
                forced_dev=call["forced_dev"], kernel=call["kernel"], stream=stream,
                workspace_bytes=call["workspace_bytes"]))
            ctx.mark_non_differentiable(status)
            return loglik, status

        @staticmethod
        @once_differentiable
        def backward(ctx, grad_loglik, _grad_status):
            call = ctx.call
            (emis,) = ctx.saved_tensors
            hmm = call["hmm"]
            n, dev = hmm.nstates(), emis.device
            off = call["offsets_host"]
            nseq = len(off) - 1
            weight = grad_loglik.to(device=dev, dtype=torch.float64).contiguous()
            egrad = None
            if ctx.needs_input_grad[0]:
                # the call writes the N scores of the elements the offsets cover; everything else is 0
                covered = emis.shape[1] == n and int(off[0]) == 0 and int(off[-1]) == emis.shape[0]
                egrad = (torch.empty if covered else torch.zeros)(emis.shape, dtype=torch.float64, device=dev)
            loglik = torch.empty(nseq, dtype=torch.float64, device=dev)
            status = torch.empty(nseq, dtype=torch.uint8, device=dev)
            pi_grad = torch.empty(n, dtype=torch.float64, device=dev)
            a_grad = torch.empty((n, n), dtype=torch.float64, device=dev)
            _ordered(torch, dev, lambda stream: loglik_grad_emissions_device(
                hmm, call["offsets_dev"], emis, loglik, pi_grad, a_grad, status, weight_dev=weight, emis_grad_dev=egrad,
                offsets_host=off, forced_dev=call["forced_dev"], kernel=call["kernel"], stream=stream,
                workspace_bytes=call["workspace_bytes"]))
            return (egrad, pi_grad.to(ctx.param_devices[0]) if ctx.needs_input_grad[1] else None,
                    a_grad.to(ctx.param_devices[1]) if ctx.needs_input_grad[2] else None, None)

    _FN = SequenceLoglik
    return _FN


def _check(emis, log_pi, log_a):
    import torch

    for name, x in (("emis", emis), ("log_pi", log_pi), ("log_a", log_a)):
        if not isinstance(x, torch.Tensor):
            raise ValueError(f"{name} must be a torch tensor, got {type(x).__name__}")
        if x.dtype != torch.float64:
            raise ValueError(f"{name} must be float64, got {x.dtype}")
    if log_pi.dim() != 1 or log_pi.shape[0] < 1 or tuple(log_a.shape) != (log_pi.shape[0], log_pi.shape[0]):
        raise ValueError(f"log_pi {tuple(log_pi.shape)} and log_a {tuple(log_a.shape)} must be [N] and [N, N]")
    if emis.device.type != "cuda":
        raise ValueError(f"emis must be on a GPU, it is on {emis.device}")
    for name, x in (("log_pi", log_pi), ("log_a", log_a)):
        if x.device.type != "cpu" and x.device != emis.device:
            raise ValueError(f"{name} is on {x.device}, emis on {emis.device}")
    if emis.dim() != 2 or emis.shape[1] < log_pi.shape[0]:
        raise ValueError(f"emis must be [sum T, >= N = {log_pi.shape[0]}], got {tuple(emis.shape)}")
    return torch


def sequence_loglik(emis, offsets, log_pi, log_a, *, forced=None, hmm=None, kernel="auto", workspace_bytes=0,
                    return_status=False):
    """log10 P(o_s | pi, A, emis) of the CSR sequences `offsets` ([B + 1], host integers or a torch
    tensor) -> loglik f64[B] on emis's device, differentiable in emis, log_pi and log_a.

    emis: f64 [L, >= N] on a GPU, stride(1) == 1 (a slice of a wider tensor passes without a copy);
    log_pi [N] and log_a [N, N]: f64 torch tensors, log10 (-inf = impossible), on the CPU or on
    emis's device.  forced (optional, int32 [L]): -1 free, s >= 0 admits only state s.  Wrong
    dtypes (f32 included), devices or shapes raise ValueError before anything is launched.

    hmm=None builds a handle from the current values of log_pi and log_a at each call (with a dummy
    emission table, which the dense entries ignore): one copy of the parameters to the host and one
    N^2 upload per forward.  A caller whose parameters are fixed, or who rebuilds the handle once
    per optimiser step, passes hmm= and so vouches that it holds these values on emis's device;
    the gradients for log_pi and log_a are still returned.

    The gradient of a loss through loglik is loglik_grad_emissions_device with grad_output as the
    weights: emis's in emis's shape (0 in the columns beyond N and the rows outside the offsets),
    log_pi's and log_a's only where they require grad; exactly 0 on every -inf parameter.
    Sequences that are not SEQ_OK (empty, a NaN / +inf score, likelihood 0) get the loglik that
    score_emissions gives them and a zero gradient, whatever grad_output holds for them;
    return_status=True also returns their statuses (u8 [B], on the device)."""
    torch = _check(emis, log_pi, log_a)
    n = log_pi.shape[0]
    if torch.is_tensor(offsets):
        offsets = offsets.detach().cpu().numpy()
    off = np.array(offsets, np.int64)  # a copy: the call keeps it until backward
    if off.ndim != 1 or off.shape[0] < 1 or np.any(np.diff(off) < 0) or off[0] < 0 or off[-1] > emis.shape[0]:
        raise ValueError(f"offsets must be non-decreasing [B + 1] within emis's {emis.shape[0]} rows")
    forced_dev = None
    if forced is not None:
        forced_dev = torch.as_tensor(forced).to(device=emis.device, dtype=torch.int32).contiguous()
        if forced_dev.dim() != 1 or forced_dev.shape[0] < int(off[-1]):
            raise ValueError(f"forced must be [sum T], got {tuple(forced_dev.shape)}")
    if hmm is None:
        dummy_b = np.log10(np.full((n, 2), 0.5))
        hmm = HMM(log_pi.detach().cpu().numpy(), log_a.detach().cpu().numpy(), dummy_b, device=emis.device.index or 0)
    elif hmm.nstates() != n:
        raise ValueError(f"hmm has {hmm.nstates()} states, log_pi {n}")
    _dev_ld(hmm, emis)  # stride and device against the handle's
    call = dict(hmm=hmm, offsets_host=off, offsets_dev=torch.from_numpy(off).to(emis.device), forced_dev=forced_dev,
                kernel=kernel, workspace_bytes=workspace_bytes)
    loglik, status = _function().apply(emis, log_pi, log_a, call)
    return (loglik, status) if return_status else loglik


def _discrete_function():
    """The torch.autograd.Function of discrete_loglik, built at first use."""
    global _DFN
    if _DFN is not None:
        return _DFN
    import torch
    from torch.autograd.function import once_differentiable

    class DiscreteLoglik(torch.autograd.Function):
        @staticmethod
        def forward(ctx, log_pi, log_a, log_b, call):
            ctx.call = call
            ctx.param_devices = (log_pi.device, log_a.device, log_b.device)
            obs = call["obs"]
            nseq = len(call["offsets_host"]) - 1
            loglik = torch.empty(nseq, dtype=torch.float64, device=obs.device)
            status = torch.empty(nseq, dtype=torch.uint8, device=obs.device)
            _ordered(torch, obs.device, lambda stream: posterior_batch_device(
                call["hmm"], call["offsets_dev"], obs, loglik, status, offsets_host=call["offsets_host"],
                forced_dev=call["forced_dev"], kernel=call["kernel"], stream=stream,
                workspace_bytes=call["workspace_bytes"]))
            ctx.mark_non_differentiable(status)
            return loglik, status

        @staticmethod
        @once_differentiable
        def backward(ctx, grad_loglik, _grad_status):
            call = ctx.call
            hmm, obs = call["hmm"], call["obs"]
            n, v, dev = hmm.nstates(), hmm.nobs(), obs.device
            off = call["offsets_host"]
            nseq = len(off) - 1
            weight = grad_loglik.to(device=dev, dtype=torch.float64).contiguous()
            loglik = torch.empty(nseq, dtype=torch.float64, device=dev)
            status = torch.empty(nseq, dtype=torch.uint8, device=dev)
            pi_grad = torch.empty(n, dtype=torch.float64, device=dev)
            a_grad = torch.empty((n, n), dtype=torch.float64, device=dev)
            b_grad = torch.empty((n, v), dtype=torch.float64, device=dev)
            _ordered(torch, dev, lambda stream: expected_counts_model_device(
                hmm, call["offsets_dev"], obs, loglik, pi_grad, a_grad, b_grad, status, weight_dev=weight,
                offsets_host=off, forced_dev=call["forced_dev"], kernel=call["kernel"], stream=stream,
                workspace_bytes=call["workspace_bytes"]))
            grads = (pi_grad, a_grad, b_grad)
            return tuple(g.to(d) if need else None
                         for g, d, need in zip(grads, ctx.param_devices, ctx.needs_input_grad[:3])) + (None,)

    _DFN = DiscreteLoglik
    return _DFN


def _check_discrete(obs, log_pi, log_a, log_b):
    import torch

    for name, x in (("obs", obs), ("log_pi", log_pi), ("log_a", log_a), ("log_b", log_b)):
        if not isinstance(x, torch.Tensor):
            raise ValueError(f"{name} must be a torch tensor, got {type(x).__name__}")
    if obs.dtype != torch.int32:
        raise ValueError(f"obs must be int32, got {obs.dtype}")
    for name, x in (("log_pi", log_pi), ("log_a", log_a), ("log_b", log_b)):
        if x.dtype != torch.float64:
            raise ValueError(f"{name} must be float64, got {x.dtype}")
    if log_pi.dim() != 1 or log_pi.shape[0] < 1 or tuple(log_a.shape) != (log_pi.shape[0], log_pi.shape[0]):
        raise ValueError(f"log_pi {tuple(log_pi.shape)} and log_a {tuple(log_a.shape)} must be [N] and [N, N]")
    if log_b.dim() != 2 or log_b.shape[0] != log_pi.shape[0] or log_b.shape[1] < 1:
        raise ValueError(f"log_b must be [N = {log_pi.shape[0]}, V >= 1], got {tuple(log_b.shape)}")
    if obs.device.type != "cuda":
        raise ValueError(f"obs must be on a GPU, it is on {obs.device}")
    for name, x in (("log_pi", log_pi), ("log_a", log_a), ("log_b", log_b)):
        if x.device.type != "cpu" and x.device != obs.device:
            raise ValueError(f"{name} is on {x.device}, obs on {obs.device}")
    if obs.dim() != 1 or not obs.is_contiguous():
        raise ValueError(f"obs must be a contiguous [sum T] vector, got {tuple(obs.shape)}")
    return torch


def discrete_loglik(obs, offsets, log_pi, log_a, log_b, *, forced=None, hmm=None, kernel="auto", workspace_bytes=0,
                    return_status=False):
    """log10 P(o_s | pi, A, b) of the CSR sequences `offsets` ([B + 1], host integers or a torch
    tensor) over the observation indices obs -> loglik f64[B] on obs's device, differentiable in
    log_pi, log_a and log_b.

    obs: int32 [L] on a GPU, contiguous, values in [0, V) (a sequence with a value outside is
    SEQ_BADOBS); log_pi [N], log_a [N, N] and log_b [N, V]: f64 torch tensors, log10 (-inf =
    impossible), on the CPU or on obs's device.  forced (optional, int32 [L]): -1 free, s >= 0
    admits only state s.  Wrong dtypes, devices or shapes raise ValueError before anything is
    launched.

    hmm=None builds a handle from the current values of the three parameters at each call; a
    caller who rebuilds the handle once per optimiser step passes hmm= and so vouches that it
    holds these values on obs's device; the gradients are still returned.

    The gradient of a loss through loglik is one expected_counts_model_device call with
    grad_output as the weights: returned for log_pi, log_a and log_b only where they require grad;
    exactly 0 on every -inf parameter, and in log_b for every value no OK sequence observes.
    Sequences that are not SEQ_OK get the loglik that score_batch gives them and a zero gradient,
    whatever grad_output holds for them; return_status=True also returns their statuses."""
    torch = _check_discrete(obs, log_pi, log_a, log_b)
    n, v = log_b.shape
    if torch.is_tensor(offsets):
        offsets = offsets.detach().cpu().numpy()
    off = np.array(offsets, np.int64)  # a copy: the call keeps it until backward
    if off.ndim != 1 or off.shape[0] < 1 or np.any(np.diff(off) < 0) or off[0] < 0 or off[-1] > obs.shape[0]:
        raise ValueError(f"offsets must be non-decreasing [B + 1] within obs's {obs.shape[0]} elements")
    forced_dev = None
    if forced is not None:
        forced_dev = torch.as_tensor(forced).to(device=obs.device, dtype=torch.int32).contiguous()
        if forced_dev.dim() != 1 or forced_dev.shape[0] < int(off[-1]):
            raise ValueError(f"forced must be [sum T], got {tuple(forced_dev.shape)}")
    if hmm is None:
        hmm = HMM(log_pi.detach().cpu().numpy(), log_a.detach().cpu().numpy(), log_b.detach().cpu().numpy(),
                  device=obs.device.index or 0)
    elif hmm.nstates() != n or hmm.nobs() != v:
        raise ValueError(f"hmm has {hmm.nstates()} states and {hmm.nobs()} observation values, log_b [{n}, {v}]")
    call = dict(hmm=hmm, obs=obs, offsets_host=off, offsets_dev=torch.from_numpy(off).to(obs.device),
                forced_dev=forced_dev, kernel=kernel, workspace_bytes=workspace_bytes)
    loglik, status = _discrete_function().apply(log_pi, log_a, log_b, call)
    return (loglik, status) if return_status else loglik
