#!/usr/bin/env python3
"""Times cv_posterior_emissions_device against the discrete evaluation of the same problem and
against a plain device copy of the score matrix, in one session, on device-resident inputs:

  (a) cv_posterior_batch_device on observations obs of a model with table b, in scoring mode
      (forward pass only) and in path mode (forward rows stored, backward pass);
  (b) cv_posterior_emissions_device on E = b^T[obs], gathered once beforehand with torch -- the
      same problem, so its log-likelihoods agree with (a)'s within the error bounds (the largest
      difference is reported) and its statuses are equal (asserted);
  (c) torch's device-to-device copy_ of a [sum T, N] f64 tensor: the bytes the staging kernel
      emis_prepare_lin_f64 has to move at the least.

Each is timed with torch events around `--calls` back-to-back calls after `--warmup` calls; the
kernels' own device events (cv_last_timing) split (a) and (b) into forward and backward -- (b)'s
forward span includes the staging kernel.  The staging kernel's own time comes from a separate
rocprofv3 --kernel-trace --stats run of this program.  Prints one JSON line.

    python tools/bench_posterior_emissions.py [--nstates 256] [--nseq 4096] [--T 512] [--calls 10] [--warmup 3]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "consistent-viterbi_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nstates", type=int, default=256)
    ap.add_argument("--nobs", type=int, default=1024)
    ap.add_argument("--nseq", type=int, default=4096)
    ap.add_argument("--T", type=int, default=512)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--kernel", default="auto")
    ap.add_argument("--workspace-bytes", type=int, default=0)
    args = ap.parse_args()

    import numpy as np
    import torch

    import cviterbi as cv
    from cviterbi import synth

    if not torch.cuda.is_available():
        print("bench_posterior_emissions: no GPU visible", file=sys.stderr)
        return 2
    n, v, nseq, T = args.nstates, args.nobs, args.nseq, args.T
    pi, a, b = synth.random_hmm(n, v, seed=20261020)
    off = np.arange(nseq + 1, dtype=np.int64) * T
    total = int(off[-1])
    obs = synth.iid_obs(v, total, seed=20261020)
    h = cv.HMM(pi, a, b, device=args.device)
    dev = torch.device("cuda", args.device)
    d_off, d_obs = torch.from_numpy(off).to(dev), torch.from_numpy(obs).to(dev)
    E = torch.from_numpy(np.ascontiguousarray(b.T)).to(dev)[d_obs.long()]  # [sum T, N], ld = N
    E2 = torch.empty_like(E)
    outs = {k: (torch.zeros(nseq, dtype=torch.float64, device=dev), torch.zeros(nseq, dtype=torch.uint8, device=dev),
                torch.zeros(total, dtype=torch.int32, device=dev)) for k in "ab"}
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    kw = dict(offsets_host=off, kernel=args.kernel, stream=stream.cuda_stream, workspace_bytes=args.workspace_bytes)

    def discrete(path):
        ll, st, p = outs["a"]
        return lambda: cv.posterior_batch_device(h, d_off, d_obs, ll, st, p if path else None, **kw)

    def dense(path):
        ll, st, p = outs["b"]
        return lambda: cv.posterior_emissions_device(h, d_off, E, ll, st, p if path else None, **kw)

    def copy():
        E2.copy_(E)

    def timed(fn, timing):
        with torch.cuda.stream(stream):
            for _ in range(args.warmup):
                fn()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            for _ in range(args.calls):
                fn()
            t1.record(stream)
        stream.synchronize()
        r = dict(ms_per_call=round(t0.elapsed_time(t1) / args.calls, 4))
        if timing:
            t = cv.last_timing(h)
            r.update(fwd_ms=round(t["fwd_ms"], 4), bt_ms=round(t["bt_ms"], 4), total_ms=round(t["total_ms"], 4),
                     launches=t["launches"], kernel=t["kernel"], padded_states=t["padded_states"])
        return r

    out = dict(tool="bench_posterior_emissions", nstates=n, nobs=v, nseq=nseq, T=T, calls=args.calls,
               warmup=args.warmup, workspace_bytes=args.workspace_bytes)
    # interleaved twice, so a drift of the clocks shows as a difference between the rounds
    for rnd in (0, 1):
        for mode, path in (("score", False), ("path", True)):
            out[f"a_discrete_{mode}_{rnd}"] = timed(discrete(path), True)
            out[f"b_emissions_{mode}_{rnd}"] = timed(dense(path), True)
        out[f"c_copy_{rnd}"] = timed(copy, False)
    la, lb = outs["a"][0], outs["b"][0]
    out["statuses_equal"] = bool(torch.equal(outs["a"][1], outs["b"][1]))
    out["status_ok"] = int((outs["b"][1] == 0).sum().item())
    out["paths_equal_fraction"] = round(float((outs["a"][2] == outs["b"][2]).double().mean().item()), 6)
    out["max_abs_loglik_difference"] = float((la - lb).abs().max().item())
    best = lambda key: min(out[f"{key}_{r}"]["ms_per_call"] for r in (0, 1))
    Cms = best("c_copy")
    P = out["b_emissions_score_0"]["padded_states"] or n
    moved = 8.0 * (2 * n + P) * total  # two reads of ld = N (the second from cache at best), P doubles written
    for mode in ("score", "path"):
        out[f"b_minus_a_{mode}_ms"] = round(best(f"b_emissions_{mode}") - best(f"a_discrete_{mode}"), 4)
        stage = min(out[f"b_emissions_{mode}_{r}"]["fwd_ms"] - out[f"a_discrete_{mode}_{r}"]["fwd_ms"] for r in (0, 1))
        out[f"staging_ms_from_fwd_spans_{mode}"] = round(stage, 4)
        out[f"staging_over_copy_{mode}"] = round(stage / Cms, 3)
    out["copy_gbps"] = round(2 * 8.0 * n * total / Cms / 1e6, 1)
    out["staging_bytes_moved"] = moved
    out["device_bytes_peak"] = cv.device_memory()["peak"]
    print(json.dumps(out))
    assert out["statuses_equal"], "posterior_emissions_device statuses differ from the discrete evaluation"
    return 0


if __name__ == "__main__":
    sys.exit(main())
