#!/usr/bin/env python3
"""Times cv_loglik_grad_emissions_device (weights and the gradient rows of E requested) against
cv_expected_counts_emissions_device with gamma requested -- the same passes and the same bytes,
the new call one product per stored value more -- on device-resident inputs, in one process:

  (a) cv_expected_counts_emissions_device, gamma     the yardstick
  (b) cv_loglik_grad_emissions_device, emis_grad     signed random weights
  (c) cviterbi.autograd.sequence_loglik              forward (scoring mode) + backward (= b), hmm given

(a) and (b) alternate call by call; after `--warmup` rounds each of `--rounds` rounds records the
library's own device events of one call of each (cv_last_timing: fwd_ms the forward pass with
staging, bt_ms the backward pass plus the GEMM, fold and final kernels).  (c) is timed by torch
events around forward + backward on the current stream, beside the library's events of its two
calls.  Reported: median, min and max per call.  Prints one line per round and one JSON line.

    python tools/bench_loglik_grad.py [--nstates 256] [--nseq 4096] [--T 512] [--rounds 7] [--warmup 2]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "consistent-viterbi_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nstates", type=int, default=256)
    ap.add_argument("--nseq", type=int, default=4096)
    ap.add_argument("--T", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--kernel", default="auto")
    ap.add_argument("--workspace-bytes", type=int, default=0)
    args = ap.parse_args()

    import numpy as np
    import torch

    import cviterbi as cv
    from cviterbi import synth

    if not torch.cuda.is_available():
        print("bench_loglik_grad: no GPU visible", file=sys.stderr)
        return 2
    n, nseq, T = args.nstates, args.nseq, args.T
    pi, a, b0 = synth.random_hmm(n, 2, seed=20261021)
    off = np.arange(nseq + 1, dtype=np.int64) * T
    total = int(off[-1])
    h = cv.HMM(pi, a, b0, device=args.device)
    dev = torch.device("cuda", args.device)
    gen = torch.Generator(device=dev).manual_seed(20261021)
    E = torch.randn((total, n), dtype=torch.float64, device=dev, generator=gen) * 1.5
    w = torch.randn(nseq, dtype=torch.float64, device=dev, generator=gen)
    d_off = torch.from_numpy(off).to(dev)
    ll = {k: torch.zeros(nseq, dtype=torch.float64, device=dev) for k in "ab"}
    st = {k: torch.zeros(nseq, dtype=torch.uint8, device=dev) for k in "ab"}
    pc = {k: torch.zeros(n, dtype=torch.float64, device=dev) for k in "ab"}
    ac = {k: torch.zeros((n, n), dtype=torch.float64, device=dev) for k in "ab"}
    rows = torch.zeros((total, n), dtype=torch.float64, device=dev)  # gamma of (a), emis_grad of (b): both overwrite it
    kw = dict(offsets_host=off, kernel=args.kernel, workspace_bytes=args.workspace_bytes)

    def call_a():
        cv.expected_counts_emissions_device(h, d_off, E, ll["a"], pc["a"], ac["a"], st["a"], gamma_dev=rows,
                                            stream=torch.cuda.current_stream(dev).cuda_stream, **kw)
        return cv.last_timing(h)

    def call_b():
        cv.loglik_grad_emissions_device(h, d_off, E, ll["b"], pc["b"], ac["b"], st["b"], weight_dev=w, emis_grad_dev=rows,
                                        stream=torch.cuda.current_stream(dev).cuda_stream, **kw)
        return cv.last_timing(h)

    lp, la = torch.from_numpy(pi), torch.from_numpy(a)
    Eg = E.requires_grad_(True)

    def call_c():
        Eg.grad = None
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        loglik = cv.autograd.sequence_loglik(Eg, off, lp, la, hmm=h, kernel=args.kernel, workspace_bytes=args.workspace_bytes)
        e1.record()
        loglik.backward(w)
        e2.record()
        torch.cuda.synchronize(dev)
        t = cv.last_timing(h)  # the backward call's
        return dict(total_ms=e0.elapsed_time(e2), fwd_ms=e0.elapsed_time(e1), bt_ms=e1.elapsed_time(e2),
                    backward_call_ms=t["total_ms"])

    series = {k: [] for k in ("a_counts_gamma", "b_loglik_grad", "c_autograd")}
    stream = torch.cuda.Stream(device=dev)  # every call, torch's own kernels included, on this one stream
    stream.wait_stream(torch.cuda.current_stream(dev))
    torch.cuda.synchronize(dev)
    for rnd in range(-args.warmup, args.rounds):
        with torch.cuda.stream(stream):
            ta, tb, tc = call_a(), call_b(), call_c()
        if rnd < 0:
            continue
        series["a_counts_gamma"].append(ta)
        series["b_loglik_grad"].append(tb)
        series["c_autograd"].append(tc)
        print(f"round {rnd}: counts+gamma {ta['total_ms']:.3f} ms (fwd {ta['fwd_ms']:.3f}, bwd {ta['bt_ms']:.3f}) | "
              f"loglik_grad {tb['total_ms']:.3f} ms (fwd {tb['fwd_ms']:.3f}, bwd {tb['bt_ms']:.3f}) | "
              f"autograd fwd+bwd {tc['total_ms']:.3f} ms (fwd {tc['fwd_ms']:.3f}, bwd {tc['bt_ms']:.3f}, "
              f"its backward call {tc['backward_call_ms']:.3f})", flush=True)

    def stats(xs, key):
        v = [x[key] for x in xs]
        return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))

    out = dict(tool="bench_loglik_grad", nstates=n, nseq=nseq, T=T, rounds=args.rounds, warmup=args.warmup,
               kernel=args.kernel, padded_states=series["b_loglik_grad"][0]["padded_states"],
               launches=series["b_loglik_grad"][0]["launches"])
    for name, xs in series.items():
        out[name] = {key: stats(xs, key) for key in ("total_ms", "fwd_ms", "bt_ms")}
    out["c_autograd"]["backward_call_ms"] = stats(series["c_autograd"], "backward_call_ms")
    ya, yb = out["a_counts_gamma"]["total_ms"], out["b_loglik_grad"]["total_ms"]
    out["loglik_grad_over_counts"] = round(yb["median"] / ya["median"], 4)
    out["inside_the_yardsticks_spread"] = bool(yb["median"] <= ya["max"])  # no slower than the yardstick's slowest round
    out["autograd_over_loglik_grad"] = round(out["c_autograd"]["total_ms"]["median"] / yb["median"], 4)
    torch.cuda.synchronize(dev)
    out["statuses_ok"] = [int((st[k] == 0).sum().item()) for k in "ab"]
    out["logliks_equal"] = bool(torch.equal(ll["a"], ll["b"]))
    out["autograd_grad_equals_raw"] = bool(torch.equal(Eg.grad, rows))  # (b) ran last into rows before (c)
    out["device_bytes_peak"] = cv.device_memory()["peak"]
    print(json.dumps(out))
    assert out["logliks_equal"], "the gradient call's logliks differ from the counts call's"
    return 0


if __name__ == "__main__":
    sys.exit(main())
