#!/usr/bin/env python3
"""Times cv_posterior_batch_device on a config-4-shaped batch (N = 256, V = 1,024, T = 512,
65,536 sequences; --small: 4,096 sequences): scoring mode (forward pass only: loglik) and path
mode (forward rows + backward pass: loglik and the posterior-decoding path).  Inputs and
outputs are resident on the device.  Prints one JSON line.

A call's time is a host clock around enqueue + stream synchronise (what a caller waits for);
fwd_ms / bt_ms are the kernels' device events (cv_last_timing).  FMA/s counts the N^2 FMAs per
element of each pass (the products X . A); frac_f64_matrix is that rate over the MI355X nominal
f64 matrix rate (78.6 TFLOP/s = 3.93e13 FMA/s).

    python tools/bench_posterior.py [--small] [--warmup 2] [--repeats 5]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "consistent-viterbi_amd"))

NOMINAL_F64_MATRIX_FMAS = 78.6e12 / 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="4,096 sequences instead of 65,536")
    ap.add_argument("--nseq", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kernel", default="auto", choices=["auto", "generic"])
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()

    import numpy as np
    import torch

    import cviterbi as cv
    from cviterbi import synth

    if not torch.cuda.is_available():
        print("bench_posterior: no GPU visible", file=sys.stderr)
        return 2
    nseq = args.nseq or (4096 if args.small else 65536)
    c = synth.config("c4", nseq)
    n = len(c["pi"])
    off = c["offsets"]
    total = int(off[-1])
    h = cv.HMM(c["pi"], c["a"], c["b"], c["bdims"], device=args.device)
    dev = torch.device("cuda", args.device)
    d_off, d_obs = torch.from_numpy(off).to(dev), torch.from_numpy(c["obs"]).to(dev)
    d_ll = torch.zeros(nseq, dtype=torch.float64, device=dev)
    d_st = torch.zeros(nseq, dtype=torch.uint8, device=dev)
    d_path = torch.zeros(total, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))

    def run(path):
        t0 = time.perf_counter()
        cv.posterior_batch_device(h, d_off, d_obs, d_ll, d_st, d_path if path else None, None, offsets_host=off,
                                  kernel=args.kernel, stream=stream.cuda_stream)
        stream.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        return ms, cv.last_timing(h)

    out = dict(tool="bench_posterior", nstates=n, nseq=nseq, T=int(off[1] - off[0]), kernel=args.kernel,
               warmup=args.warmup, repeats=args.repeats)
    fmas = float(total) * n * n
    for mode, path in (("score", False), ("path", True)):
        for _ in range(args.warmup):
            run(path)
        calls, fwd, bwd = [], [], []
        for _ in range(args.repeats):
            ms, t = run(path)
            calls.append(ms)
            fwd.append(t["fwd_ms"])
            bwd.append(t["bt_ms"])
        med = statistics.median(calls)
        out[f"{mode}_ms_per_call"] = round(med, 3)
        out[f"{mode}_ms_min"] = round(min(calls), 3)
        out[f"{mode}_ms_max"] = round(max(calls), 3)
        out[f"{mode}_fwd_ms"] = round(statistics.median(fwd), 3)
        out[f"{mode}_bwd_ms"] = round(statistics.median(bwd), 3)
        out[f"{mode}_launches"] = t["launches"]
        passes = 2 if path else 1
        out[f"{mode}_fma_per_s"] = float(f"{passes * fmas / (med * 1e-3):.4g}")
        out[f"{mode}_frac_f64_matrix"] = round(passes * fmas / (med * 1e-3) / NOMINAL_F64_MATRIX_FMAS, 4)
    ll = d_ll.cpu().numpy()
    st = d_st.cpu().numpy()
    out["status_ok"] = int((st == 0).sum())
    out["loglik_mean"] = float(np.mean(ll[st == 0])) if (st == 0).any() else None
    out["device_bytes_peak"] = cv.device_memory()["peak"]
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
