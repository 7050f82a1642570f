#!/usr/bin/env python3
"""Times cv_sample_batch_device on a config-4-shaped batch (N = 256, V = 1,024, T = 512, 4,096
sequences by default) at R = 1 and R = 8 draws, interleaved with cv_posterior_batch_device in
path mode (no gamma) on the same inputs in the same process: the sampler's bt_ms (sampling plus
scoring) is set against the posterior's backward pass, which this tool does not change.  Inputs
and outputs are resident on the device.  Prints one JSON line.

fwd_ms / bt_ms are the kernels' device events (cv_last_timing), medians over the repeats; wall_ms
is a host clock around enqueue + stream synchronise.  rows_bytes is what one pass over the stored
forward rows reads (elements x NP x 8); rows_tbps = rows_bytes / bt_ms, the rate at which the
sampler consumes them (the dependent A^T row of each step and draw comes from L2 and is not
counted).

    python tools/bench_sample.py [--nseq 4096] [--warmup 2] [--repeats 5] [--kernel auto]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nseq", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--draws", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--kernel", default="auto", choices=["auto", "generic"])
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()

    import torch

    import cviterbi as cv
    from cviterbi import synth

    if not torch.cuda.is_available():
        print("bench_sample: no GPU visible", file=sys.stderr)
        return 2
    nseq = args.nseq
    c = synth.config("c4", nseq)
    n = len(c["pi"])
    np_states = (n + 63) // 64 * 64
    off = c["offsets"]
    total = int(off[-1])
    h = cv.HMM(c["pi"], c["a"], c["b"], c["bdims"], device=args.device)
    dev = torch.device("cuda", args.device)
    d_off, d_obs = torch.from_numpy(off).to(dev), torch.from_numpy(c["obs"]).to(dev)
    d_ll = torch.zeros(nseq, dtype=torch.float64, device=dev)
    d_st = torch.zeros(nseq, dtype=torch.uint8, device=dev)
    rmax = max(args.draws)
    d_path = torch.zeros((rmax, total), dtype=torch.int32, device=dev)
    d_score = torch.zeros((rmax, nseq), dtype=torch.float64, device=dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))

    def posterior():
        cv.posterior_batch_device(h, d_off, d_obs, d_ll, d_st, d_path[0], offsets_host=off, kernel=args.kernel,
                                  stream=stream.cuda_stream)

    def sampler(r):
        def run():
            cv.sample_batch_device(h, d_off, d_obs, r, d_path, d_st, d_score, d_ll, seed=1, offsets_host=off,
                                   kernel=args.kernel, stream=stream.cuda_stream)
        return run

    modes = [("posterior_path", posterior)] + [(f"sample_r{r}", sampler(r)) for r in args.draws]
    times = {name: {"fwd_ms": [], "bt_ms": [], "wall_ms": []} for name, _ in modes}
    for rep in range(args.warmup + args.repeats):
        for name, fn in modes:  # interleaved: every repeat runs every mode once
            t0 = time.perf_counter()
            fn()
            stream.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            t = cv.last_timing(h)
            if rep >= args.warmup:
                times[name]["fwd_ms"].append(t["fwd_ms"])
                times[name]["bt_ms"].append(t["bt_ms"])
                times[name]["wall_ms"].append(wall)
    rows_bytes = total * np_states * 8
    out = {"tool": "bench_sample", "nseq": nseq, "elements": total, "nstates": n, "padded_states": np_states,
           "kernel": args.kernel, "repeats": args.repeats, "rows_bytes": rows_bytes,
           "seq_ok": int((d_st == 0).sum().item())}
    for name, _ in modes:
        med = {k: statistics.median(v) for k, v in times[name].items()}
        out[name] = {k: round(v, 4) for k, v in med.items()}
        out[name]["bt_ms_min_max"] = [round(min(times[name]["bt_ms"]), 4), round(max(times[name]["bt_ms"]), 4)]
        out[name]["rows_tbps"] = round(rows_bytes / (med["bt_ms"] * 1e-3) / 1e12, 4)
    base = out["posterior_path"]["bt_ms"]
    for r in args.draws:
        out[f"sample_r{r}"]["bt_over_posterior_bt"] = round(out[f"sample_r{r}"]["bt_ms"] / base, 4)
    if 1 in args.draws and 8 in args.draws:
        out["r8_over_r1"] = round(out["sample_r8"]["bt_ms"] / out["sample_r1"]["bt_ms"], 4)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
