#!/usr/bin/env python3
"""Times cv_expected_counts*_device (gamma not requested) against the posterior path call on the
same input, in one session, on device-resident inputs:

  (a) cv_posterior_batch_device, path only           (b) cv_expected_counts_device
  (c) cv_posterior_emissions_device, path only       (d) cv_expected_counts_emissions_device
      on E = b^T[obs], gathered once beforehand with torch -- the same problem as (a) / (b)

Each is timed by the library's own device events summed over `--calls` back-to-back calls after
`--warmup` calls (cv_timing_begin / cv_timing_end: fwd_ms the forward pass with staging, bt_ms the
backward pass plus, for the counts, the GEMM, fold and final kernels), interleaved twice so a
drift of the clocks shows as a difference between the rounds.  The split of bt_ms by kernel comes
from a separate rocprofv3 --kernel-trace --stats run of this program.  Prints one JSON line.

    python tools/bench_counts.py [--nstates 256] [--nseq 4096] [--T 512] [--calls 10] [--warmup 3]
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
    ap.add_argument("--xi-part-rows", type=int, default=None, help="tuning key xi_part_rows (default: by rule)")
    args = ap.parse_args()

    import numpy as np
    import torch

    import cviterbi as cv
    from cviterbi import synth

    if not torch.cuda.is_available():
        print("bench_counts: no GPU visible", file=sys.stderr)
        return 2
    n, v, nseq, T = args.nstates, args.nobs, args.nseq, args.T
    pi, a, b = synth.random_hmm(n, v, seed=20261020)
    off = np.arange(nseq + 1, dtype=np.int64) * T
    total = int(off[-1])
    obs = synth.iid_obs(v, total, seed=20261020)
    h = cv.HMM(pi, a, b, device=args.device)
    if args.xi_part_rows is not None:
        h.set_tuning(xi_part_rows=args.xi_part_rows)
    dev = torch.device("cuda", args.device)
    d_off, d_obs = torch.from_numpy(off).to(dev), torch.from_numpy(obs).to(dev)
    E = torch.from_numpy(np.ascontiguousarray(b.T)).to(dev)[d_obs.long()]  # [sum T, N], ld = N
    ll = {k: torch.zeros(nseq, dtype=torch.float64, device=dev) for k in "abcd"}
    st = {k: torch.zeros(nseq, dtype=torch.uint8, device=dev) for k in "abcd"}
    path = torch.zeros(total, dtype=torch.int32, device=dev)
    pc = {k: torch.zeros(n, dtype=torch.float64, device=dev) for k in "bd"}
    ac = {k: torch.zeros((n, n), dtype=torch.float64, device=dev) for k in "bd"}
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    kw = dict(offsets_host=off, kernel=args.kernel, stream=stream.cuda_stream, workspace_bytes=args.workspace_bytes)
    calls = {
        "a_posterior_path": lambda: cv.posterior_batch_device(h, d_off, d_obs, ll["a"], st["a"], path, **kw),
        "b_counts": lambda: cv.expected_counts_device(h, d_off, d_obs, ll["b"], pc["b"], ac["b"], st["b"], **kw),
        "c_posterior_emissions_path": lambda: cv.posterior_emissions_device(h, d_off, E, ll["c"], st["c"], path, **kw),
        "d_counts_emissions": lambda: cv.expected_counts_emissions_device(h, d_off, E, ll["d"], pc["d"], ac["d"], st["d"],
                                                                          **kw),
    }

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        stream.synchronize()
        cv.timing_begin(h)
        for _ in range(args.calls):
            fn()
        t = cv.timing_end(h)
        return dict(ms_per_call=round(t["total_ms"] / args.calls, 4), fwd_ms=round(t["fwd_ms"] / args.calls, 4),
                    bt_ms=round(t["bt_ms"] / args.calls, 4), launches=t["launches"] // args.calls, kernel=t["kernel"],
                    padded_states=t["padded_states"])

    out = dict(tool="bench_counts", nstates=n, nobs=v, nseq=nseq, T=T, calls=args.calls, warmup=args.warmup,
               workspace_bytes=args.workspace_bytes, xi_part_rows=h.tuning("xi_part_rows"))
    for rnd in (0, 1):
        for name, fn in calls.items():
            out[f"{name}_{rnd}"] = timed(fn)
    best = lambda key: min(out[f"{key}_{r}"]["ms_per_call"] for r in (0, 1))
    out["counts_over_posterior_path"] = round(best("b_counts") / best("a_posterior_path"), 3)
    out["counts_emissions_over_posterior_emissions_path"] = round(
        best("d_counts_emissions") / best("c_posterior_emissions_path"), 3)
    torch.cuda.synchronize(dev)
    out["statuses_ok"] = [int((st[k] == 0).sum().item()) for k in "abcd"]
    out["logliks_equal"] = bool(torch.equal(ll["a"], ll["b"]) and torch.equal(ll["c"], ll["d"]))
    out["sum_pi_cnt"] = [float(pc[k].sum().item()) for k in "bd"]
    out["sum_a_cnt"] = [float(ac[k].sum().item()) for k in "bd"]
    out["max_rel_difference_dense_vs_discrete"] = float(
        ((ac["b"] - ac["d"]).abs() / ac["b"].clamp_min(1e-300)).max().item())
    out["device_bytes_peak"] = cv.device_memory()["peak"]
    print(json.dumps(out))
    assert out["logliks_equal"], "the counts calls' logliks differ from the posterior calls'"
    return 0


if __name__ == "__main__":
    sys.exit(main())
