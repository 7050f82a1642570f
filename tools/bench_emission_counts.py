#!/usr/bin/env python3
"""Times cv_expected_counts_model_device (gamma not requested) against cv_expected_counts_device on
the same input and against a device-to-device copy of an L x NP f64 array (one write and one read of
the rows w_s gamma is what the emission counts add), in one session on device-resident inputs:

  (a) cv_expected_counts_device        (b) cv_expected_counts_model_device        (c) the copy

for every V of --nobs (comma separated).  (a) and (b) are timed by stream events around `--calls`
back-to-back calls after `--warmup` calls -- so the accumulator's memset, the sort and every
kernel count -- and by the library's own events (bt_ms: the backward pass plus the count kernels),
interleaved twice.  The split by kernel comes from a separate rocprofv3 --kernel-trace --stats run
of this program.  Prints one JSON line per V.

    python tools/bench_emission_counts.py [--nstates 256] [--nobs 1024,2,65536] [--nseq 4096] [--T 512]
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
    ap.add_argument("--nobs", default="1024,2,65536")
    ap.add_argument("--nseq", type=int, default=4096)
    ap.add_argument("--T", type=int, default=512)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--kernel", default="auto")
    ap.add_argument("--workspace-bytes", type=int, default=0)
    ap.add_argument("--bcnt-part-rows", type=int, default=None, help="tuning key bcnt_part_rows (default: by rule)")
    args = ap.parse_args()

    import numpy as np
    import torch

    import cviterbi as cv
    from cviterbi import synth

    if not torch.cuda.is_available():
        print("bench_emission_counts: no GPU visible", file=sys.stderr)
        return 2
    n, nseq, T = args.nstates, args.nseq, args.T
    npad = (n + 63) // 64 * 64
    dev = torch.device("cuda", args.device)
    off = np.arange(nseq + 1, dtype=np.int64) * T
    total = int(off[-1])
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))

    def stream_ms(fn, calls):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            t0.record()
            for _ in range(calls):
                fn()
            t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) / calls

    # (c) the copy, once for the session
    src = torch.ones((total, npad), dtype=torch.float64, device=dev)
    dst = torch.empty_like(src)

    def copy():
        with torch.cuda.stream(stream):
            dst.copy_(src)

    for _ in range(args.warmup):
        copy()
    copy_ms = [round(stream_ms(copy, args.calls), 4) for _ in (0, 1)]
    del src, dst
    torch.cuda.empty_cache()

    for v in [int(x) for x in args.nobs.split(",")]:
        pi, a, b = synth.random_hmm(n, v, seed=20261020)
        obs = synth.iid_obs(v, total, seed=20261020)
        h = cv.HMM(pi, a, b, device=args.device)
        if args.bcnt_part_rows is not None:
            h.set_tuning(bcnt_part_rows=args.bcnt_part_rows)
        d_off, d_obs = torch.from_numpy(off).to(dev), torch.from_numpy(obs).to(dev)
        ll = {k: torch.zeros(nseq, dtype=torch.float64, device=dev) for k in "ab"}
        st = {k: torch.zeros(nseq, dtype=torch.uint8, device=dev) for k in "ab"}
        pc = {k: torch.zeros(n, dtype=torch.float64, device=dev) for k in "ab"}
        ac = {k: torch.zeros((n, n), dtype=torch.float64, device=dev) for k in "ab"}
        bc = torch.zeros((n, v), dtype=torch.float64, device=dev)
        kw = dict(offsets_host=off, kernel=args.kernel, stream=stream.cuda_stream, workspace_bytes=args.workspace_bytes)
        calls = {
            "a_counts": lambda: cv.expected_counts_device(h, d_off, d_obs, ll["a"], pc["a"], ac["a"], st["a"], **kw),
            "b_counts_model": lambda: cv.expected_counts_model_device(h, d_off, d_obs, ll["b"], pc["b"], ac["b"], bc,
                                                                      st["b"], **kw),
        }

        def timed(fn):
            for _ in range(args.warmup):
                fn()
            stream.synchronize()
            ms = stream_ms(fn, args.calls)
            cv.timing_begin(h)
            for _ in range(args.calls):
                fn()
            t = cv.timing_end(h)
            return dict(stream_ms_per_call=round(ms, 4), ms_per_call=round(t["total_ms"] / args.calls, 4),
                        fwd_ms=round(t["fwd_ms"] / args.calls, 4), bt_ms=round(t["bt_ms"] / args.calls, 4),
                        launches=t["launches"] // args.calls)

        out = dict(tool="bench_emission_counts", nstates=n, nobs=v, nseq=nseq, T=T, calls=args.calls, warmup=args.warmup,
                   workspace_bytes=args.workspace_bytes, bcnt_part_rows=h.tuning("bcnt_part_rows"),
                   c_copy_ms=copy_ms, copy_bytes=total * npad * 8)
        for rnd in (0, 1):
            for name, fn in calls.items():
                out[f"{name}_{rnd}"] = timed(fn)
        best = lambda key: min(out[f"{key}_{r}"]["stream_ms_per_call"] for r in (0, 1))  # noqa: E731
        out["added_ms"] = round(best("b_counts_model") - best("a_counts"), 4)
        out["added_over_copy"] = round(out["added_ms"] / min(copy_ms), 3)
        torch.cuda.synchronize(dev)
        out["statuses_ok"] = [int((st[k] == 0).sum().item()) for k in "ab"]
        out["same_bits_as_counts"] = bool(torch.equal(ll["a"], ll["b"]) and torch.equal(pc["a"], pc["b"])
                                          and torch.equal(ac["a"], ac["b"]))
        out["sum_b_cnt"] = float(bc.sum().item())
        out["device_bytes_peak"] = cv.device_memory()["peak"]
        print(json.dumps(out), flush=True)
        assert out["same_bits_as_counts"], "loglik, pi_cnt or a_cnt differ from cv_expected_counts_device's"
        h.release_workspaces()
        del h, bc
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
