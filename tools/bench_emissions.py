#!/usr/bin/env python3
"""Times cv_decode_emissions_device against the discrete decode of the same problem and against a
plain device copy of the score matrix, in one session, on device-resident inputs:

  (a) cv_decode_batch_device(f64, VITERBI) on observations obs of a model with table b;
  (b) cv_decode_emissions_device on E = b^T[obs], gathered once beforehand with torch -- the
      same problem, so its paths, scores and statuses must equal (a)'s bit for bit (asserted);
  (c) torch's device-to-device copy_ of a [sum T, N] f64 tensor: the bytes the staging kernel
      emis_prepare_f64 has to move at the least.

Each is timed with torch events around `--calls` back-to-back calls after `--warmup` calls; the
kernels' own device events (cv_last_timing) split (a) and (b) into forward and backtrack --
(b)'s forward span includes the staging kernel, and its backtrack runs the general f64 interval
test where (a) may run the NONPOS one.  Prints one JSON line.

    python tools/bench_emissions.py [--nstates 256] [--nseq 4096] [--T 512] [--calls 10] [--warmup 3]
                                    [--workspace-bytes B] [--emis-overlap 0|1]
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
    ap.add_argument("--emis-overlap", type=int, default=None,
                    help="tuning key emis_overlap: 0 stages every chunk in line, 1 the next chunk beside the forward")
    args = ap.parse_args()

    import numpy as np
    import torch

    import cviterbi as cv
    from cviterbi import synth

    if not torch.cuda.is_available():
        print("bench_emissions: no GPU visible", file=sys.stderr)
        return 2
    n, v, nseq, T = args.nstates, args.nobs, args.nseq, args.T
    pi, a, b = synth.random_hmm(n, v, seed=20261015)
    off = np.arange(nseq + 1, dtype=np.int64) * T
    total = int(off[-1])
    obs = synth.iid_obs(v, total, seed=20261015)
    h = cv.HMM(pi, a, b, device=args.device)
    if args.emis_overlap is not None:
        h.set_tuning(emis_overlap=args.emis_overlap)
    dev = torch.device("cuda", args.device)
    d_off, d_obs = torch.from_numpy(off).to(dev), torch.from_numpy(obs).to(dev)
    E = torch.from_numpy(np.ascontiguousarray(b.T)).to(dev)[d_obs.long()]  # [sum T, N], ld = N
    E2 = torch.empty_like(E)
    outs = {k: (torch.zeros(total, dtype=torch.int32, device=dev), torch.zeros(nseq, dtype=torch.float64, device=dev),
                torch.zeros(nseq, dtype=torch.uint8, device=dev)) for k in "ab"}
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    kw = dict(offsets_host=off, kernel=args.kernel, stream=stream.cuda_stream, workspace_bytes=args.workspace_bytes)

    def discrete():
        cv.decode_batch_device(h, d_off, d_obs, *outs["a"], dtype="f64", **kw)

    def dense():
        cv.decode_emissions_device(h, d_off, E, *outs["b"], **kw)

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
                     launches=t["launches"], kernel=t["kernel"], padded_states=t["padded_states"],
                     seqs_per_wave=t["seqs_per_wave"])
        return r

    out = dict(tool="bench_emissions", nstates=n, nobs=v, nseq=nseq, T=T, calls=args.calls, warmup=args.warmup,
               workspace_bytes=args.workspace_bytes, emis_overlap=h.tuning("emis_overlap"))
    # interleaved twice, so a drift of the clocks shows as a difference between the rounds
    for rnd in (0, 1):
        out[f"a_discrete_{rnd}"] = timed(discrete, True)
        out[f"b_emissions_{rnd}"] = timed(dense, True)
        out[f"c_copy_{rnd}"] = timed(copy, False)
    same = all(torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x,
                           y.view(torch.int64) if y.dtype == torch.float64 else y)
               for x, y in zip(outs["a"], outs["b"]))
    out["b_equals_a_bit_for_bit"] = bool(same)
    out["status_ok"] = int((outs["b"][2] == 0).sum().item())
    A, B, C = (min(out[f"{k}_{r}"]["ms_per_call"] for r in (0, 1)) for k in ("a_discrete", "b_emissions", "c_copy"))
    P = out["b_emissions_0"]["padded_states"] or n
    moved = 8.0 * (n + P) * total  # read ld = N, write P doubles per element
    stage = min(out[f"b_emissions_{r}"]["fwd_ms"] - out[f"a_discrete_{r}"]["fwd_ms"] for r in (0, 1))
    out["b_minus_a_ms"] = round(B - A, 4)
    out["staging_ms_from_fwd_spans"] = round(stage, 4)
    out["staging_gbps_from_fwd_spans"] = round(moved / stage / 1e6, 1) if stage > 0 else None
    out["copy_gbps"] = round(2 * 8.0 * n * total / C / 1e6, 1)
    out["staging_over_copy"] = round(stage / C, 3)
    out["device_bytes_peak"] = cv.device_memory()["peak"]
    print(json.dumps(out))
    assert same, "decode_emissions_device differs from the discrete decode of the same problem"
    return 0


if __name__ == "__main__":
    sys.exit(main())
