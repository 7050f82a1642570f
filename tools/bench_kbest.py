#!/usr/bin/env python3
"""Times cv_kbest_batch_device at 4,096 sequences, T = 512, N = 256 for K in {1, 2, 4, 8, 16},
interleaved in the same session with cv_decode_batch_device(kernel=GENERIC, f64, VITERBI) at the
same shape -- the yardstick.  Inputs and outputs are resident on the device.  Every round runs
the decode and then each K once; the figures are the medians over the rounds of the kernels'
device events (cv_last_timing: fwd_ms the forward pass, bt_ms select plus walk, or the decode's
backtrack and re-score).  Prints one line per round and configuration, then one JSON line.

    python tools/bench_kbest.py [--nseq 4096] [--warmup 1] [--rounds 5] [--ks 1,8]
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

KS = [1, 2, 4, 8, 16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nseq", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--ks", default="", help="comma-separated K values (default 1,2,4,8,16)")
    args = ap.parse_args()

    import torch

    import cviterbi as cv
    from cviterbi import synth

    if not torch.cuda.is_available():
        print("bench_kbest: no GPU visible", file=sys.stderr)
        return 2
    nseq = args.nseq
    ks = [int(x) for x in args.ks.split(",")] if args.ks else KS
    c = synth.config("c4", nseq)
    n = len(c["pi"])
    off = c["offsets"]
    total = int(off[-1])
    h = cv.HMM(c["pi"], c["a"], c["b"], c["bdims"], device=args.device)
    dev = torch.device("cuda", args.device)
    d_off, d_obs = torch.from_numpy(off).to(dev), torch.from_numpy(c["obs"]).to(dev)
    d_path = torch.zeros(max(ks), total, dtype=torch.int32, device=dev)
    d_score = torch.zeros(nseq, max(ks), dtype=torch.float64, device=dev)
    d_count = torch.zeros(nseq, dtype=torch.int32, device=dev)
    d_st = torch.zeros(nseq, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))

    def run(k):
        t0 = time.perf_counter()
        if k == 0:
            cv.decode_batch_device(h, d_off, d_obs, d_path, d_score, d_st, offsets_host=off, dtype="f64",
                                   kernel="generic", stream=stream.cuda_stream)
        else:
            cv.kbest_batch_device(h, d_off, d_obs, k, d_path, d_score, d_count, d_st, offsets_host=off,
                                  stream=stream.cuda_stream)
        stream.synchronize()
        return (time.perf_counter() - t0) * 1e3, cv.last_timing(h)

    configs = [0] + ks  # 0: the generic decode
    name = lambda k: "decode_generic" if k == 0 else f"kbest_k{k}"
    rec = {k: dict(call=[], fwd=[], bt=[]) for k in configs}
    info = {}
    for rnd in range(-args.warmup, args.rounds):
        for k in configs:
            ms, t = run(k)
            print(f"round {rnd:2d} {name(k):15s} call {ms:9.3f} ms  fwd {t['fwd_ms']:9.3f}  bt {t['bt_ms']:8.3f}  "
                  f"launches {t['launches']}  kernel {t['kernel']}  S {t['seqs_per_wave']}", flush=True)
            if rnd >= 0:
                rec[k]["call"].append(ms)
                rec[k]["fwd"].append(t["fwd_ms"])
                rec[k]["bt"].append(t["bt_ms"])
                info[k] = t
    out = dict(tool="bench_kbest", nstates=n, nseq=nseq, T=int(off[1] - off[0]), warmup=args.warmup, rounds=args.rounds)
    base = statistics.median(rec[0]["fwd"])
    for k in configs:
        r = rec[k]
        out[name(k)] = dict(fwd_ms=round(statistics.median(r["fwd"]), 3), fwd_min=round(min(r["fwd"]), 3),
                            fwd_max=round(max(r["fwd"]), 3), bt_ms=round(statistics.median(r["bt"]), 3),
                            call_ms=round(statistics.median(r["call"]), 3), launches=info[k]["launches"],
                            seqs_per_workgroup=info[k]["seqs_per_wave"],
                            fwd_over_decode_fwd=round(statistics.median(r["fwd"]) / base, 3))
    out["count_min"] = int(d_count.min().item())
    out["status_ok"] = int((d_st == 0).sum().item())
    out["device_bytes_peak"] = cv.device_memory()["peak"]
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
