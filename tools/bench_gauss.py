#!/usr/bin/env python3
"""Times the Gaussian entries on device-resident inputs, in one session:

  (a) cv_gauss_emissions_device for every D of --dims against (c) a device-to-device copy of the
      L x N f64 array it writes (the store of E is the floor of the density kernel at small D);
      with it the kernel's f64 VALU operations per second -- 3 per (e, j, d): the difference, the
      square, the fma -- against --roof-tflops when given (the measured f64 VALU roof,
      profiles/r06_valu_roof.txt);
  (b) cv_expected_counts_gauss_device against (d) cv_loglik_grad_emissions_device on the
      precomputed E of the same inputs: what the fused call adds is the density kernel per chunk
      and the moment GEMM.

Each is timed by stream events around `--calls` back-to-back calls after `--warmup` calls, twice,
interleaved; (b) and (d) also by the library's own events (fwd_ms covers the density kernel, bt_ms
the moment kernels).  Prints one JSON line per D.

    python tools/bench_gauss.py [--nstates 256] [--dims 8,32,128] [--nseq 4096] [--T 512]
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
    ap.add_argument("--dims", default="8,32,128")
    ap.add_argument("--nseq", type=int, default=4096)
    ap.add_argument("--T", type=int, default=512)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--workspace-bytes", type=int, default=0)
    ap.add_argument("--gm-part-rows", type=int, default=None, help="tuning key gm_part_rows (default: by rule)")
    ap.add_argument("--roof-tflops", type=float, default=None, help="measured f64 VALU roof, in 1e12 operations / s")
    ap.add_argument("--skip-counts", action="store_true", help="time the density kernel only")
    args = ap.parse_args()

    import numpy as np
    import torch

    import cviterbi as cv
    from cviterbi import synth

    if not torch.cuda.is_available():
        print("bench_gauss: no GPU visible", file=sys.stderr)
        return 2
    n, nseq, T = args.nstates, args.nseq, args.T
    dev = torch.device("cuda", args.device)
    f64 = dict(dtype=torch.float64, device=dev)
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

    def timed_stream(fn):
        for _ in range(args.warmup):
            fn()
        stream.synchronize()
        return round(stream_ms(fn, args.calls), 4)

    pi, a, _ = synth.random_hmm(n, 2, seed=20261021)
    h = cv.gauss_hmm(pi, a, device=args.device)
    if args.gm_part_rows is not None:
        h.set_tuning(gm_part_rows=args.gm_part_rows)
    d_off = torch.from_numpy(off).to(dev)
    E = torch.zeros((total, n), **f64)
    E2 = torch.empty_like(E)

    def copy():
        with torch.cuda.stream(stream):
            E2.copy_(E)

    copy_ms = [timed_stream(copy) for _ in (0, 1)]
    del E2
    torch.cuda.empty_cache()

    for D in [int(v) for v in args.dims.split(",")]:
        rng = np.random.default_rng(20261021 + D)
        mean = rng.normal(0.0, 1.0, size=(n, D))
        var = rng.uniform(0.5, 2.0, size=(n, D))
        # every element drawn around a random state's mean, generated on the device
        g = torch.Generator(device=dev).manual_seed(D)
        z = torch.randint(0, n, (total,), generator=g, device=dev)
        x = torch.from_numpy(mean).to(dev)[z] + torch.randn((total, D), generator=g, **f64)
        center = x.mean(dim=0).cpu().numpy()
        del z
        kw = dict(offsets_host=off, stream=stream.cuda_stream, workspace_bytes=args.workspace_bytes)
        out = dict(tool="bench_gauss", nstates=n, D=D, nseq=nseq, T=T, calls=args.calls, warmup=args.warmup,
                   workspace_bytes=args.workspace_bytes, gm_part_rows=h.tuning("gm_part_rows"), c_copy_ms=copy_ms,
                   copy_bytes=total * n * 8)

        def density():
            cv.gauss_emissions_device(h, x, mean, var, E, stream=stream.cuda_stream)

        out["a_density_ms"] = [timed_stream(density) for _ in (0, 1)]
        best = min(out["a_density_ms"])
        out["density_over_copy"] = round(best / min(copy_ms), 3)
        out["density_valu_tflops"] = round(3.0 * total * n * D / (best * 1e-3) / 1e12, 3)
        if args.roof_tflops:
            out["density_of_valu_roof"] = round(out["density_valu_tflops"] / args.roof_tflops, 3)
        stream.synchronize()
        out["finite_E"] = bool(torch.isfinite(E).all().item())
        if not args.skip_counts:
            ll = {k: torch.zeros(nseq, **f64) for k in "bd"}
            st = {k: torch.zeros(nseq, dtype=torch.uint8, device=dev) for k in "bd"}
            pc = {k: torch.zeros(n, **f64) for k in "bd"}
            ac = {k: torch.zeros((n, n), **f64) for k in "bd"}
            gc, m1, m2 = torch.zeros(n, **f64), torch.zeros((n, D), **f64), torch.zeros((n, D), **f64)
            calls = {
                "d_loglik_grad": lambda: cv.loglik_grad_emissions_device(h, d_off, E, ll["d"], pc["d"], ac["d"], st["d"], **kw),
                "b_counts_gauss": lambda: cv.expected_counts_gauss_device(h, d_off, x, mean, var, ll["b"], pc["b"], ac["b"],
                                                                          gc, m1, m2, st["b"], center=center, **kw),
            }

            def timed(fn):
                ms = timed_stream(fn)
                cv.timing_begin(h)
                for _ in range(args.calls):
                    fn()
                t = cv.timing_end(h)
                return dict(stream_ms_per_call=ms, ms_per_call=round(t["total_ms"] / args.calls, 4),
                            fwd_ms=round(t["fwd_ms"] / args.calls, 4), bt_ms=round(t["bt_ms"] / args.calls, 4),
                            launches=t["launches"] // args.calls)

            for rnd in (0, 1):
                for name, fn in calls.items():
                    out[f"{name}_{rnd}"] = timed(fn)
            bestof = lambda key: min(out[f"{key}_{r}"]["stream_ms_per_call"] for r in (0, 1))  # noqa: E731
            out["added_ms"] = round(bestof("b_counts_gauss") - bestof("d_loglik_grad"), 4)
            out["added_over_density"] = round(out["added_ms"] / best, 3)
            torch.cuda.synchronize(dev)
            out["statuses_ok"] = [int((st[k] == 0).sum().item()) for k in "bd"]
            out["same_bits_as_the_pair"] = bool(torch.equal(ll["b"], ll["d"]) and torch.equal(st["b"], st["d"]))
            out["sum_g_cnt"] = float(gc.sum().item())
        out["device_bytes_peak"] = cv.device_memory()["peak"]
        print(json.dumps(out), flush=True)
        if not args.skip_counts:
            assert out["same_bits_as_the_pair"], "loglik or status differ from gauss_emissions + loglik_grad_emissions"
        h.release_workspaces()
        del x
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
