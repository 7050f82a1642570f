"""Config 4 (N = 256, T = 512, 65,536 sequences) through cv_decode_batch_device, f64, CALLS times:
the program to put behind `rocprofv3 --kernel-trace -d <dir> --output-format csv --` (kernel
trace only, one run per library; CV_LIB_PATH selects the library, CV_<KEY> the tuning keys), then
`python tools/kt_list.py <dir> obs_first_bad 0.2` lists the last call's kernels.  Prints per call
the wall time, the event sums, the first pass's counters and, where the library has it, its kind.
  python tools/trace_config4.py [CALLS] [B]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "consistent-viterbi_amd"))
import torch  # noqa: E402

import cviterbi as cv  # noqa: E402
from cviterbi import synth  # noqa: E402


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    B = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
    c = synth.config("c4", B)
    h = cv.HMM(c["pi"], c["a"], c["b"])
    dev = torch.device("cuda", 0)
    off = np.asarray(c["offsets"], np.int64)
    off_d, obs_d = torch.from_numpy(off).to(dev), torch.from_numpy(np.asarray(c["obs"], np.int32)).to(dev)
    p_d = torch.empty(len(c["obs"]), dtype=torch.int32, device=dev)
    s_d = torch.empty(B, dtype=torch.float64, device=dev)
    st_d = torch.empty(B, dtype=torch.uint8, device=dev)
    for k in range(1, calls + 1):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        cv.decode_batch_device(h, off_d, obs_d, p_d, s_d, st_d, offsets_host=off, dtype="f64")
        torch.cuda.synchronize(dev)
        wall = (time.perf_counter() - t0) * 1e3
        t = cv.last_timing(h)
        kind = getattr(cv, "last_first_pass_kind", lambda _: "?")(h)  # an older tree has no such accessor
        print(f"call {k}: wall {wall:.2f} ms, {t}, stats {cv.last_fixed_first_stats(h)}, first pass {kind}", flush=True)
    print(f"score sum {float(s_d.sum().item())!r}, status max {int(st_d.max().item())}")


if __name__ == "__main__":
    main()
