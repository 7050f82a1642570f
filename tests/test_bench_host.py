"""CPU: bench.py's host-side helpers -- the committed PMC summaries it scales `roofline.traffic`
and the effective clock from (the full-batch forward at N = 1, the row-split shard kernel of
the N = 8 strong-scaling line, the f32 forward)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def test_pmc_summaries_per_kernel():
    full = bench.load_pmc(True)
    shard = bench.load_pmc(True, row_split=True)
    f32 = bench.load_pmc(False)
    assert full and shard and f32
    # HBM bytes per decoded element: the f64 delta rows (16 N B) plus a little read traffic,
    # about the same per element whatever the batch
    for d in (full, shard):
        assert 16 * 256 * 0.45 < d["per_elem"] < 16 * 256 * 0.55, d
    assert abs(shard["per_elem"] / full["per_elem"] - 1) < 0.02
    assert "rs_8192" in shard["source"] and "rs_8192" not in full["source"]
    assert 2.0 < full["clock_ghz"] < 2.5 and 2.0 < shard["clock_ghz"] < 2.5
    assert f32["per_elem"] < full["per_elem"]


def test_dump_outputs_files(tmp_path):
    """--dump-outputs: every score and status, the paths of a seeded sample of sequences that is
    the same from call to call, float arrays only, under 64 MB at the flagship batch."""
    import numpy as np
    import torch

    n, T = bench.DUMP_PATH_SEQS + 37, bench.T_LEN  # above the sample size: the sampled branch
    path = (torch.arange(n * T, dtype=torch.int64) % 251).to(torch.int32)
    score = -torch.arange(n, dtype=torch.float64) / 3
    status = (torch.arange(n) % 3 == 0).to(torch.uint8)
    got = []
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), path, score, status, n)
        got.append({f[:-4]: np.load(str(tmp_path / d / f)) for f in os.listdir(str(tmp_path / d))})
    a, b = got
    assert sorted(a) == ["path", "path_sequences", "score", "status"]
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert a["path"].dtype == np.float32 and a["status"].dtype == np.float32
    assert a["score"].dtype == np.float64 and a["path_sequences"].dtype == np.float64
    seqs = a["path_sequences"].astype(np.int64)
    assert len(seqs) == bench.DUMP_PATH_SEQS and np.all(np.diff(seqs) > 0) and 0 <= seqs[0] and seqs[-1] < n
    assert np.array_equal(a["path"], path.view(n, T).numpy()[seqs].astype(np.float32))
    assert np.array_equal(a["score"], score.numpy()) and np.array_equal(a["status"], status.numpy().astype(np.float32))
    # the flagship batch: sampled paths + every score and status
    assert bench.DUMP_PATH_SEQS * T * 4 + bench.B_TOTAL * (8 + 4) + bench.DUMP_PATH_SEQS * 8 < 64e6
    # a batch at or below the sample size is written whole
    bench.dump_outputs(str(tmp_path / "c"), path[: 5 * T], score[:5], status[:5], 5)
    assert np.array_equal(np.load(str(tmp_path / "c" / "path_sequences.npy")), np.arange(5.0))
    assert np.load(str(tmp_path / "c" / "path.npy")).shape == (5, T)
