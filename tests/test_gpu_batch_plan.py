"""GPU: the batch entries split a batch into the same chunks under a workspace cap as before the
planner moved to csrc/batchplan.cpp, and the split never changes a result.  cv.last_timing(h)
["launches"] is the number of chunks a call ran; the expected counts below were printed by the
build of the commit before the move (same inputs, same caps) and written down here -- they are
not read from the build under test."""
import numpy as np
import pytest

import cviterbi as cv
from cviterbi import _lib as L
from cviterbi import synth

pytestmark = pytest.mark.gpu

N, V, K = 8, 6, 3


def _ragged():
    lengths = np.random.default_rng(11).integers(0, 31, size=40)
    lengths[3], lengths[7] = 0, 30
    return lengths


BATCHES = {"ragged": _ragged(), "uniform": np.full(24, 16)}

# entry -> (call, workspace bytes one element takes from the cap).  The bytes are the kernels'
# rows at N = 8: the f64 trellis and the posterior pad to 64 states of f64, the f32 trellis to 16
# (one wave per sequence) or 32 (workgroup kernels), the generic kernels keep N reals, K-best
# N * KT u16 at list width KT = 4, dense emissions add a staged row of 64 f64 and an index.  The
# pipelined decodes (two streams, double-buffered workspace) give each chunk half the cap.
ENTRIES = {
    "f64_auto": (lambda h, off, obs, em, ws: cv.decode_batch(h, off, obs, dtype="f64", workspace_bytes=ws), 512),
    "f32_trellis": (lambda h, off, obs, em, ws: cv.decode_batch(h, off, obs, dtype="f32", kernel="trellis",
                                                                workspace_bytes=ws), 64),
    "f32_trellis_pipelined": (lambda h, off, obs, em, ws: cv.decode_batch(
        h, off, obs, dtype="f32", kernel="trellis", variant="nowave", workspace_bytes=ws), 2 * 128),
    "generic_f64": (lambda h, off, obs, em, ws: cv.decode_batch(h, off, obs, dtype="f64", kernel="generic",
                                                                workspace_bytes=ws), 2 * 64),
    "generic_f32": (lambda h, off, obs, em, ws: cv.decode_batch(h, off, obs, dtype="f32", kernel="generic",
                                                                workspace_bytes=ws), 2 * 32),
    "posterior_gamma": (lambda h, off, obs, em, ws: cv.posterior_batch(h, off, obs, gamma=True, workspace_bytes=ws),
                        512),
    "kbest3": (lambda h, off, obs, em, ws: cv.kbest_batch(h, off, obs, K, workspace_bytes=ws), 64),
    "emissions": (lambda h, off, obs, em, ws: cv.decode_emissions(h, off, em, workspace_bytes=ws), 512 + 512 + 4),
}

# (batch, entry) -> chunks run at the caps (unset, about three chunks, below the longest
# sequence's need); None: the call fails with CV_ENOMEM (K-best never splits a sequence)
EXPECTED = {
    ("ragged", "f64_auto"): (1, 4, 30),
    ("ragged", "f32_trellis"): (1, 4, 30),
    ("ragged", "f32_trellis_pipelined"): (1, 4, 30),
    ("ragged", "generic_f64"): (1, 4, 30),
    ("ragged", "generic_f32"): (1, 4, 30),
    ("ragged", "posterior_gamma"): (1, 4, 30),
    ("ragged", "kbest3"): (1, 4, None),
    ("ragged", "emissions"): (1, 4, 30),
    ("uniform", "f64_auto"): (1, 3, 24),
    ("uniform", "f32_trellis"): (1, 3, 24),
    ("uniform", "f32_trellis_pipelined"): (1, 3, 24),
    ("uniform", "generic_f64"): (1, 3, 24),
    ("uniform", "generic_f32"): (1, 3, 24),
    ("uniform", "posterior_gamma"): (1, 3, 24),
    ("uniform", "kbest3"): (1, 3, None),
    ("uniform", "emissions"): (1, 3, 24),
}


def caps(lengths, per_elem):
    total, longest = int(lengths.sum()), int(lengths.max())
    return 0, per_elem * -(-total // 3), per_elem * (longest - 1)


@pytest.fixture(scope="module")
def hmm(gpu):
    pi, a, b = synth.random_hmm(N, V, seed=5)
    return cv.HMM(pi, a, b, device=gpu)


def inputs(lengths):
    off = synth.offsets_from_lengths(lengths)
    rng = np.random.default_rng(12)
    obs = rng.integers(0, V, size=int(off[-1])).astype(np.int32)
    emis = -5.0 * rng.random((int(off[-1]), N))
    return off, obs, emis


def run(h, batch, entry):
    """[(launches, outputs) or None where the call fails with CV_ENOMEM] at the three caps."""
    call, per_elem = ENTRIES[entry]
    off, obs, emis = inputs(BATCHES[batch])
    res = []
    for ws in caps(BATCHES[batch], per_elem):
        try:
            out = call(h, off, obs, emis, ws)
        except cv.CVError as e:
            assert e.status == L.CV_ENOMEM, e
            res.append(None)
            continue
        res.append((cv.last_timing(h)["launches"], out))
    return res


@pytest.mark.parametrize("entry", list(ENTRIES))
@pytest.mark.parametrize("batch", list(BATCHES))
def test_chunks_and_results_under_a_cap(hmm, batch, entry):
    res = run(hmm, batch, entry)
    got = tuple(r[0] if r else None for r in res)
    print(batch, entry, got)
    assert got == EXPECTED[(batch, entry)]
    whole = res[0][1]
    for r in res[1:]:
        if r is None:
            continue
        for x, y in zip(whole, r[1]):
            assert (x is None and y is None) or (x.dtype == y.dtype and x.shape == y.shape
                                                 and x.tobytes() == y.tobytes()), (batch, entry)
