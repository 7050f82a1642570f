"""GPU: the few-sequence f64 forward at NP = 256 (trellis_few_f64, tuning key t64_few; DESIGN.md,
the f64 trellis's layout list): one 16-wave workgroup per two sequences.

With the key at 1 (whenever supported) a plain row-A0 f64 batch decode at 192 < N <= 256 must
equal, bit for bit -- paths, score bits, statuses -- the same decode with the key at 0 (the
pair-of-waves layouts) and the C oracle, and with t64_lo_every at 1 and at 8 alike: the layout
writes full rows, which the sparse backtrack must accept.
"""
import numpy as np
import pytest

import c_oracle as O
import cviterbi as cv
from cviterbi import _lib as L
from cviterbi import synth

pytestmark = pytest.mark.gpu

V = 12
NSEQ = (1, 2, 3, 5, 64)


def _same(got, ref, what):
    for x, y, name in zip(got, ref, ("path", "score", "status")):
        x, y = np.asarray(x), np.asarray(y)
        if name == "score":
            x, y = x.view(np.uint64), y.view(np.uint64)
        bad = np.nonzero(x != y)[0]
        assert bad.size == 0, f"{what}: {name} differs at {bad[:8]}"


def _decode_device(h, off, obs):
    """The device entry (its observations are range-checked on the device)."""
    import torch

    dev = torch.device("cuda", 0)
    off_d, obs_d = torch.from_numpy(np.asarray(off, np.int64)).to(dev), torch.from_numpy(obs).to(dev)
    p_d = torch.full((len(obs),), -9, dtype=torch.int32, device=dev)
    s_d = torch.full((len(off) - 1,), np.nan, dtype=torch.float64, device=dev)
    st_d = torch.full((len(off) - 1,), 77, dtype=torch.uint8, device=dev)
    cv.decode_batch_device(h, off_d, obs_d, p_d, s_d, st_d, offsets_host=np.asarray(off, np.int64), dtype="f64")
    torch.cuda.synchronize(dev)
    return p_d.cpu().numpy(), s_d.cpu().numpy(), st_d.cpu().numpy()


def _all_ways(model, off, obs, what, device=False):
    """The decode with the few-sequence layout at t64_lo_every 8 and 1 and with the pair-of-waves
    layouts; all agree.  Returns the few-sequence result."""
    h = cv.HMM(*model)
    run = (lambda: _decode_device(h, off, obs)) if device else (
        lambda: cv.decode_batch(h, off, obs, dtype="f64", rescore_f64=False))
    h.set_tuning(t64_few=1, t64_lo_every=8)
    few = run()
    t = cv.last_timing(h)
    assert t["kernel"] == "trellis_f64" and t["padded_states"] == 256 and t["seqs_per_wave"] == 0, t
    h.set_tuning(t64_few=1, t64_lo_every=1)
    _same(run(), few, f"{what}: t64_lo_every 1 vs 8")
    h.set_tuning(t64_few=0, t64_lo_every=8)
    ref = run()
    assert cv.last_timing(h)["seqs_per_wave"] > 0
    _same(few, ref, f"{what}: t64_few 1 vs 0")
    return few


@pytest.fixture(scope="module", params=[193, 225, 256])
def model(request):
    return synth.random_hmm(request.param, V, seed=request.param)


@pytest.mark.parametrize("T", [1, 2, 9, 33])
def test_equal_lengths(gpu, model, T):
    """1 (half a workgroup), 2, 3 and 5 (an odd last workgroup) and 64 sequences."""
    for B in NSEQ:
        off = np.arange(B + 1, dtype=np.int64) * T
        obs = synth.iid_obs(V, B * T, seed=1000 * T + B)
        got = _all_ways(model, off, obs, f"T={T} B={B}")
        _same(got, O.decode_batch(*model, off, obs, O.VITERBI, np.float64), f"T={T} B={B} vs the oracle")


def test_ragged_lengths_and_order(gpu, model):
    """Unequal lengths force the longest-first schedule: the two sequences of a workgroup come
    through `order` and differ in length, one of them is empty, one has a single element."""
    rng = np.random.default_rng(4)
    for B in NSEQ:
        lengths = rng.integers(1, 41, size=B)
        if B >= 3:
            lengths[0], lengths[1], lengths[2] = 7, 0, 1
        if B == 2:
            lengths[:] = (3, 29)
        off = synth.offsets_from_lengths(lengths)
        obs = rng.integers(0, V, size=max(int(off[-1]), 1)).astype(np.int32)[: int(off[-1])]
        got = _all_ways(model, off, obs, f"ragged B={B}")
        _same(got, O.decode_batch(*model, off, obs, O.VITERBI, np.float64), f"ragged B={B} vs the oracle")


def test_inf_transitions_and_an_infeasible_sequence(gpu):
    """-inf transitions (a band), emissions and initial states at N = 256; observation V - 1 is
    impossible and ends every fifth sequence."""
    n = 256
    pi, a, b = synth.random_hmm(n, V, seed=13)
    i, j = np.indices((n, n))
    a[(j - i) % n > 3] = -np.inf
    rng = np.random.default_rng(13)
    b[rng.random((n, V)) < 0.5] = -np.inf
    pi[::2] = -np.inf
    b[:, V - 1] = -np.inf
    B, T = 21, 24
    off = np.arange(B + 1, dtype=np.int64) * T
    obs = rng.integers(0, V - 1, size=B * T).astype(np.int32)
    obs[off[1::5] - 1] = V - 1
    got = _all_ways((pi, a, b), off, obs, "banded -inf")
    ref = O.decode_batch(pi, a, b, off, obs, O.VITERBI, np.float64)
    _same(got, ref, "banded -inf vs the oracle")
    assert (ref[2] == L.SEQ_INFEASIBLE).any() and (ref[2] == L.SEQ_OK).any()


def test_bad_observation_beside_clean_neighbours(gpu, model):
    """An out-of-range observation in one sequence of a workgroup: BADOBS there, its partner and
    every other sequence as the oracle decodes them."""
    B, T = 6, 17
    off = np.arange(B + 1, dtype=np.int64) * T
    clean = synth.iid_obs(V, B * T, seed=21)
    obs = clean.copy()
    k = 2
    obs[off[k] + 5] = V + 3
    got = _all_ways(model, off, obs, "bad observation", device=True)
    assert got[2][k] == L.SEQ_BADOBS
    rp, rs, rst = O.decode_batch(*model, off, clean, O.VITERBI, np.float64)
    keep = np.arange(B) != k
    ek = np.ones(len(obs), bool)
    ek[off[k]:off[k + 1]] = False
    assert np.array_equal(got[2][keep], np.asarray(rst)[keep])
    assert np.array_equal(got[1][keep].view(np.uint64), np.asarray(rs)[keep].view(np.uint64))
    assert np.array_equal(got[0][ek], np.asarray(rp)[ek])
