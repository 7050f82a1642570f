"""GPU: the pipelined schedule of the certified fixed-point first pass (tuning key
t64_fixed_chunks, DESIGN.md "Certified fixed-point first pass").

The pass is forced at small sizes (t64_fixed_first = 1) and split into chunks by the workspace cap,
so that both halves of the double-buffered workspace are reused and a chunk's certificate backtrack
and score run on the second stream beside the next chunk's forward.  Every case holds sequences that
cannot certify -- states 0 and 1 are interchangeable and win under observation 15, an exact tie at
every step -- in its first, a middle and its last chunk, and one out-of-range observation.  A
decode must equal, bit for bit -- paths, score bits, statuses -- the same call with the pass off,
the serial schedule (t64_fixed_chunks = 0) with the same counters, and the C oracle.
"""
import numpy as np
import pytest

import c_oracle as O
import cviterbi as cv
from cviterbi import _lib as L
from cviterbi import synth

pytestmark = pytest.mark.gpu

N, V = 256, 16
TIE = V - 1  # the observation under which states 0 and 1 tie
ROW = N * 4  # workspace bytes per element: one int32 row


def _model():
    pi, a, b = synth.random_hmm(N, V, seed=11)
    b[:, TIE] = -6.0
    b[:2, :] = -8.0
    b[:2, TIE] = np.log10(0.9)
    a[1, :] = a[0, :]
    a[:, 1] = a[:, 0]
    pi[1] = pi[0]
    return pi, a, b


def _case(name):
    """lengths, tie sequences, the sequence with the bad observation, the workspace cap, the chunks
    of the pipelined and of the serial schedule under it."""
    rng = np.random.default_rng(17)
    if name == "eight_chunks":  # two chunks of 12 sequences fit the cap: 8 chunks, each buffer four times
        return dict(lengths=np.full(96, 16), ties=[1, 50, 95], bad=30, cap=2 * 12 * 16 * ROW, unpaired=0)
    if name == "odd_last_chunk":  # 20 + 20 + 9: the last chunk leaves a sequence unpaired
        return dict(lengths=np.full(49, 16), ties=[0, 25, 47], bad=33, cap=2 * 20 * 16 * ROW, unpaired=1)
    # ragged: eight blocks of 200 elements, one chunk each (the serial schedule: two each); even
    # lengths in the even blocks and odd ones in the odd blocks, so a serial chunk pairs exactly the
    # sequences its two blocks pair; 5 and 2 leftovers per block, an empty sequence among them
    even, odd = [40, 40, 22, 22, 22, 8, 30, 16], [39, 39, 33, 33, 17, 35, 1, 1, 1, 1]
    lengths, ties, bad = [], [], None
    for k in range(8):
        blk = np.array(even if k % 2 == 0 else odd)
        rng.shuffle(blk)
        if k % 2 == 0:
            blk = np.insert(blk, 4, 0)
        if k in (0, 4, 7):
            ties.append(len(lengths) + int(np.argmax(blk)))  # one of the paired longest
        if k == 3:
            bad = len(lengths) + int(np.nonzero(blk == 33)[0][0])
        lengths += blk.tolist()
    return dict(lengths=np.array(lengths), ties=ties, bad=bad, cap=2 * 200 * ROW, unpaired=4 * 5 + 4 * 2)


CASES = ("eight_chunks", "odd_last_chunk", "ragged")


def _same(got, ref, what):
    for x, y, name in zip(got, ref, ("path", "score", "status")):
        x, y = np.asarray(x), np.asarray(y)
        if name == "score":
            x, y = x.view(np.uint64), y.view(np.uint64)
        bad = np.nonzero(x != y)[0]
        assert bad.size == 0, f"{what}: {name} differs at {bad[:8]}"


def _decode(h, off, obs, cap, stream=False):
    """The device entry (its observations are range-checked on the device), optionally on a
    stream of the caller's."""
    import torch

    dev = torch.device("cuda", 0)
    off_d, obs_d = torch.from_numpy(off).to(dev), torch.from_numpy(obs).to(dev)
    p_d = torch.full((len(obs),), -9, dtype=torch.int32, device=dev)
    s_d = torch.full((len(off) - 1,), np.nan, dtype=torch.float64, device=dev)
    st_d = torch.full((len(off) - 1,), 77, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    s = torch.cuda.Stream(dev) if stream else None
    cv.decode_batch_device(h, off_d, obs_d, p_d, s_d, st_d, offsets_host=off, dtype="f64", workspace_bytes=cap,
                           stream=s.cuda_stream if stream else None)
    if stream:
        s.synchronize()
    torch.cuda.synchronize(dev)
    return p_d.cpu().numpy(), s_d.cpu().numpy(), st_d.cpu().numpy()


def _handle(model, first, chunks):
    h = cv.HMM(*model)
    h.set_tuning(t64_fixed_first=first, t64_fixed_chunks=chunks)
    return h


@pytest.fixture(scope="module")
def model():
    return _model()


@pytest.fixture(scope="module", params=CASES)
def case(request, model):
    """The batch, and computed once per case: the decode with the pass off, the oracle's decode of
    the batch without its bad observation."""
    c = _case(request.param)
    rng = np.random.default_rng(5)
    off = synth.offsets_from_lengths(c["lengths"])
    obs = rng.integers(0, TIE, size=int(off[-1])).astype(np.int32)
    for s in c["ties"]:
        obs[off[s]:off[s + 1]] = TIE
    clean = obs.copy()
    assert off[c["bad"] + 1] - off[c["bad"]] > 5 and c["bad"] not in c["ties"]
    obs[off[c["bad"]] + 5] = V + 1
    c.update(name=request.param, off=off, obs=obs)
    h0 = _handle(model, 0, 8)
    c["f64"] = _decode(h0, off, obs, c["cap"])
    assert cv.last_fixed_first_stats(h0)["engaged"] == 0
    c["oracle"] = O.decode_batch(*model, off, clean, O.VITERBI, np.float64, nthreads=8)
    return c


def test_pipelined_equals_f64_serial_and_oracle(gpu, model, case):
    off, obs, cap, bad = case["off"], case["obs"], case["cap"], case["bad"]
    nseq = len(off) - 1
    hp, hs = _handle(model, 1, 8), _handle(model, 1, 0)
    pipe = _decode(hp, off, obs, cap)
    stp = cv.last_fixed_first_stats(hp)
    assert cv.last_timing(hp)["kernel"] == "trellis_f64"
    ser = _decode(hs, off, obs, cap)
    sts = cv.last_fixed_first_stats(hs)
    _same(pipe, case["f64"], f"{case['name']}: pipelined vs the pass off")
    _same(ser, case["f64"], f"{case['name']}: serial vs the pass off")
    _same(pipe, ser, f"{case['name']}: pipelined vs serial")
    assert stp == sts, (stp, sts)
    # the ties, the bad observation, the unpaired and the empty sequence are the f64 kernels'
    assert stp["engaged"] == 1 and stp["pinned"] == 0 and stp["certified"] + stp["fallback"] == nseq, stp
    assert stp["certified"] > 0 and stp["fallback"] >= len(case["ties"]) + 1 + case["unpaired"], stp
    # the oracle, but for the sequence with the bad observation
    assert pipe[2][bad] == L.SEQ_BADOBS
    keep = np.arange(nseq) != bad
    ek = np.ones(len(obs), bool)
    ek[off[bad]:off[bad + 1]] = False
    rp, rs, rst = case["oracle"]
    assert np.array_equal(pipe[2][keep], np.asarray(rst)[keep])
    assert np.array_equal(pipe[1][keep].view(np.uint64), np.asarray(rs)[keep].view(np.uint64))
    assert np.array_equal(pipe[0][ek], np.asarray(rp)[ek])


def test_repeated_calls_and_callers_stream(gpu, model, case):
    """Two consecutive calls on one handle, then one on a stream of the caller's: the second call
    reuses both buffers while the handle's events still refer to the first."""
    off, obs, cap = case["off"], case["obs"], case["cap"]
    h = _handle(model, 1, 8)
    first = _decode(h, off, obs, cap)
    st1 = cv.last_fixed_first_stats(h)
    second = _decode(h, off, obs, cap)
    third = _decode(h, off, obs, cap, stream=True)
    assert cv.last_fixed_first_stats(h) == st1
    _same(first, case["f64"], f"{case['name']}: first call")
    _same(second, first, f"{case['name']}: second call")
    _same(third, first, f"{case['name']}: caller's stream")


def test_large_chunks_reuse_buffers(gpu, model):
    """8,192 sequences of T = 8 under a cap of two chunks of 2,048: four chunks of four rounds of
    workgroups each, so a forward that did not wait for the backtrack still reading its buffer, or
    a certificate copy that did not wait for the last backtrack, has time to show.  Pipelined,
    serial (two chunks of 4,096) and the pass off agree, twice in a row on one handle."""
    B, T = 8192, 8
    off = np.arange(B + 1, dtype=np.int64) * T
    obs = synth.iid_obs(TIE, B * T, seed=8)
    obs[off[4000]:off[4001]] = TIE  # a tie in a middle chunk
    cap = 2 * 2048 * T * ROW
    ref = _decode(_handle(model, 0, 8), off, obs, cap)
    hp, hs = _handle(model, 1, 8), _handle(model, 1, 0)
    pipe = _decode(hp, off, obs, cap)
    stp = cv.last_fixed_first_stats(hp)
    assert cv.last_timing(hp)["launches"] >= 4
    again = _decode(hp, off, obs, cap)
    ser = _decode(hs, off, obs, cap)
    assert stp == cv.last_fixed_first_stats(hs) and stp["engaged"] == 1 and stp["pinned"] == 0, stp
    assert stp["certified"] > B // 2 and stp["fallback"] >= 1, stp
    _same(pipe, ref, "large chunks: pipelined vs the pass off")
    _same(again, pipe, "large chunks: second call")
    _same(ser, pipe, "large chunks: serial vs pipelined")


def test_chunk_count_key(gpu, model):
    """t64_fixed_chunks is the least number of chunks of a large batch: 4,096 sequences of T = 2 run
    as two chunks at 2 and as one at 0 or 1, with the same results and counters."""
    B, T = 4096, 2
    off = np.arange(B + 1, dtype=np.int64) * T
    obs = synth.iid_obs(TIE, B * T, seed=3)
    ref = None
    for k, extra in ((0, 0), (1, 0), (2, 1)):
        h = _handle(model, 1, k)
        got = _decode(h, off, obs, 0)
        st = cv.last_fixed_first_stats(h)
        launches = cv.last_timing(h)["launches"]  # the pass's chunks and the fallback's
        assert st["engaged"] == 1 and st["pinned"] == 0, st
        if ref is None:
            ref = (got, st, launches)
        _same(got, ref[0], f"t64_fixed_chunks={k}")
        assert st == ref[1], (k, st, ref[1])
        assert launches == ref[2] + extra, (k, launches, ref[2])
