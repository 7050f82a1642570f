"""GPU: the certified f32 round-up first pass of the plain f64 batch decode (tuning key
t64_f32ru_first, DESIGN.md "Certified f32 round-up first pass").

  * what the forward and the certificate backtrack store -- rows, the shifts mu, the path, the
    losing candidates r_t and E -- equals the numpy model (tools/probe_f32ru.py) bit for bit, and
    differs from the same model run with round-to-nearest adds (the rounding mode is in force);
  * with the key at 1 a decode equals, bit for bit -- paths, score bits, statuses -- the same
    decode on the f64 kernels alone (both first-pass keys 0);
  * the counters are the model's, last_first_pass_kind names the pass, and with the key at its
    default a small call under t64_fixed_first = 1 still takes the integer pass;
  * the chunked pipeline and the serial schedule agree, one handle alternates between the round-up
    pass, the integer pass and the f64 kernels, and the f64 kernels that follow the forward on its
    stream return their usual bits.
"""
import importlib.util
import os

import numpy as np
import pytest

import cviterbi as cv
from cviterbi import _lib as L
from cviterbi import synth

pytestmark = pytest.mark.gpu


def _tool(name):
    spec = importlib.util.spec_from_file_location(
        name, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


M = _tool("probe_f32ru")
MI = _tool("probe_fixed_first")

N, V = 256, 16
ROW = N * 4
DEFAULT = 16777216


def _same(got, ref, what):
    for x, y, name in zip(got, ref, ("path", "score", "status")):
        x, y = np.asarray(x), np.asarray(y)
        if name == "score":
            x, y = x.view(np.uint64), y.view(np.uint64)
        bad = np.nonzero(x != y)[0]
        assert bad.size == 0, f"{what}: {name} differs at {bad[:8]}"


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _decode_device(h, off, obs, cap=0):
    """The device entry (observations are range-checked on the device, not by the host)."""
    import torch

    dev = torch.device("cuda", 0)
    off = np.asarray(off, np.int64)
    off_d, obs_d = torch.from_numpy(off).to(dev), torch.from_numpy(obs).to(dev)
    p_d = torch.full((len(obs),), -9, dtype=torch.int32, device=dev)
    s_d = torch.full((len(off) - 1,), np.nan, dtype=torch.float64, device=dev)
    st_d = torch.full((len(off) - 1,), 77, dtype=torch.uint8, device=dev)
    cv.decode_batch_device(h, off_d, obs_d, p_d, s_d, st_d, offsets_host=off, dtype="f64", workspace_bytes=cap)
    torch.cuda.synchronize(dev)
    return p_d.cpu().numpy(), s_d.cpu().numpy(), st_d.cpu().numpy()


def _run(h, off, obs, device=False, cap=0):
    if device or cap:
        return _decode_device(h, off, obs, cap)
    return cv.decode_batch(h, off, obs, dtype="f64", rescore_f64=False)


def _on_off(h, off, obs, what, device=False, cap=0, chunks=8):
    """The decode through the round-up pass and on the f64 kernels alone; they agree.  Returns
    (result, the pass's stats, the pass's kind)."""
    h.set_tuning(t64_f32ru_first=1, t64_fixed_first=0, t64_fixed_chunks=chunks)
    on = _run(h, off, obs, device, cap)
    st, kind = cv.last_fixed_first_stats(h), cv.last_first_pass_kind(h)
    assert cv.last_timing(h)["kernel"] == "trellis_f64"
    h.set_tuning(t64_f32ru_first=0, t64_fixed_first=0)
    ref = _run(h, off, obs, device, cap)
    st0 = cv.last_fixed_first_stats(h)
    assert st0["engaged"] == 0 and st0["certified"] == 0 and st0["fallback"] == 0, st0
    assert cv.last_first_pass_kind(h) == "none"
    _same(on, ref, f"{what}: key 1 vs 0")
    return on, st, kind


@pytest.fixture(scope="module")
def model():
    return synth.random_hmm(N, V, seed=11)


@pytest.fixture(scope="module")
def traced():
    """Per (n, T): the model's run on 8 sequences, computed once (sequences are independent, so
    the first 2 and 4 of them are the model's run on 2 and 4)."""
    cache = {}

    def get(n, T):
        if (n, T) not in cache:
            pi, a, b = synth.random_hmm(n, V, seed=100 + n)
            obs = synth.iid_obs(V, 9 * T, seed=7 * n + T).reshape(9, T)
            tb = M.tables(pi, a, b)
            rows, mu = M.forward(tb, obs[:8].astype(np.int64))
            path, r, E = M.backtrack(tb, rows)
            cache[(n, T)] = dict(model=(pi, a, b), obs=obs, tb=tb, rows=rows, mu=mu, path=path, r=r, E=E)
        return cache[(n, T)]

    return get


@pytest.mark.parametrize("T", [1, 2, 3, 65, 130])
@pytest.mark.parametrize("n", [225, 240, 256])
def test_stored_values_equal_the_model_bit_for_bit(gpu, traced, n, T):
    """2, 4 and 9 sequences (of 9 the pass runs four pairs and leaves the last to the f64 kernels:
    its slots stay untouched)."""
    c = traced(n, T)
    h = cv.HMM(*c["model"])
    for S in (2, 4, 9):
        got = cv.f32ru_trace(h, c["obs"][:S])
        P = S - S % 2
        what = f"N={n} T={T} S={S}"
        assert np.array_equal(_bits(got["rows"][:, :P]), _bits(c["rows"][:, :P])), what + ": rows"
        assert np.array_equal(_bits(got["mu"][:P, 1:]), _bits(c["mu"][:P, 1:])), what + ": mu"
        assert np.array_equal(got["path"][:P], c["path"][:P]), what + ": path"
        assert np.array_equal(_bits(got["r"][:P, 1:]), _bits(c["r"][:P, 1:])), what + ": r"
        assert np.array_equal(_bits(got["E"][:P]), _bits(c["E"][:P])), what + ": E"
        if S % 2:
            assert not got["rows"][:, P:].any() and not got["path"][P:].any() and got["E"][P] == 0


def test_rows_differ_from_round_to_nearest(gpu, traced):
    """The same model with round-to-nearest adds gives other rows: the kernel's are the rounded-up
    ones, entry by entry no lower."""
    c = traced(256, 65)
    got = cv.f32ru_trace(cv.HMM(*c["model"]), c["obs"][:8])
    rn_rows, _ = M.forward(c["tb"], c["obs"][:8].astype(np.int64), add=M.rn_add)
    assert np.array_equal(_bits(got["rows"]), _bits(c["rows"]))
    differ = _bits(got["rows"]) != _bits(rn_rows)
    assert differ.mean() > 0.25, differ.mean()
    assert differ[1:4].any()  # from the first steps on


@pytest.mark.parametrize("T", [1, 2, 3, 64])
def test_equal_lengths_counts_and_kind(gpu, model, T):
    """B = 1 (not the pass's), 7 and 9 (an unpaired sequence), 8, 130: results are the f64
    kernels', the counters the model's."""
    pi, a, b = model
    for B in (1, 7, 8, 9, 130):
        off = np.arange(B + 1, dtype=np.int64) * T
        obs = synth.iid_obs(V, B * T, seed=100 * T + B)
        got, st, kind = _on_off(cv.HMM(pi, a, b), off, obs, f"T={T} B={B}")
        if B == 1:
            assert st["engaged"] == 0 and kind == "none", (st, kind)
            continue
        _, cert, _, _ = M.decode(pi, a, b, obs.reshape(B, T).astype(np.int64)[: B - B % 2])
        assert kind == "f32ru"
        assert st == dict(engaged=1, certified=int(cert.sum()), fallback=B - int(cert.sum()), pinned=0), (st, cert.sum())
        assert st["fallback"] >= B % 2


def test_ragged_lengths_and_empty_sequences(gpu, model):
    """Lengths 1..40 and empty sequences, 77 sequences through the order schedule: equal-length
    neighbours of the longest-first order are paired, the others take the f64 kernels."""
    pi, a, b = model
    rng = np.random.default_rng(3)
    lengths = np.concatenate([[0, 0, 1, 1, 2, 2, 3, 40, 40, 40], rng.integers(1, 41, size=67)])
    rng.shuffle(lengths)
    off = synth.offsets_from_lengths(lengths)
    obs = rng.integers(0, V, size=int(off[-1])).astype(np.int32)
    got, st, kind = _on_off(cv.HMM(pi, a, b), off, obs, "ragged")
    assert kind == "f32ru" and st["engaged"] == 1 and st["certified"] + st["fallback"] == len(lengths), st
    assert st["certified"] > 0 and st["fallback"] >= 2, st
    assert (got[2][lengths == 0] == got[2][lengths == 0][0]).all()


def test_bad_observation(gpu, model):
    """An out-of-range observation in one sequence of a pair: that sequence reports it, its
    partner and everything else is bit-identical to the f64 kernels'."""
    pi, a, b = model
    B, T = 12, 20
    off = np.arange(B + 1, dtype=np.int64) * T
    obs = synth.iid_obs(V, B * T, seed=21)
    obs[off[5] + 7] = V + 3
    got, st, _ = _on_off(cv.HMM(pi, a, b), off, obs, "bad observation", device=True)
    assert got[2][5] == L.SEQ_BADOBS and (np.delete(got[2], 5) == L.SEQ_OK).all()
    assert st["engaged"] == 1 and st["fallback"] >= 1 and st["certified"] + st["fallback"] == B, st


def test_banded_inf_model_at_256(gpu):
    """-inf transitions, emissions and initial states at N = 256 (banded a, half of b and pi), and
    an impossible observation that ends every sixth sequence."""
    pi, a, b = synth.random_hmm(N, 8, seed=13)
    i, j = np.indices((N, N))
    a[(j - i) % N > 3] = -np.inf
    rng = np.random.default_rng(13)
    b[rng.random((N, 8)) < 0.5] = -np.inf
    pi[::2] = -np.inf
    b[:, 7] = -np.inf
    B, T = 64, 24
    off = np.arange(B + 1, dtype=np.int64) * T
    obs = rng.integers(0, 7, size=B * T).astype(np.int32)
    obs[off[1::16] - 1] = 7  # 4 of 64: an infeasible sequence fails its certificate, and the guard counts it
    got, st, _ = _on_off(cv.HMM(pi, a, b), off, obs, "banded -inf")
    bad = int((got[2] != L.SEQ_OK).sum())
    assert (got[2] == L.SEQ_INFEASIBLE).sum() >= 4 and (got[2] == L.SEQ_OK).any()
    _, cert, _, _ = M.decode(pi, a, b, obs.reshape(B, T).astype(np.int64))
    nc = int(cert.sum())
    assert not cert[got[2] != L.SEQ_OK].any() and nc > B // 2
    assert st == dict(engaged=1, certified=nc, fallback=B - nc, pinned=0) and B - nc >= bad, (st, nc, bad)


@pytest.mark.parametrize("eps,mixed", [(1e-3, True), (1e-4, False)])
def test_small_margins(gpu, model, eps, mixed):
    """f32 arithmetic is scale-free, so margins are made small against the values: the model on a
    grid of quarter decades plus eps times itself.  1e-3: a few of 96 sequences fail, so certified
    and f64-decoded sequences share the call and each must land in its own slot.  1e-4: more than
    a quarter fail, which is above 1 in 8: the guard."""
    pi, a, b = (np.round(x * 4) / 4 + eps * x for x in model)
    B, T = 96, 48
    off = np.arange(B + 1, dtype=np.int64) * T
    obs = synth.iid_obs(V, B * T, seed=11)
    _, cert, _, _ = M.decode(pi, a, b, obs.reshape(B, T).astype(np.int64))
    nc = int(cert.sum())
    h = cv.HMM(pi, a, b)
    got, st, kind = _on_off(h, off, obs, f"eps {eps}")
    if mixed:
        assert 0 < B - nc <= B // 8
        assert st == dict(engaged=1, certified=nc, fallback=B - nc, pinned=0) and kind == "f32ru", (st, nc, kind)
    else:
        assert B // 4 < B - nc < 3 * B // 4
        assert st == dict(engaged=1, certified=0, fallback=B, pinned=1) and kind == "f32ru", (st, nc, kind)


def test_identical_states_fall_back_and_pin(gpu, model):
    """States 0 and 1 identical and dominant: an exact tie at every step, so no sequence
    certifies, the results are the f64 kernels', and the handle is pinned to them."""
    pi, a, b = (x.copy() for x in model)
    a[1, :], b[1, :], pi[1] = a[0, :], b[0, :], pi[0]
    a[:, :2] = np.log10(0.45)
    b[:2, :] = np.log10(0.9)
    B, T = 64, 16
    off = np.arange(B + 1, dtype=np.int64) * T
    obs = synth.iid_obs(V, B * T, seed=5)
    h = cv.HMM(pi, a, b)
    got, st, _ = _on_off(h, off, obs, "identical states")
    assert st == dict(engaged=1, certified=0, fallback=B, pinned=1), st
    h.set_tuning(t64_f32ru_first=1)
    again = cv.decode_batch(h, off, obs, dtype="f64", rescore_f64=False)
    assert cv.last_fixed_first_stats(h) == dict(engaged=0, certified=0, fallback=0, pinned=1)
    assert cv.last_first_pass_kind(h) == "none"
    _same(again, got, "identical states, after the guard")


def test_default_key_leaves_small_calls_to_the_integer_pass(gpu, model):
    """t64_f32ru_first at its default and t64_fixed_first = 1: a small call takes the integer pass
    and the integer model's counts hold."""
    pi, a, b = model
    B, T = 40, 24
    off = np.arange(B + 1, dtype=np.int64) * T
    obs = synth.iid_obs(V, B * T, seed=17)
    h = cv.HMM(pi, a, b)
    assert h.tuning("t64_f32ru_first") in (DEFAULT, 0)  # the measured break-even, or off
    h.set_tuning(t64_fixed_first=1)
    got = cv.decode_batch(h, off, obs, dtype="f64", rescore_f64=False)
    st = cv.last_fixed_first_stats(h)
    _, cert, _ = MI.decode(pi, a, b, obs.reshape(B, T).astype(np.int64))
    assert cv.last_first_pass_kind(h) == "fixed"
    assert st == dict(engaged=1, certified=int(cert.sum()), fallback=B - int(cert.sum()), pinned=0), st
    h.set_tuning(t64_fixed_first=0, t64_f32ru_first=0)
    _same(got, cv.decode_batch(h, off, obs, dtype="f64", rescore_f64=False), "integer pass vs the f64 kernels")


def test_chunked_pipeline_and_serial(gpu, model):
    """8,192 sequences of T = 8 under a cap of two chunks of 2,048: four chunks pipelined over two
    streams (t64_fixed_chunks = 8) and the serial schedule (0) agree with the f64 kernels and with
    each other, twice in a row on one handle."""
    B, T = 8192, 8
    off = np.arange(B + 1, dtype=np.int64) * T
    obs = synth.iid_obs(V, B * T, seed=8)
    cap = 2 * 2048 * T * ROW
    hp, hs = cv.HMM(*model), cv.HMM(*model)
    pipe, stp, kind = _on_off(hp, off, obs, "pipelined", cap=cap, chunks=8)
    hp.set_tuning(t64_f32ru_first=1)
    again = _run(hp, off, obs, cap=cap)
    assert cv.last_timing(hp)["launches"] >= 4
    ser, sts, _ = _on_off(hs, off, obs, "serial", cap=cap, chunks=0)
    assert stp == sts == cv.last_fixed_first_stats(hp) and kind == "f32ru", (stp, sts)
    assert stp["engaged"] == 1 and stp["pinned"] == 0 and stp["certified"] > B // 2, stp
    _same(again, pipe, "pipelined: second call")
    _same(ser, pipe, "serial vs pipelined")


def test_one_handle_alternates_between_the_passes(gpu, model):
    """Round-up pass, integer pass, f64 kernels, twice around on one handle; an odd count, so each
    first pass is followed on its stream by the f64 kernels' decode of the unpaired sequence, whose
    bits must be the usual ones: the rounding mode does not outlive the forward's waves."""
    pi, a, b = model
    B, T = 33, 40
    off = np.arange(B + 1, dtype=np.int64) * T
    obs = synth.iid_obs(V, B * T, seed=29)
    h = cv.HMM(pi, a, b)
    h.set_tuning(t64_fixed_chunks=0)  # one stream: bt, score and fallback right behind the forward
    ref = None
    for rnd in range(2):
        for keys, kind in ((dict(t64_f32ru_first=1, t64_fixed_first=0), "f32ru"),
                           (dict(t64_f32ru_first=0, t64_fixed_first=1), "fixed"),
                           (dict(t64_f32ru_first=0, t64_fixed_first=0), "none")):
            h.set_tuning(**keys)
            got = cv.decode_batch(h, off, obs, dtype="f64", rescore_f64=False)
            assert cv.last_first_pass_kind(h) == kind, (rnd, kind)
            if kind != "none":
                assert cv.last_fixed_first_stats(h)["fallback"] >= 1
            ref = ref or got
            _same(got, ref, f"round {rnd}, {kind}")
