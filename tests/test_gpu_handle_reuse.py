"""GPU: one cv.HMM handle across interleaved entry points and workspace release.

A handle (struct cv_hmm, csrc/handle.hpp) carries lazily built tables, grow-only workspaces
shared by unrelated kernels, device counters a call must reset itself, sticky guards and the
events that order calls on different streams ("Handle state between calls").  Here
every call on a reused handle must return the bytes the same call returns on a FRESH handle that
makes that one call and nothing else -- paths, scores, statuses, log-likelihoods and gamma alike
(no kernel accumulates floats with atomics) -- and release / destroy must give the device memory
back.  The catalogue of calls, the four models and the two batches are tests/handle_ops.py's.
"""
import gc

import numpy as np
import pytest

import c_oracle as O
import cviterbi as cv
import emis_ref
import handle_ops as H
import kbest_ref

pytestmark = pytest.mark.gpu

MODELS = list(H.MODELS)
MODEL_OPS = [(m, op) for m in MODELS for op in H.op_names(m)]
ASSOC = {"viterbi": O.VITERBI, "cp": O.CP, "dp": O.DP, "decode": O.DECODE}

_REF = {}


def reference(model, batch, op):
    """(result, kernel, agrees): the call on a fresh handle that does nothing else; the kernel
    family cv.last_timing names for the decode entries; whether a second fresh handle returned
    the same bytes.  Computed once per key and never changed."""
    key = (model, batch, op)
    if key not in _REF:
        runs = []
        for _ in range(2):
            h = H.new_handle(model)
            out = H.run(model, op, h, batch)
            kernel = cv.last_timing(h)["kernel"] if op in H.DECODE_OPS else None
            runs.append((out, kernel))
            del h
        _REF[key] = (runs[0][0], runs[0][1], H.first_difference(runs[1][0], runs[0][0]) is None
                     and runs[0][1] == runs[1][1])
    return _REF[key]


def check(model, batch, op, got, before, where):
    ref = reference(model, batch, op)[0]
    d = H.first_difference(got, ref)
    assert d is None, f"{model}/{batch}: {op} after {before} ({where}) differs from a fresh handle: {d}"


# ---- the references themselves --------------------------------------------------------------------
@pytest.mark.parametrize("batch", H.BATCHES)
@pytest.mark.parametrize("model", MODELS)
def test_fresh_handles_agree(gpu, model, batch):
    """Byte equality needs run-to-run determinism: two fresh handles return the same bytes for
    every operation, and the calls that must fail fail with their documented status."""
    loose = [op for op in H.op_names(model) if not reference(model, batch, op)[2]]
    assert not loose, f"{model}/{batch}: not reproducible between two fresh handles: {loose}"
    for op in H.op_names(model):
        ref = reference(model, batch, op)[0]
        if op in H.EXPECT_FAIL:
            assert isinstance(ref, H.Failed) and ref[0].tolist() == [H.EXPECT_FAIL[op]], (op, ref)
        else:
            assert not isinstance(ref, H.Failed), (op, ref)


def _same(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (
            f"{what}: output {k} differs at {np.nonzero(np.atleast_1d(g != w))[0][:8]}")


@pytest.mark.parametrize("batch", H.BATCHES)
@pytest.mark.parametrize("model", MODELS)
def test_anchor_decodes_equal_the_oracle(gpu, model, batch):
    """"Equal to a fresh handle" must not mean "equally wrong": the fresh-handle decodes equal
    the C oracle for their association and precision, forced tags included."""
    x = H.inputs(model, batch)
    ops = H.op_names(model)
    f64 = {a: O.decode_batch(x.pi, x.a, x.b, x.off, x.obs, ASSOC[a], np.float64) for a in ASSOC}
    for op, assoc in H.F64_ASSOC.items():
        _same(reference(model, batch, op)[0], f64[assoc], f"{model}/{batch} {op}")
    for op in ("f64_generic", "f64_capped", "f64_fixed_first_1", "f64_fixed_first_0"):
        if op in ops:
            _same(reference(model, batch, op)[0], f64["viterbi"], f"{model}/{batch} {op}")
    _same(reference(model, batch, "f64_forced")[0],
          O.decode_batch(x.pi, x.a, x.b, x.off, x.obs, O.VITERBI, np.float64, forced=x.forced), f"{model}/{batch} forced")
    f32 = O.decode_batch(x.pi, x.a, x.b, x.off, x.obs, O.VITERBI, np.float32)
    for op in ("f32_trellis", "f32_generic"):  # the kernels' own scores
        if op in ops:
            _same(reference(model, batch, op)[0], f32, f"{model}/{batch} {op}")
    if "f32_nowave" in ops:  # f64 re-score of the f32 path
        p, s, st = reference(model, batch, "f32_nowave")[0]
        _same((p, st), (f32[0], f32[2]), f"{model}/{batch} f32_nowave")
        ok = st == 0
        assert np.array_equal(s[ok], O.rescore_batch_f64(x.pi, x.a, x.b, x.off, x.obs, p)[ok])
    # the device entry: the bad sequence aside, the oracle's results
    p, s, st = reference(model, batch, "device_decode")[0]
    good = np.arange(len(st)) != x.bad_seq
    elems = np.ones(x.total, bool)
    elems[x.off[x.bad_seq]:x.off[x.bad_seq + 1]] = False
    _same((p[elems], s[good], st[good]), (f64["viterbi"][0][elems], f64["viterbi"][1][good], f64["viterbi"][2][good]),
          f"{model}/{batch} device_decode")
    # dense emissions equal to the model's own rows: the discrete decode, bit for bit, and the
    # oracle on the discrete model emis_ref builds from them
    _same(reference(model, batch, "emis_decode")[0], reference(model, batch, "f64_viterbi")[0], "emissions vs discrete")
    bd, od = emis_ref.as_discrete(x.emis, x.n)
    _same(reference(model, batch, "emis_decode")[0], O.decode_batch(x.pi, x.a, bd, x.off, od, O.VITERBI, np.float64),
          f"{model}/{batch} emis_decode")


@pytest.mark.parametrize("batch", H.BATCHES)
@pytest.mark.parametrize("model", MODELS)
def test_anchor_chain_equals_the_oracle(gpu, model, batch):
    x = H.inputs(model, batch)
    rp, robj = O.cp_superseq_f64(x.pi, x.a, x.b, x.off, x.obs_ok)
    for op in ("chain", "chain_spec"):
        _same(reference(model, batch, op)[0], (rp, np.asarray(robj)), f"{model}/{batch} {op}")


@pytest.mark.parametrize("model", MODELS)
def test_anchor_kbest_equals_the_specification(gpu, model):
    """The numpy specification on the first 5 sequences of the small batch (it takes seconds per
    sequence of the large one); on the large batch rank 0 is the f64 decode, which the oracle
    anchors above."""
    x = H.inputs(model, "small")
    for op, k in (("kbest3", 3), ("kbest8", 8)):
        paths, scores, count, status = reference(model, "small", op)[0]
        for s in range(5):
            lo, hi = x.off[s], x.off[s + 1]
            rp, rs, rc = kbest_ref.kbest_ref(x.pi, x.a, x.b, x.obs[lo:hi], k)
            assert count[s] == rc and np.array_equal(paths[:, lo:hi], rp), (model, op, s)
            assert scores[s].tobytes() == rs.tobytes(), (model, op, s)
        x2 = H.inputs(model, "large")
        paths, scores, count, status = reference(model, "large", op)[0]
        dp, ds, dst = reference(model, "large", "f64_viterbi")[0]
        ok = dst == 0
        assert np.array_equal(status, dst) and np.array_equal(scores[ok, 0], ds[ok]), (model, op)
        feasible = np.repeat(ok, x2.lengths)
        assert np.array_equal(paths[0][feasible], dp[feasible]), (model, op)
    for batch in H.BATCHES:  # the device variant is documented bit-identical to the host one
        _same(reference(model, batch, "kbest3_device")[0], reference(model, batch, "kbest3")[0],
              f"{model}/{batch} kbest3 device vs host")


# ---- (b) every ordered pair of operations, adjacent on one handle ---------------------------------
SEGMENTS = [(m, i) for m in MODELS for i in range(len(H.circuit_segments(len(H.op_names(m)))))]


@pytest.mark.parametrize("model,segment", SEGMENTS)
def test_every_ordered_pair(gpu, model, segment):
    ops = H.op_names(model)
    seq = H.circuit_segments(len(ops))[segment]
    h = H.new_handle(model)
    before = "a fresh handle"
    for pos, i in enumerate(seq):
        got = H.run(model, ops[i], h, "small")
        check(model, "small", ops[i], got, before, f"call {pos} of segment {segment}")
        before = ops[i]


# ---- (c) large, then small, then large --------------------------------------------------------------
@pytest.mark.parametrize("model,op", MODEL_OPS)
def test_large_small_large(gpu, model, op):
    """Stale tails of grow-only buffers and order arrays: the small call runs in buffers the large
    one left, and the second large call in what the small one rewrote."""
    h = H.new_handle(model)
    before = "a fresh handle"
    for batch in ("large", "small", "large"):
        check(model, batch, op, H.run(model, op, h, batch), before, "large-small-large")
        before = f"{op} on {batch}"


def test_sticky_guards_trip_and_change_no_result(gpu):
    """The quantised model is there so that the handle's two sticky guards trip in mid-sequence
    (cviterbi.h, tuning keys t64_lo_every and t64_fixed_first): its large batch replays rows
    densely more than once per 64 sequences, so the handle runs full rows from then on, and the
    fixed-point pass certifies fewer than 7 in 8 of its sequences, so the handle stays on the f64
    kernels.  Both show in the stats of the calls that follow, neither in a result or in the
    kernel family; the random model of the same size trips neither."""
    for model, trips in (("n256q", True), ("n256", False)):
        h = H.new_handle(model)
        lo_every = []
        for batch in ("small", "large", "small"):
            check(model, batch, "f64_viterbi", H.run(model, "f64_viterbi", h, batch), "f64_viterbi", "guard t64_lo_off")
            stats = cv.last_t64_stats(h)
            lo_every.append(stats["lo_every"])
            if batch == "large":  # the guard's own condition, on this call's counters
                assert (stats["overflows"] * 64 > stats["sequences"]) == trips, (model, stats)
        assert lo_every == ([8, 8, 1] if trips else [8, 8, 8]), (model, lo_every)
        seen = []  # (engaged, pinned) of each call
        for batch in ("small", "large", "small", "large"):
            got = H.run(model, "f64_fixed_first_1", h, batch)
            check(model, batch, "f64_fixed_first_1", got, "f64_fixed_first_1", "guard fx_pinned")
            assert cv.last_timing(h)["kernel"] == reference(model, batch, "f64_fixed_first_1")[1]
            fx = cv.last_fixed_first_stats(h)
            seen.append((fx["engaged"], fx["pinned"]))
        assert seen == ([(1, 0), (1, 1), (0, 1), (0, 1)] if trips else [(1, 0)] * 4), (model, seen)
        # the guards are the handle's: the other entries go on returning the fresh handle's bytes
        for op in ("f64_viterbi", "f64_capped", "device_decode", "emis_decode", "chain"):
            check(model, "large", op, H.run(model, op, h, "large"), "both guards tripped", "after the guards")


# ---- (d) release in between ---------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_release_between_calls(gpu, model):
    """60 pseudo-random (operation, batch) calls with release_workspaces() after every third: the
    results stay the fresh handle's, and the lazily built tables survive (the decode entries keep
    their kernel family)."""
    ops = H.op_names(model)
    rng = np.random.default_rng(8500 + H.MODELS[model][0])
    h = H.new_handle(model)
    before = "a fresh handle"
    for call in range(60):
        op, batch = ops[rng.integers(len(ops))], H.BATCHES[rng.integers(2)]
        got = H.run(model, op, h, batch)
        check(model, batch, op, got, before, f"call {call}, release after every third")
        if op in H.DECODE_OPS:
            assert cv.last_timing(h)["kernel"] == reference(model, batch, op)[1], (model, batch, op, before)
        before = f"{op} on {batch}"
        if call % 3 == 2:
            h.release_workspaces()
            before += " and a release"


# ---- (e) release gives the memory back -------------------------------------------------------------------
@pytest.mark.parametrize("model,op", MODEL_OPS)
def test_release_returns_the_workspaces(gpu, model, op):
    """After the tables exist, whatever a larger call allocates is a workspace, and
    release_workspaces() frees it: the library's device bytes are back where they were."""
    h = H.new_handle(model)
    H.run(model, op, h, "small")  # builds the tables
    h.release_workspaces()
    before = cv.device_memory()["current"]
    H.run(model, op, h, "large")
    held = cv.device_memory()["current"]
    h.release_workspaces()
    after = cv.device_memory()["current"]
    assert after == before, (f"{model}: {op} on the large batch left {after - before} bytes after "
                             f"release_workspaces() ({held - before} held before it)")


# ---- (f) destroy gives everything back ----------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_destroy_returns_everything(gpu, model):
    gc.collect()
    before = cv.device_memory()["current"]
    h = H.new_handle(model)
    for op in H.op_names(model):
        H.run(model, op, h, "small")
    assert cv.device_memory()["current"] > before
    del h
    gc.collect()
    after = cv.device_memory()["current"]
    assert after == before, f"{model}: {after - before} bytes left after the handle was destroyed"


# ---- (g) two streams, one handle ---------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["decode_first", "kbest_first"])
def test_two_streams_one_handle(gpu, order):
    """The f64 device decode of the large batch on one stream and the K-best device call of the
    small batch on another, enqueued with no synchronisation in between (the second waits on its
    own stream for the first's workspace, ws_done): both results are the fresh handle's."""
    import torch

    model = "n256"
    h = H.new_handle(model)
    large, small = H.inputs(model, "large"), H.inputs(model, "small")
    sx, sy = H.stream(1), H.stream(2)
    torch.cuda.synchronize()
    if order == "decode_first":
        x = H.enqueue_decode_device(h, large, sx)
        y = H.enqueue_kbest_device(h, small, 3, sy)
    else:
        y = H.enqueue_kbest_device(h, small, 3, sy)
        x = H.enqueue_decode_device(h, large, sx)
    torch.cuda.synchronize()
    other = {"decode_first": ("a fresh handle", "device_decode on large"),
             "kbest_first": ("kbest3_device on small", "a fresh handle")}[order]
    check(model, "large", "device_decode", H.fetch(x), other[0], "two streams")
    check(model, "small", "kbest3_device", H.fetch(y), other[1], "two streams")


@pytest.mark.parametrize("call", ["device_decode", "kbest3_device"])
def test_release_behind_a_device_call(gpu, call):
    """release_workspaces() right behind a *_device call enqueued on the caller's stream, with no
    synchronisation by the caller: it waits for that call's end (ws_done) before it frees the
    rows the call is still using (cviterbi.h), the result is the fresh handle's, the memory is
    back, and so is the next call's result."""
    import torch

    model = "n256"
    h = H.new_handle(model)
    large = H.inputs(model, "large")
    H.run(model, call, h, "small")  # the tables
    h.release_workspaces()
    before = cv.device_memory()["current"]
    torch.cuda.synchronize()
    s = H.stream(1)
    if call == "device_decode":
        out = H.enqueue_decode_device(h, large, s)
    else:
        out = H.enqueue_kbest_device(h, large, 3, s)
    h.release_workspaces()
    assert cv.device_memory()["current"] == before
    s.synchronize()
    check(model, "large", call, H.fetch(out), "a release", "release behind the call")
    check(model, "large", call, H.run(model, call, h, "large"), f"{call} and a release in flight", "next call")
