"""A catalogue of calls on one cv.HMM handle, for the tests of the state a handle carries from
call to call (tests/test_gpu_handle_reuse.py) and of the call sequence itself
(tests/test_handle_ops.py).  A plain helper module: nothing here is collected by pytest.

An operation is a name and a function (h, inputs) -> tuple of numpy arrays.  A call that raises
cv.CVError returns Failed((status,)) instead, so argument errors are results like any other and
the handle is used again after them.  The inputs of a (model, batch) pair are built once from
seeds; the catalogue of a model holds the operations its N supports by the limits documented in
include/cviterbi.h (f32 trellis and f32 constrained decode: N <= 256; fixed-point first pass:
224 < N <= 256; K-best: N * KT <= 8,192), decided here and not by catching errors.
"""
import functools
import types

import numpy as np

import cviterbi as cv
from cviterbi import _lib as L
from cviterbi import synth

V = 12
IMPOSSIBLE = V - 1  # quantised model: no state emits this observation
NCOMP = 4

# name -> (N, kind): the smallest sizes that reach each kernel family
MODELS = {"n40": (40, "random"), "n256": (256, "random"), "n256q": (256, "quantised"), "n300": (300, "random")}
BATCHES = ("small", "large")


class Failed(tuple):
    """The result of a call that raised cv.CVError: (status array,)."""


@functools.lru_cache(maxsize=None)
def model(name):
    """(pi, a, b) log10 tables of MODELS[name]."""
    n, kind = MODELS[name]
    if kind == "random":
        return synth.random_hmm(n, V, seed=8100 + n)
    # log-probabilities rounded to 1/4 (exact ties everywhere) with 10% -inf, one observation
    # that no state emits (infeasible sequences)
    rng = np.random.default_rng(8200 + n)
    pi = np.round(rng.uniform(-2, 0, n) * 4) / 4
    a = np.round(rng.uniform(-2, 0, (n, n)) * 4) / 4
    b = np.round(rng.uniform(-2, 0, (n, V)) * 4) / 4
    pi[rng.random(n) < 0.1] = -np.inf
    a[rng.random((n, n)) < 0.1] = -np.inf
    b[rng.random((n, V)) < 0.1] = -np.inf
    b[:, IMPOSSIBLE] = -np.inf
    # np.round gives -0.0; the library reads -0.0 as +0.0 (cviterbi.h), the references read what
    # they are given: hand both the canonical table, so that scores of 0 compare byte for byte
    return pi + 0.0, a + 0.0, b + 0.0


def lengths(batch):
    if batch == "small":
        return np.array([0, 1, 2, 9, 5, 1, 17], np.int64)
    rng = np.random.default_rng(8300)
    t = rng.integers(0, 49, size=150).astype(np.int64)
    t[75] = 0   # an empty sequence in the middle
    t[10] = 48  # the longest
    return t


@functools.lru_cache(maxsize=None)
def inputs(name, batch):
    """Everything the operations read, for one (model, batch): arrays only, never changed."""
    n, kind = MODELS[name]
    pi, a, b = model(name)
    t = lengths(batch)
    off = synth.offsets_from_lengths(t)
    total = int(off[-1])
    rng = np.random.default_rng(8400 + n + (1 if batch == "large" else 0))
    obs_ok = rng.integers(0, V - 1, size=total).astype(np.int32)  # feasible: the chain's observations
    obs = obs_ok.copy()
    if kind == "quantised":  # infeasible sequences
        if batch == "small":
            obs[off[3] + 4] = IMPOSSIBLE
        else:
            obs[rng.choice(total, size=5, replace=False)] = IMPOSSIBLE
    # one sequence with an out-of-range observation
    bad_seq = 4 if batch == "small" else int(np.nonzero(t[20:] >= 3)[0][0]) + 20
    obs_bad = obs.copy()
    obs_bad[off[bad_seq] + 2] = V + 3
    forced = np.where(rng.random(total) < 0.2, rng.integers(0, n, size=total), -1).astype(np.int32)
    # about half of the sequences hold one constrained element; the longest holds component 2 twice
    comp = np.full(total, -1, np.int32)
    if batch == "small":
        comp[off[1]], comp[off[3] + 4] = 0, 1  # the one-element sequence; the middle of another
    else:
        for s in range(len(t)):
            if t[s] > 0 and rng.random() < 0.5:
                comp[off[s] + rng.integers(0, t[s])] = rng.integers(0, NCOMP)
    longest = int(np.argmax(t))
    comp[off[longest]:off[longest + 1]] = -1
    comp[off[longest] + 2] = 2
    comp[off[longest] + t[longest] - 4] = 2
    emis = np.ascontiguousarray(b.T[obs])  # E[e][j] = b[j][obs[e]]: the model's own table rows
    return types.SimpleNamespace(model=name, batch=batch, n=n, kind=kind, pi=pi, a=a, b=b, lengths=t, off=off,
                                 total=total, obs=obs, obs_ok=obs_ok, obs_bad=obs_bad, bad_seq=bad_seq, forced=forced,
                                 comp=comp, emis=emis, tmax=int(t.max()), dev={})


def f64_row_bytes(n):
    """Workspace bytes per element of the default f64 viterbi decode: the f64 trellis pads to 64
    states up to N = 256, the generic kernels' rows mode keeps N reals above."""
    return 8 * 64 * ((n + 63) // 64) if n <= 256 else 8 * n


def kbest_width(k):
    return next(w for w in (2, 4, 8, 16) if w >= k)


# ---- device-pointer calls -----------------------------------------------------------------------
_streams = []


def stream(i=0):
    """The i-th non-default torch stream of this process."""
    import torch

    while len(_streams) <= i:
        _streams.append(torch.cuda.Stream(torch.device("cuda", 0)))
    return _streams[i]


def _dev(x, key, arr):
    """arr on the device, uploaded once per inputs object."""
    import torch

    if key not in x.dev:
        x.dev[key] = torch.from_numpy(np.ascontiguousarray(arr)).to(torch.device("cuda", 0))
    return x.dev[key]


def _sentinels(x, rows=None):
    """Output tensors (path, score, status) filled with values no call writes."""
    import torch

    dev = torch.device("cuda", 0)
    nseq = len(x.lengths)
    path = torch.full((x.total,) if rows is None else (rows, x.total), -7, dtype=torch.int32, device=dev)
    score = torch.full((nseq,) if rows is None else (nseq, rows), 7.5, dtype=torch.float64, device=dev)
    status = torch.full((nseq,), 9, dtype=torch.uint8, device=dev)
    return path, score, status


def enqueue_decode_device(h, x, s):
    """cv_decode_batch_device (f64) on torch stream s, one sequence BADOBS; returns the output
    tensors without synchronising."""
    import torch

    outs = _sentinels(x)
    d_off, d_obs = _dev(x, "off", x.off), _dev(x, "obs_bad", x.obs_bad)
    s.wait_stream(torch.cuda.current_stream())
    cv.decode_batch_device(h, d_off, d_obs, *outs, offsets_host=x.off, dtype="f64", stream=s.cuda_stream)
    return outs


def enqueue_kbest_device(h, x, k, s):
    import torch

    path, score, status = _sentinels(x, rows=k)
    count = torch.full((len(x.lengths),), -3, dtype=torch.int32, device=path.device)
    d_off, d_obs = _dev(x, "off", x.off), _dev(x, "obs", x.obs)
    s.wait_stream(torch.cuda.current_stream())
    cv.kbest_batch_device(h, d_off, d_obs, k, path, score, count, status, offsets_host=x.off, stream=s.cuda_stream)
    return path, score, count, status


def fetch(tensors):
    return tuple(t.cpu().numpy().copy() for t in tensors)


def _decode_device(h, x):
    s = stream(0)
    outs = enqueue_decode_device(h, x, s)
    s.synchronize()
    got = fetch(outs)
    assert got[2][x.bad_seq] == L.SEQ_BADOBS, got[2]
    return got


def _kbest_device(k):
    def op(h, x):
        s = stream(0)
        outs = enqueue_kbest_device(h, x, k, s)
        s.synchronize()
        return fetch(outs)
    return op


def _constrained_device(h, x):
    import torch

    outs = _sentinels(x)
    s = stream(0)
    s.wait_stream(torch.cuda.current_stream())
    states, obj = cv.decode_constrained_device(h, x.off, _dev(x, "off", x.off), _dev(x, "obs", x.obs), x.comp, *outs,
                                               ncomp=NCOMP, stream=s.cuda_stream)
    s.synchronize()
    return fetch(outs) + (states, obj)


# ---- host calls ---------------------------------------------------------------------------------
def _decode(dtype, **kw):
    forced = kw.pop("forced", False)

    def op(h, x):
        return cv.decode_batch(h, x.off, x.obs, dtype=dtype, forced=x.forced if forced else None, **kw)
    return op


def _decode_capped(h, x):
    cap = f64_row_bytes(x.n) * -(-x.total // 3)
    out = cv.decode_batch(h, x.off, x.obs, dtype="f64", workspace_bytes=cap)
    assert cv.last_timing(h)["launches"] >= 3, cv.last_timing(h)
    return out


def _fixed_first(value):
    def op(h, x):
        with h.tuned(t64_fixed_first=value):
            return cv.decode_batch(h, x.off, x.obs, dtype="f64")
    return op


def _kbest(k, forced=False):
    def op(h, x):
        return cv.kbest_batch(h, x.off, x.obs, k, forced=x.forced if forced else None)
    return op


def _chain(**keys):
    def op(h, x):
        with h.tuned(**keys):
            path, obj = cv.decode_superseq_cp(h, x.off, x.obs_ok)
            stats = cv.last_superseq_stats(h)
        if keys.get("chain_spec") == 1:
            assert stats["spec_batches"] >= 1, stats
        if keys.get("chain_par") == 0:
            assert not stats["parallel"], stats
        return path, obj
    return op


def _kbest_nomem(h, x):
    need = x.tmax * x.n * kbest_width(3) * 2  # the longest sequence's u16 back-pointers
    return cv.kbest_batch(h, x.off, x.obs, 3, workspace_bytes=need - 2)


# the calls that must fail, with the status they fail with: argument errors the library rejects
# on the host before any kernel runs
EXPECT_FAIL = {"bad_obs_einval": L.CV_EINVAL, "kbest_enomem": L.CV_ENOMEM, "kbest_k17_einval": L.CV_EINVAL}
# decode_batch-style entries: cv.last_timing(h)["kernel"] names the kernel family of the call
DECODE_OPS = ("f64_viterbi", "f64_cp", "f64_dp", "f64_decode", "f64_forced", "f64_generic", "f64_capped",
              "f32_trellis", "f32_nowave", "f32_generic", "f64_fixed_first_1", "f64_fixed_first_0", "emis_decode")
F64_ASSOC = {"f64_viterbi": "viterbi", "f64_cp": "cp", "f64_dp": "dp", "f64_decode": "decode"}


@functools.lru_cache(maxsize=None)
def catalogue(name):
    """The ordered (op name, function) pairs of a model."""
    n = MODELS[name][0]
    ops = [(k, _decode("f64", assoc=v)) for k, v in F64_ASSOC.items()]
    ops += [("f64_forced", _decode("f64", forced=True)),
            ("f64_generic", _decode("f64", kernel="generic")),
            ("f64_capped", _decode_capped)]
    if n <= 256:
        ops += [("f32_trellis", _decode("f32", kernel="trellis", rescore_f64=False)),
                ("f32_nowave", _decode("f32", kernel="trellis", variant="nowave"))]
    ops += [("f32_generic", _decode("f32", kernel="generic", rescore_f64=False))]
    if 224 < n <= 256:
        ops += [("f64_fixed_first_1", _fixed_first(1)), ("f64_fixed_first_0", _fixed_first(0))]
    ops += [("device_decode", _decode_device),
            ("kbest3", _kbest(3)), ("kbest8", _kbest(8)), ("kbest3_forced", _kbest(3, forced=True)),
            ("kbest3_device", _kbest_device(3)),
            ("posterior_gamma", lambda h, x: cv.posterior_batch(h, x.off, x.obs, gamma=True)),
            ("score", lambda h, x: cv.score_batch(h, x.off, x.obs)),
            ("posterior_forced", lambda h, x: cv.posterior_batch(h, x.off, x.obs, forced=x.forced)),
            ("emis_decode", lambda h, x: cv.decode_emissions(h, x.off, x.emis)),
            ("emis_posterior_gamma", lambda h, x: cv.posterior_emissions(h, x.off, x.emis, gamma=True)),
            ("emis_score", lambda h, x: cv.score_emissions(h, x.off, x.emis)),
            ("constrained_f64", lambda h, x: cv.decode_constrained(h, x.off, x.obs, x.comp, ncomp=NCOMP))]
    if n <= 256:
        ops += [("constrained_f32", lambda h, x: cv.decode_constrained(h, x.off, x.obs, x.comp, ncomp=NCOMP,
                                                                       dtype="f32"))]
    ops += [("constrained_device", _constrained_device),
            ("chain", _chain()),
            ("chain_spec", _chain(chain_par_force=2, chain_spec=1)),
            ("chain_serial", _chain(chain_par=0)),
            ("bad_obs_einval", lambda h, x: cv.decode_batch(h, x.off, x.obs_bad, dtype="f64")),
            ("kbest_enomem", _kbest_nomem),
            ("kbest_k17_einval", lambda h, x: cv.kbest_batch(h, x.off, x.obs, 17))]
    assert n * kbest_width(8) <= 8192  # the K-best limit N * KT <= 8,192 holds for every model at K = 8
    return tuple(ops)


def op_names(name):
    return tuple(k for k, _ in catalogue(name))


def run(name, op, h, batch):
    """One call of the model's operation `op` on handle h -> tuple of arrays (Failed on CVError)."""
    fn = dict(catalogue(name))[op]
    try:
        out = fn(h, inputs(name, batch))
    except cv.CVError as e:
        if e.status in (L.CV_EDEVICE, L.CV_EINTERNAL, L.CV_EIO):  # not a verdict on the arguments: let it show
            raise
        return Failed((np.array([e.status], np.int32),))
    return tuple(np.asarray(v) for v in out if v is not None)


def new_handle(name):
    return cv.HMM(*model(name), device=0)


def first_difference(got, ref):
    """None when the two results are the same bytes (type, dtype and shape too), else a
    description naming the first differing output and index."""
    if type(got) is not type(ref):
        return f"{type(got).__name__} {[v.tolist() for v in got][:1]} where {type(ref).__name__} is expected"
    if len(got) != len(ref):
        return f"{len(got)} outputs, expected {len(ref)}"
    for k, (g, r) in enumerate(zip(got, ref)):
        if g.dtype != r.dtype or g.shape != r.shape:
            return f"output {k}: {g.dtype}{g.shape}, expected {r.dtype}{r.shape}"
        if g.tobytes() != r.tobytes():
            gb = np.ascontiguousarray(g).reshape(-1).view(np.uint8).reshape(g.size, -1)
            rb = np.ascontiguousarray(r).reshape(-1).view(np.uint8).reshape(r.size, -1)
            i = int(np.nonzero((gb != rb).any(axis=1))[0][0])
            return (f"output {k}: first difference at flat index {i} of {g.size}: {g.reshape(-1)[i]!r}, "
                    f"expected {r.reshape(-1)[i]!r}")
    return None


# ---- the call sequence that makes every ordered pair of operations adjacent -----------------------
def pair_circuit(n):
    """An Eulerian circuit of the complete digraph with loops on n vertices (Hierholzer, out-edges
    taken in index order): n * n + 1 vertices in which every ordered pair (x, y), x = y included,
    is adjacent exactly once."""
    nxt = [0] * n
    stack, circuit = [0], []
    while stack:
        v = stack[-1]
        if nxt[v] < n:
            nxt[v] += 1
            stack.append(nxt[v] - 1)
        else:
            circuit.append(stack.pop())
    circuit.reverse()
    return circuit


SEGMENT_CALLS = 240  # pairs per test case: a few seconds of small calls


def circuit_segments(n):
    """The circuit cut into consecutive runs of at most SEGMENT_CALLS pairs.  A segment after the
    first starts with the previous segment's last vertex (one warming call), so no pair is lost."""
    c = pair_circuit(n)
    return [c[s:s + SEGMENT_CALLS + 1] for s in range(0, len(c) - 1, SEGMENT_CALLS)]
