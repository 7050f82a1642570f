"""GPU: cv_decode_emissions / cv_decode_emissions_device (the exact-f64 decode of caller-supplied
emission scores) against the C oracle on the equivalent discrete model (tests/emis_ref.py) and
against the product's own discrete decode of that model, bit for bit: no tolerance anywhere.
The shapes are the edges of the staging (every table stride, row strides and alignments, chunk
boundaries, the batch layouts of the f64 trellis), not the workload."""
import functools

import numpy as np
import pytest
import torch

import c_oracle
import cviterbi as cv
from cviterbi import _lib as L
from emis_ref import LENGTHS, as_discrete, model, offsets_of, scores

pytestmark = pytest.mark.gpu

ASSOCS = {"viterbi": c_oracle.VITERBI, "cp": c_oracle.CP, "dp": c_oracle.DP, "decode": c_oracle.DECODE}


def assert_same(got, ref, what=""):
    for name, x, y in zip(("path", "score", "status"), got, ref):
        assert x.shape == y.shape and x.dtype == y.dtype, (what, name, x.shape, y.shape, x.dtype, y.dtype)
        assert np.array_equal(x, y, equal_nan=True), (what, name, np.argwhere(x != y)[:5])


@functools.lru_cache(maxsize=None)
def case(N, lengths=tuple(LENGTHS)):
    """(pi, a, b0, off, E) -- shared by the tests and never modified (copy before editing)."""
    pi, a, b0 = model(N)
    off, E = scores(N, list(lengths), dead=2 if len(lengths) > 2 else None)
    E.setflags(write=False)
    return pi, a, b0, off, E


@functools.lru_cache(maxsize=None)
def oracle(N, assoc, lengths=tuple(LENGTHS)):
    pi, a, _, off, E = case(N, lengths)
    b, obs = as_discrete(E, N)
    return c_oracle.decode_batch(pi, a, b, off, obs, ASSOCS[assoc])


def on_device(h, off, E_dev, **kw):
    """decode_emissions_device on a torch tensor (or a strided view of one) -> numpy results."""
    dev = E_dev.device
    total, nseq = int(off[-1]), len(off) - 1
    off_d = torch.from_numpy(np.ascontiguousarray(off)).to(dev)
    path = torch.full((max(total, 1),), -7, dtype=torch.int32, device=dev)
    score = torch.full((max(nseq, 1),), 77.0, dtype=torch.float64, device=dev)
    status = torch.full((max(nseq, 1),), 9, dtype=torch.uint8, device=dev)
    forced = kw.pop("forced", None)
    if forced is not None:
        kw["forced_dev"] = torch.from_numpy(np.ascontiguousarray(forced, np.int32)).to(dev)
    torch.cuda.synchronize(dev)
    cv.decode_emissions_device(h, off_d, E_dev, path, score, status, offsets_host=off, **kw)
    torch.cuda.synchronize(dev)
    return path.cpu().numpy()[:total], score.cpu().numpy()[:nseq], status.cpu().numpy()[:nseq]


def discrete_on_device(h, off, obs, dev, **kw):
    """cv.decode_batch_device of a discrete model (it range-checks obs on the device)."""
    total, nseq = int(off[-1]), len(off) - 1
    off_d = torch.from_numpy(np.ascontiguousarray(off)).to(dev)
    obs_d = torch.from_numpy(np.ascontiguousarray(obs, np.int32)).to(dev)
    path = torch.zeros(max(total, 1), dtype=torch.int32, device=dev)
    score = torch.zeros(max(nseq, 1), dtype=torch.float64, device=dev)
    status = torch.zeros(max(nseq, 1), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    cv.decode_batch_device(h, off_d, obs_d, path, score, status, offsets_host=off, dtype="f64", **kw)
    torch.cuda.synchronize(dev)
    return path.cpu().numpy()[:total], score.cpu().numpy()[:nseq], status.cpu().numpy()[:nseq]


def expected_kernel(N, kernel):
    """(kernel, padded states) cv_last_timing reports for these small batches."""
    if kernel == "generic" or (kernel == "auto" and N > 256):
        return "generic", 0
    return "trellis_f64", 64 * ((N + 63) // 64) if N <= 256 else 512 if N <= 512 else 1024


def check_timing(h, N, kernel, what):
    t = cv.last_timing(h)
    assert (t["kernel"], t["padded_states"]) == expected_kernel(N, kernel), (what, t)
    assert t["launches"] >= 1 and t["total_ms"] > 0, (what, t)
    return t


# ---- 1. against the oracle, every stride class -------------------------------------------------
def _grid():
    out = []
    for N in (1, 3, 47, 48, 49, 64, 65, 130, 256, 257):
        kernels = ["auto", "generic"] + (["trellis_f64"] if N in (130, 256, 257) else [])
        for assoc in (ASSOCS if N in (3, 65, 257) else ["viterbi"]):
            for kernel in kernels:
                if not (N == 257 and kernel == "trellis_f64" and assoc == "cp"):
                    out.append((N, kernel, assoc))
    return out


@pytest.mark.parametrize("N,kernel,assoc", _grid())
def test_matches_the_oracle(gpu, N, kernel, assoc):
    pi, a, b0, off, E = case(N)
    ref = oracle(N, assoc)
    assert ref[2][2] == L.SEQ_INFEASIBLE and ref[2][4] == L.SEQ_EMPTY
    h = cv.HMM(pi, a, b0, device=gpu)
    what = (N, kernel, assoc)
    assert_same(cv.decode_emissions(h, off, E, assoc=assoc, kernel=kernel), ref, what)
    check_timing(h, N, kernel, what)
    E_dev = torch.from_numpy(np.array(E)).to(f"cuda:{gpu}")
    assert_same(on_device(h, off, E_dev, assoc=assoc, kernel=kernel), ref, what)
    check_timing(h, N, kernel, what)


def test_cp_on_the_pair_trellis_is_unsupported_like_the_discrete_decode(gpu):
    pi, a, b0, off, E = case(257)
    h = cv.HMM(pi, a, b0, device=gpu)
    with pytest.raises(cv.CVError) as e:
        cv.decode_emissions(h, off, E, assoc="cp", kernel="trellis_f64")
    assert e.value.status == L.CV_EUNSUPPORTED
    with pytest.raises(cv.CVError) as e:
        cv.decode_batch(h, [0, 1], np.zeros(1, np.int32), dtype="f64", assoc="cp", kernel="trellis_f64")
    assert e.value.status == L.CV_EUNSUPPORTED


@pytest.mark.parametrize("N,kernel", [(513, "trellis_f64"), (1100, "auto")])
def test_quads_and_the_wide_kernels(gpu, N, kernel):
    lengths = (5, 1)
    pi, a, b0, off, E = case(N, lengths)
    h = cv.HMM(pi, a, b0, device=gpu)
    ref = oracle(N, "viterbi", lengths)
    assert_same(cv.decode_emissions(h, off, E, kernel=kernel, ), ref, (N, kernel))
    t = check_timing(h, N, kernel, (N, kernel))
    if N == 1100:
        assert t["seqs_per_wave"] == 0, t  # GENERIC: 0 = the wide kernels


# ---- 2. row stride and column padding ----------------------------------------------------------
def _strided_views(E, N, xp_full, addr):
    """The same scores behind four layouts: (name, 2-D view, row stride in doubles)."""
    rows = len(E)
    out = [("ld = N", xp_full((rows, N)), N)]
    out.append(("ld = N + 3, NaN beyond N", xp_full((rows, N + 3))[:, :N], N + 3))
    out.append(("ld = 128", xp_full((rows, 128))[:, :N], 128))
    flat = xp_full((rows * (N + 3) + 2,))
    start = 0 if addr(flat) % 16 == 8 else 1
    shifted = flat[start:start + rows * (N + 3)].reshape(rows, N + 3)[:, :N]
    assert addr(shifted) % 16 == 8
    out.append(("base 8 bytes off 16-byte alignment", shifted, N + 3))
    return out


def test_row_stride_and_column_padding(gpu):
    N = 65
    pi, a, b0, off, E = case(N)
    h = cv.HMM(pi, a, b0, device=gpu)
    ref = oracle(N, "viterbi")
    dev = f"cuda:{gpu}"
    E_t = torch.from_numpy(np.array(E))
    host = _strided_views(E, N, lambda shape: np.full(shape, np.nan), lambda x: x.ctypes.data)
    device = _strided_views(E, N, lambda shape: torch.full(shape, float("nan"), dtype=torch.float64, device=dev),
                            lambda x: x.data_ptr())
    for kernel in ("auto", "generic"):  # table stride 128 (16-byte stores) and 65 (8-byte stores)
        for name, view, ld in host:
            view[...] = E
            assert view.strides[0] == 8 * ld
            assert_same(cv.decode_emissions(h, off, view, kernel=kernel), ref, ("host", kernel, name))
        for name, view, ld in device:
            view.copy_(E_t)
            assert view.stride(0) == ld and view.stride(1) == 1
            assert_same(on_device(h, off, view, kernel=kernel), ref, ("device", kernel, name))


# ---- 3. chunking -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ragged600():
    N = 65
    lengths = tuple((7 * k) % 6 for k in range(600))
    return N, lengths, case(N, lengths)


@pytest.mark.parametrize("kernel", ["auto", "generic"])
@pytest.mark.parametrize("assoc", ["viterbi", "decode", "dp", "cp"])
def test_chunks_give_the_one_chunk_result(gpu, assoc, kernel):
    """Each chunk's rows are staged for that chunk alone and its backtrack (DECODE, DP and the
    generic rows mode read them again) runs before they go; the generic kernels overlap the
    next chunk's staging and forward pass with it out of the other half of the workspace."""
    N, lengths, (pi, a, b0, off, E) = ragged600()
    h = cv.HMM(pi, a, b0, device=gpu)
    one = cv.decode_emissions(h, off, E, assoc=assoc, kernel=kernel)
    assert cv.last_timing(h)["launches"] == 1
    assert_same(one, oracle(N, assoc, lengths), (assoc, kernel, "oracle"))
    # rows + staged scores + index: at most 2 * 8 * 128 + 4 bytes per element (the f64 trellis);
    # room for ~300 of the 1,500 elements (the overlapped generic path halves the cap)
    cap = 300 * (2 * 8 * 128 + 4)
    many = cv.decode_emissions(h, off, E, assoc=assoc, kernel=kernel, workspace_bytes=cap)
    t = cv.last_timing(h)
    assert t["launches"] >= 3, t
    assert_same(many, one, (assoc, kernel, "chunked"))
    with h.tuned(emis_overlap=1):  # the f64 trellis stages the next chunk beside the forward pass, out of
        # a second staging buffer under the same cap: at least as many chunks, the same result
        beside = cv.decode_emissions(h, off, E, assoc=assoc, kernel=kernel, workspace_bytes=cap)
        assert cv.last_timing(h)["launches"] >= t["launches"]
        assert_same(beside, one, (assoc, kernel, "chunked, staged beside the forward pass"))
        # a batch that fits one chunk with one staging buffer is not split to make room for a second
        fits = int(off[-1]) * (2 * 8 * 128 + 4)
        assert_same(cv.decode_emissions(h, off, E, assoc=assoc, kernel="auto", workspace_bytes=fits), one, "fits")
        assert cv.last_timing(h)["launches"] == 1
    b, obs = as_discrete(E, N)
    hd = cv.HMM(pi, a, b, device=gpu)
    assert_same(many, cv.decode_batch(hd, off, obs, dtype="f64", assoc=assoc, kernel=kernel), (assoc, kernel, "discrete"))


# ---- 4. forced tags ----------------------------------------------------------------------------
@pytest.mark.parametrize("N", [3, 65, 257])
def test_forced_tags(gpu, N):
    pi, a, b0, off, E0 = case(N)
    E = np.array(E0)
    rng = np.random.default_rng(N)
    forced = np.full(int(off[-1]), -1, np.int32)
    dead_state = int(rng.integers(0, N))
    E[off[0] + 10, dead_state] = -np.inf  # a tag whose emission is -inf: the sequence is infeasible
    forced[off[0] + 10] = dead_state
    for t in (0, 20, 63):  # tags the last sequence can honour
        E[off[5] + t, t % N] = 0.5
        forced[off[5] + t] = t % N
    forced[off[3] + 2] = N - 1
    b, obs = as_discrete(E, N)
    ref = c_oracle.decode_batch(pi, a, b, off, obs, c_oracle.VITERBI, forced=forced)
    assert ref[2][0] == L.SEQ_INFEASIBLE
    if ref[2][5] == L.SEQ_OK:
        assert all(ref[0][off[5] + t] == t % N for t in (0, 20, 63))
    h = cv.HMM(pi, a, b0, device=gpu)
    E_dev = torch.from_numpy(E).to(f"cuda:{gpu}")
    for kernel in ["auto", "generic"] + (["trellis_f64"] if N == 257 else []):
        assert_same(cv.decode_emissions(h, off, E, kernel=kernel, forced=forced), ref, (N, kernel, "host"))
        check_timing(h, N, kernel, (N, kernel))
        assert_same(on_device(h, off, E_dev, kernel=kernel, forced=forced), ref, (N, kernel, "device"))


# ---- 5. validation -----------------------------------------------------------------------------
@pytest.mark.parametrize("N", [65, 257])
def test_nan_and_plus_inf_flag_their_sequence_only(gpu, N):
    pi, a, b0, off, E0 = case(N)
    h = cv.HMM(pi, a, b0, device=gpu)
    b, obs = as_discrete(E0, N)
    hd = cv.HMM(pi, a, b, device=gpu)
    dev = f"cuda:{gpu}"
    bad = np.array(E0)
    bad[off[0] + 7, 3] = np.nan
    bad[off[5] + 1, N - 1] = np.inf
    bad_obs = obs.copy()
    bad_obs[off[0] + 7] = len(obs)  # out of range: BADOBS in the discrete decode
    bad_obs[off[5] + 1] = -1
    for kernel in ["auto", "generic"] + (["trellis_f64"] if N == 257 else []):
        clean = cv.decode_emissions(h, off, E0, kernel=kernel)
        assert_same(clean, oracle(N, "viterbi"), (N, kernel, "clean"))
        want = discrete_on_device(hd, off, bad_obs, dev, kernel=kernel)
        assert list(want[2][[0, 5]]) == [L.SEQ_BADOBS, L.SEQ_BADOBS]
        keep = np.ones(len(obs), bool)
        for s in (0, 5):
            keep[off[s]:off[s + 1]] = False
        assert np.array_equal(want[0][keep], clean[0][keep])  # the reference itself is sound
        for got in (cv.decode_emissions(h, off, bad, kernel=kernel),
                    on_device(h, off, torch.from_numpy(bad).to(dev), kernel=kernel)):
            assert_same(got, want, (N, kernel, "bad entries"))
            assert np.array_equal(got[0][keep], clean[0][keep])
            others = [1, 2, 3, 4]
            assert np.array_equal(got[1][others], clean[1][others], equal_nan=True)
            assert np.array_equal(got[2][others], clean[2][others])
        # a NaN with the sign bit set, and a NaN payload, are NaN too
        weird = np.array(E0)
        weird.view(np.uint64)[off[0] + 7, 3] = 0xFFF8000000000001
        weird.view(np.uint64)[off[5] + 1, N - 1] = 0x7FF0000000000001
        assert_same(cv.decode_emissions(h, off, weird, kernel=kernel), want, (N, kernel, "NaN patterns"))


@pytest.mark.parametrize("N", [65, 257])
def test_minus_zero_reads_as_plus_zero(gpu, N):
    pi, a, b0, off, E0 = case(N)
    h = cv.HMM(pi, a, b0, device=gpu)
    mask = np.random.default_rng(N).random(E0.shape) < 0.2
    plus, minus = np.array(E0), np.array(E0)
    plus[mask] = 0.0
    minus[mask] = -0.0
    assert np.signbit(minus[mask]).all() and not np.signbit(plus[mask]).any()
    b, obs = as_discrete(plus, N)
    ref = c_oracle.decode_batch(pi, a, b, off, obs, c_oracle.VITERBI)
    for kernel in ("auto", "generic"):
        assert_same(cv.decode_emissions(h, off, plus, kernel=kernel), ref, (N, kernel, "+0.0"))
        assert_same(cv.decode_emissions(h, off, minus, kernel=kernel), ref, (N, kernel, "-0.0"))


# ---- 6. batch layouts of the f64 trellis -------------------------------------------------------
def _layout_lengths(name):
    if name == "8 per wave":
        return 130, [3] * 16384
    if name == "row-split pairs":
        return 256, [4] * 2048
    return 256, [1 + (5 * k) % 4 for k in range(2050)]  # column-split pairs


@pytest.mark.parametrize("name", ["8 per wave", "row-split pairs", "column-split pairs"])
def test_batch_layouts_match_the_discrete_decode(gpu, name):
    N, lengths = _layout_lengths(name)
    pi, a, b0 = model(N)
    off, E = scores(N, lengths, dead=2)
    b, obs = as_discrete(E, N)
    hd = cv.HMM(pi, a, b, device=gpu)
    want = cv.decode_batch(hd, off, obs, dtype="f64")
    td = cv.last_timing(hd)
    h = cv.HMM(pi, a, b0, device=gpu)
    got = cv.decode_emissions(h, off, E)
    t = cv.last_timing(h)
    assert_same(got, want, name)
    for key in ("kernel", "padded_states", "seqs_per_wave", "launches"):
        assert t[key] == td[key], (key, t, td)
    assert t["kernel"] == "trellis_f64"
    if name == "8 per wave":
        assert t["seqs_per_wave"] == 8, t
    assert (got[2] == L.SEQ_OK).sum() > len(lengths) // 2 and got[2][2] == L.SEQ_INFEASIBLE


# ---- 7. the device entry point with torch ------------------------------------------------------
def test_torch_gaussian_scores_on_a_stream(gpu):
    N, D = 65, 3
    dev = torch.device(f"cuda:{gpu}")
    pi, a, b0 = model(N)
    off = offsets_of(LENGTHS)
    total = int(off[-1])
    g = torch.Generator(device="cpu").manual_seed(11)
    x = torch.randn(total, D, dtype=torch.float64, generator=g).to(dev)
    mu = torch.randn(N, D, dtype=torch.float64, generator=g).to(dev)
    sigma = (0.05 + torch.rand(N, D, dtype=torch.float64, generator=g)).to(dev)
    # log10 N(x; mu_j, diag sigma_j^2): positive where a narrow component sits on the observation
    z = (x[:, None, :] - mu[None]) / sigma[None]
    logp = (-0.5 * (z * z).sum(-1) - sigma.log().sum(-1)[None] - 0.5 * D * np.log(2 * np.pi)) / np.log(10.0)
    wide = torch.full((total, 96), float("nan"), dtype=torch.float64, device=dev)
    wide[:, :N] = logp
    E_dev = wide[:, :N]
    assert E_dev.stride(0) == 96 > N and not E_dev.is_contiguous()
    E = E_dev.cpu().numpy()
    assert (E > 0).any() and np.isfinite(E).all()
    b, obs = as_discrete(E, N)
    ref = c_oracle.decode_batch(pi, a, b, off, obs, c_oracle.VITERBI)
    assert (ref[2] == [0, 0, 0, 0, L.SEQ_EMPTY, 0]).all()

    h = cv.HMM(pi, a, b0, device=gpu)
    off_d = torch.from_numpy(off).to(dev)
    outs = [(torch.full((total,), -7, dtype=torch.int32, device=dev),
             torch.full((len(LENGTHS),), 77.0, dtype=torch.float64, device=dev),
             torch.full((len(LENGTHS),), 9, dtype=torch.uint8, device=dev)) for _ in range(2)]
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        for path, score, status in outs:  # twice in a row, nothing in between
            cv.decode_emissions_device(h, off_d, E_dev, path, score, status, offsets_host=off,
                                       stream=stream.cuda_stream)
    stream.synchronize()
    first, second = [tuple(t.cpu().numpy() for t in o) for o in outs]
    assert_same(first, ref, "first call")
    assert_same(second, first, "second call")
    with pytest.raises(ValueError):
        cv.decode_emissions_device(h, off_d, wide[:, :2 * N:2], *outs[0], offsets_host=off)  # stride(1) != 1
    with pytest.raises(ValueError):
        cv.decode_emissions_device(h, off_d, E_dev.float(), *outs[0], offsets_host=off)
    with pytest.raises(ValueError):
        cv.decode_emissions_device(h, off_d, E_dev.cpu(), *outs[0], offsets_host=off)
    with pytest.raises(ValueError):
        cv.decode_emissions_device(h, off_d, wide[:, :N - 1], *outs[0], offsets_host=off)  # stride(0) >= N, too narrow
