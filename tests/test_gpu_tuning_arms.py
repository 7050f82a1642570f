"""GPU: every kernel arm that only a tuning key can select (csrc/tuning.h: "Every key is
bit-identical in results"; DESIGN.md §4 has the table key -> instantiation -> launcher -> test).

Each arm is compared bit for bit -- path, score as uint64 bits, status -- with the C oracle at
the matching association and dtype (cp_superseq_f64 for the chain) and with the default-key call
on the same handle.  No tolerances.  The inputs are the suite's own trouble makers: a quantised
model (multiples of 0.5: exact ties, so the first-index rule decides paths), about 20% -inf
transitions, one impossible observation, a near-tie model (1e-12 perturbations below f32
resolution), a "positive" model (a + 0.75: not log-probabilities, the general interval test)
and ragged lengths that straddle every ring depth of the backtrack (2 / 4 / 8 / 16 / 32 rows in
flight) with a partly filled last workgroup of four.

Where last_timing or a stats call can show which layout ran the test asserts it; where it cannot
(backtrack depth, t64_rs, the chain's A in LDS) the docstring cites the launcher lines that make
the arm the only reachable one.
"""
import numpy as np
import pytest

import c_oracle as O
import cviterbi as cv
from cviterbi import _lib as L
from cviterbi import synth

pytestmark = pytest.mark.gpu

ASSOC = {"viterbi": O.VITERBI, "decode": O.DECODE, "dp": O.DP, "cp": O.CP}
V = 9
BAD = 3  # the impossible observation: b[:, BAD] = -inf
LENGTHS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 64, 65, 70]  # 18: 4 full workgroups of 4 + 2
PFS = (2, 4, 8, 16, 32)


def _same(got, ref, what):
    for x, y, name in zip(got, ref, ("path", "score", "status")):
        x, y = np.asarray(x), np.asarray(y)
        if name == "score":
            x, y = x.view(np.uint64), y.view(np.uint64)
        assert x.shape == y.shape, f"{what}: {name} shape {x.shape} vs {y.shape}"
        bad = np.nonzero(x != y)[0]
        assert bad.size == 0, f"{what}: {name} differs at {bad[:8]}"


def _same_chain(got, ref, what):
    (gp, gobj), (rp, robj) = got, ref
    assert np.float64(gobj).view(np.uint64) == np.float64(robj).view(np.uint64), f"{what}: objective {gobj} vs {robj}"
    bad = np.nonzero(np.asarray(gp) != np.asarray(rp))[0]
    assert bad.size == 0, f"{what}: path differs at {bad[:8]} of {len(rp)}"


def _quantised(rng, shape):
    """Multiples of 0.5 in [-2, 0].  The sum with 0.0 turns the -0.0 that rounding leaves for
    draws above -0.25 into +0.0: the same model value for value, but a best path made of zeros
    then scores +0.0 whatever the order of the additions and maxima.  With -0.0 entries the
    oracle's strict '>' keeps the first zero's sign and the kernels' max instructions prefer
    +0.0, so scores of 0.0 and -0.0 met (measured on the default keys: equal as numbers, and the
    paths equal); which zero a score of zero carries is not part of the project's contract
    (the suite compares scores with ==), and the bit comparison here should not depend on it."""
    return np.round(rng.uniform(-2, 0, shape) * 2) / 2 + 0.0


def _model(n, kind, seed):
    """quant: multiples of 0.5 in [-2, 0], ~20% of the transitions -inf, observation BAD
    impossible; near: the same minus uniform(0, 1e-12) (test_t64_backtrack_interval_paths);
    positive: a + 0.75 (entries above 0: the general interval test)."""
    rng = np.random.default_rng(seed)
    pi = _quantised(rng, n)
    a = _quantised(rng, (n, n))
    b = _quantised(rng, (n, V))
    a[rng.random((n, n)) < 0.2] = -np.inf
    b[:, BAD] = -np.inf
    if kind == "near":
        a = a - rng.uniform(0, 1e-12, (n, n))
        b = b - rng.uniform(0, 1e-12, (n, V))
    elif kind == "positive":
        a = a + 0.75
    else:
        assert kind == "quant", kind
    return pi, a, b


def _ragged(seed, lengths=LENGTHS, bad_at=(5, 11, 16)):
    """The ragged batch; sequences bad_at hold the impossible observation (infeasible)."""
    rng = np.random.default_rng(seed)
    off = synth.offsets_from_lengths(lengths)
    obs = rng.integers(0, V - 1, size=int(off[-1])).astype(np.int32)
    obs[obs >= BAD] += 1  # 0 .. V - 1 without BAD
    for k in bad_at:
        if k < len(lengths) and lengths[k] > 0:
            obs[off[k] + lengths[k] // 2] = BAD
    return off, obs


def _tie_rule_decides(pi, a, b, off, obs, path, status):
    """True when a row-A0 Viterbi that takes the LAST index among equal maxima decodes some OK
    sequence differently from `path` (the shortest such sequence ends the search).  The quantised
    models' sums are exact in f64, so against the oracle only the tie rule differs."""
    n = len(pi)
    for k in range(len(off) - 1):
        lo, hi = int(off[k]), int(off[k + 1])
        if status[k] != L.SEQ_OK or hi == lo:
            continue
        d = pi + b[:, obs[lo]]
        psi = np.zeros((hi - lo, n), np.int64)
        for t in range(1, hi - lo):
            c = d[:, None] + a
            psi[t] = n - 1 - np.argmax(c[::-1], axis=0)
            d = c[psi[t], np.arange(n)] + b[:, obs[lo + t]]
        s = n - 1 - int(np.argmax(d[::-1]))
        for t in range(hi - lo - 1, -1, -1):
            if path[lo + t] != s:
                return True
            s = psi[t][s]
    return False


def _cp_tie_rule_decides(pi, a, b, off, obs, path, status):
    """The same for CPSolver's association (psi = argmax_i d[i] + a[i, j], d'[j] = d[psi] +
    (a[psi, j] + b[j, o])): a forward pass that records the LAST maximal index (index 0 where
    every candidate is -inf) decodes some OK sequence differently from `path`."""
    n = len(pi)
    cols = np.arange(n)
    for k in range(len(off) - 1):
        lo, hi = int(off[k]), int(off[k + 1])
        if status[k] != L.SEQ_OK or hi == lo:
            continue
        d = pi + b[:, obs[lo]]
        psi = np.zeros((hi - lo, n), np.int64)
        for t in range(1, hi - lo):
            c = d[:, None] + a
            m = c.max(axis=0)
            psi[t] = np.where(m > -np.inf, n - 1 - np.argmax((c == m)[::-1], axis=0), 0)
            d = d[psi[t]] + (a[psi[t], cols] + b[:, obs[lo + t]])
        s = int(np.argmax(d))
        for t in range(hi - lo - 1, -1, -1):
            if path[lo + t] != s:
                return True
            s = psi[t][s]
    return False


_REF = {}


def _oracle(key, pi, a, b, off, obs, assoc, dtype=np.float64):
    """The oracle's decode, computed once per case and shared (never modified)."""
    k = (key, assoc, np.dtype(dtype).name)
    if k not in _REF:
        ref = O.decode_batch(pi, a, b, off, obs, ASSOC[assoc], dtype)
        for x in ref:
            x.setflags(write=False)
        _REF[k] = ref
    return _REF[k]


def _check_inputs(ref, pi, a, b, off, obs, ties):
    st = np.asarray(ref[2])
    assert (st == L.SEQ_INFEASIBLE).any() and (st == L.SEQ_OK).any(), st
    if ties:
        assert _tie_rule_decides(pi, a, b, off, obs, ref[0], st), "no tie decides a path element"


# ---- 1. backtrack_f64<KP, PF, ...>: t64_bt_pf ------------------------------------------------
NP_OF = {40: 64, 100: 128, 150: 192, 256: 256, 300: 512, 800: 1024}


@pytest.mark.parametrize("kind", ["quant", "near", "positive"])
@pytest.mark.parametrize("n", sorted(NP_OF))
def test_backtrack_rows_in_flight(gpu, n, kind):
    """t64_bt_pf in {2, 4, 8, 16, 32} at KP = 1, 2, 3, 4, 8, 16 under VITERBI / DECODE / DP: the
    NONPOS kernel (quant, near), the general one (positive) and, under DECODE, the second
    only_infeasible launch (the batch holds infeasible sequences); at 64 < N <= 256 with
    t64_lo_every 8 (the SPARSE kernel, last_t64_stats shows it) and 1.  The depth cannot be read
    back: launch_t64_bt (trellis64.hip) switches on t64_bt_depth(np, key) alone, which maps a
    request to the deepest instantiated depth not above it and the layout's cap (32 at NP = 64,
    16 up to 256, 8 at 512, 4 at 1,024), so every request succeeds.  Before that mapping the
    launcher returned hipErrorInvalidValue for 32 at NP = 128 / 192 / 256 (every variant, the
    sparse one included), 16 and 32 at NP = 512 and 8, 16 and 32 at NP = 1,024 (observed on an
    MI355X with the quant and positive models: 51 of their 195 keyed decodes here)."""
    pi, a, b = _model(n, kind, seed=100 + n)
    off, obs = _ragged(seed=200 + n)
    h = cv.HMM(pi, a, b)

    def run(assoc):
        got = cv.decode_batch(h, off, obs, dtype="f64", assoc=assoc, kernel="trellis_f64", rescore_f64=False)
        t = cv.last_timing(h)
        assert t["kernel"] == "trellis_f64" and t["padded_states"] == NP_OF[n], t
        return got

    for assoc in ("viterbi", "decode", "dp"):
        ref = _oracle(("bt", n, kind), pi, a, b, off, obs, assoc)
        if assoc == "viterbi":
            _check_inputs(ref, pi, a, b, off, obs, ties=kind != "near")
        sparse = assoc == "viterbi" and kind != "positive" and 64 < n <= 256
        for lo in (8, 1) if sparse else (8,):
            h.set_tuning(t64_lo_every=lo, t64_bt_pf=0)
            base = run(assoc)
            _same(base, ref, f"N={n} {kind} {assoc} lo={lo} default depth vs the oracle")
            for pf in PFS:
                if sparse and lo > 1:  # the handle's guard may pin a used handle to full rows: a fresh one
                    h = cv.HMM(pi, a, b)
                    h.set_tuning(t64_lo_every=lo)
                h.set_tuning(t64_bt_pf=pf)
                got = run(assoc)
                if sparse:
                    assert cv.last_t64_stats(h)["lo_every"] == lo, cv.last_t64_stats(h)
                _same(got, ref, f"N={n} {kind} {assoc} lo={lo} t64_bt_pf={pf} vs the oracle")
                _same(got, base, f"N={n} {kind} {assoc} lo={lo} t64_bt_pf={pf} vs the default depth")


@pytest.mark.parametrize("kind", ["quant", "near"])
@pytest.mark.parametrize("n", [40, 100, 150, 256])
def test_backtrack_rows_in_flight_certified_chain(gpu, n, kind):
    """The parallel chain's certified backtrack (backtrack_f64<KP, PF, true, true>: bt_pf's
    ba.cert arm, taken with chain_cert_fused = 1 at NP <= 256) at every t64_bt_pf, against the
    oracle's chained super-sequence."""
    pi, a, b = _model(n, kind, seed=100 + n)
    off, obs = _ragged(seed=300 + n, bad_at=())
    ref = O.cp_superseq_f64(pi, a, b, off, obs)
    assert ref[1] > -np.inf
    h = cv.HMM(pi, a, b)
    h.set_tuning(chain_cert_fused=1)
    base = cv.decode_superseq_cp(h, off, obs)
    assert cv.last_superseq_stats(h)["parallel"]
    _same_chain(base, ref, f"chain N={n} {kind} default depth vs the oracle")
    for pf in PFS:
        with h.tuned(t64_bt_pf=pf):
            got = cv.decode_superseq_cp(h, off, obs)
            assert cv.last_superseq_stats(h)["parallel"]
        _same_chain(got, ref, f"chain N={n} {kind} t64_bt_pf={pf} vs the oracle")
        _same_chain(got, base, f"chain N={n} {kind} t64_bt_pf={pf} vs the default depth")


# ---- 2. trellis_cp_f64<C, S, PF, W> ------------------------------------------------------------
CP_SEED = {40: 45, 100: 1105, 150: 155, 256: 261}


@pytest.mark.parametrize("n", sorted(CP_SEED))
def test_cp_trellis_waves_seqs_rows(gpu, n):
    """t64_cp_w in {1, 2} x t64_cp_s in {1, 2, 4} x t64_cp_pf in {0, 16} on test_t64_cp_seqs_per_wave's
    model (quantised ties, -inf, an impossible observation, 37 ragged sequences with empties).
    t64_cp_w = 1: one wave per workgroup (trellis_cp_f64<C, S, 4, 1>, which the default takes only
    above 4,096 sequences: t64_cp_waves); 2: the columns over NP / 64 waves (W = 2, 3, 4), 32 or
    16 rows in flight (launch_t64_cp_fwd).  N = 40: NP = 64, W stays 1.  seqs_per_wave is the S
    launched.  The seeds are that test's (n + 5) except at N = 100, where no tie decided a path
    element of its batch (a forward pass that kept the last maximal index passed there)."""
    rng = np.random.default_rng(CP_SEED[n])
    pi = _quantised(rng, n)
    a = _quantised(rng, (n, n))
    b = _quantised(rng, (n, V))
    a[rng.random((n, n)) < 0.2] = -np.inf
    b[:, BAD] = -np.inf
    lengths = rng.integers(0, 70, size=37)
    lengths[4] = 0
    off = synth.offsets_from_lengths(lengths)
    obs = rng.integers(0, V, size=int(off[-1])).astype(np.int32)
    ref = O.decode_batch(pi, a, b, off, obs, O.CP, np.float64)
    st = np.asarray(ref[2])
    assert (st == L.SEQ_INFEASIBLE).any() and (st == L.SEQ_OK).any() and (st == L.SEQ_EMPTY).any(), st
    assert _cp_tie_rule_decides(pi, a, b, off, obs, ref[0], st), "no tie decides a path element"
    h = cv.HMM(pi, a, b)
    base = cv.decode_batch(h, off, obs, dtype="f64", assoc="cp", rescore_f64=False)
    _same(base, ref, f"cp N={n} default keys vs the oracle")
    for w in (1, 2):
        for s in (1, 2, 4):
            for pf in (0, 16):
                with h.tuned(t64_cp_w=w, t64_cp_s=s, t64_cp_pf=pf):
                    got = cv.decode_batch(h, off, obs, dtype="f64", assoc="cp", rescore_f64=False)
                    t = cv.last_timing(h)
                what = f"cp N={n} t64_cp_w={w} t64_cp_s={s} t64_cp_pf={pf}"
                assert t["kernel"] == "trellis_f64" and t["seqs_per_wave"] == s, (what, t)
                _same(got, ref, what + " vs the oracle")
                _same(got, base, what + " vs the default keys")


# ---- 3. four column-split pairs per workgroup at S = 8 -----------------------------------------
@pytest.mark.parametrize("n", [193, 256])
def test_column_split_four_pairs(gpu, n):
    """t64_rs = 0, t64_s = 4 at NP = 256: fwd_cs<4, 4> hands the batch to fwd_w2<8> (trellis64.hip),
    where the row split is off (rs_mode false), so with wg_ok (equal lengths: decode.cpp sets it
    when 8 tmin >= 7 tmax) or t64_wg_force = 1 (the ragged batch) the only launch left is
    trellis_fwd_f64<2, 8, 8, false, false, 2, true, 2, 1, true, 4, 2>: four pairs of waves per
    workgroup, a barrier per step, units that finish at different steps.  t64_s = 4 also keeps the
    few-sequence kernel out (t64_few_launch).  B = 1, 31, 33, 70: less than one unit, one short of
    a workgroup of 32, one over, three workgroups."""
    pi, a, b = _model(n, "quant", seed=400 + n)
    h = cv.HMM(pi, a, b)
    cases = [(f"T={T} B={B}", [T] * B, ()) for T in (1, 2, 19) for B in (1, 31, 33, 70)]
    cases.append(("ragged", LENGTHS, (5, 11, 16)))
    for what, lengths, bad_at in cases:
        off, obs = _ragged(seed=400 + n + len(lengths), lengths=lengths, bad_at=bad_at)
        ref = O.decode_batch(pi, a, b, off, obs, O.VITERBI, np.float64)
        if what == "ragged":
            _check_inputs(ref, pi, a, b, off, obs, ties=True)
        h.set_tuning(t64_rs=1, t64_s=0, t64_wg_force=0, t64_lo_every=8)
        base = cv.decode_batch(h, off, obs, dtype="f64", rescore_f64=False)
        _same(base, ref, f"N={n} {what} default keys vs the oracle")
        for lo in (1, 8):
            h.set_tuning(t64_rs=0, t64_s=4, t64_wg_force=1 if what == "ragged" else 0, t64_lo_every=lo)
            got = cv.decode_batch(h, off, obs, dtype="f64", rescore_f64=False)
            t = cv.last_timing(h)
            assert t["kernel"] == "trellis_f64" and t["seqs_per_wave"] == 4 and t["padded_states"] == 256, t
            _same(got, ref, f"N={n} {what} lo={lo} four pairs vs the oracle")
            _same(got, base, f"N={n} {what} lo={lo} four pairs vs the default keys")


# ---- 4. t64_nonpos = 0 on log-probability models -----------------------------------------------
@pytest.mark.parametrize("kind", ["quant", "near"])
@pytest.mark.parametrize("n", [40, 130, 256, 300])
def test_general_interval_test_on_log_probability_models(gpu, n, kind):
    """t64_nonpos = 0 on a model that IS a log-probability model: the general f64 interval
    backtrack (no at32 tables, no sparse low planes), no fixed-point first pass even with
    t64_fixed_first = 1, the serial chain.  Back at 1 on the same handle everything returns."""
    pi, a, b = _model(n, kind, seed=500 + n)
    off, obs = _ragged(seed=600 + n)
    offc, obsc = _ragged(seed=700 + n, bad_at=())
    chain_ref = O.cp_superseq_f64(pi, a, b, offc, obsc)
    assert chain_ref[1] > -np.inf
    h = cv.HMM(pi, a, b)
    h.set_tuning(t64_fixed_first=1)

    def sweep(what):
        for assoc in ("viterbi", "decode", "dp", "cp"):
            ref = _oracle(("nonpos", n, kind), pi, a, b, off, obs, assoc)
            if assoc == "viterbi":
                _check_inputs(ref, pi, a, b, off, obs, ties=kind == "quant")
            # N = 300: AUTO takes the generic kernels for a batch this small; CP has no other there
            kernel = "trellis_f64" if assoc != "cp" else "auto"
            got = cv.decode_batch(h, off, obs, dtype="f64", assoc=assoc, kernel=kernel, rescore_f64=False)
            if assoc != "cp" or n <= 256:
                assert cv.last_timing(h)["kernel"] == "trellis_f64"
            if assoc == "viterbi":
                fx = cv.last_fixed_first_stats(h)
            _same(got, ref, f"N={n} {kind} {assoc} {what} vs the oracle")
        chain = cv.decode_superseq_cp(h, offc, obsc)
        _same_chain(chain, chain_ref, f"N={n} {kind} chain {what} vs the oracle")
        return fx, cv.last_superseq_stats(h)

    fx1, ch1 = sweep("t64_nonpos=1")
    assert ch1["parallel"], ch1
    if n == 256:  # the pass covers this N: the handle has built its tables and taken it once
        assert fx1["engaged"] == 1, fx1
    h.set_tuning(t64_nonpos=0)
    fx0, ch0 = sweep("t64_nonpos=0")
    assert fx0["engaged"] == 0, fx0
    assert not ch0["parallel"], ch0
    h.set_tuning(t64_nonpos=1)
    fx2, ch2 = sweep("t64_nonpos back at 1")
    assert ch2["parallel"], ch2
    assert fx2["engaged"] == fx1["engaged"], (fx1, fx2)


def test_general_interval_test_constrained(gpu):
    """test_constrained_small's smallest shape: the constrained decode under t64_nonpos = 0 (no
    certified suffix trace: trace_supported) equals the default key's, field by field."""
    n = 4
    pi, a, b = synth.random_hmm(n, 11, seed=50 + n)
    rng = np.random.default_rng(n)
    off = synth.offsets_from_lengths(rng.integers(1, 40, size=24))
    obs = rng.integers(0, 11, size=int(off[-1])).astype(np.int32)
    comp = synth.constraint_components(off, seed=n, ncomp=3, prob=0.6)
    h = cv.HMM(pi, a, b)
    base = cv.decode_constrained(h, off, obs, comp)
    with h.tuned(t64_nonpos=0):
        got = cv.decode_constrained(h, off, obs, comp)
        assert cv.last_suffix_traced(h) == 0
    _same(got[:3], base[:3], "constrained t64_nonpos=0 vs 1")
    assert np.array_equal(got[3], base[3])
    assert np.float64(got[4]).view(np.uint64) == np.float64(base[4]).view(np.uint64)
    ref_states, forced = O.constrained_forced(pi, a, b, off, obs, comp, np.float64)
    for c, s in ref_states.items():
        assert got[3][c] == s
    rp, rs, rst = O.decode_batch(pi, a, b, off, obs, O.VITERBI, np.float64, forced=forced)
    assert np.array_equal(got[0], rp) and np.array_equal(got[2], rst)
    ok = rst == L.SEQ_OK
    assert np.array_equal(got[1][ok].view(np.uint64), rs[ok].view(np.uint64))


# ---- 5. cp_superseq_chain<true>: chain_old = 1 -------------------------------------------------
@pytest.mark.parametrize("n", [3, 64, 100, 142, 143, 256])
def test_one_thread_per_state_chain(gpu, n):
    """chain_old = 1: cv_decode_superseq_cp skips the parallel chain and cp_chain_wg and launches
    cp_superseq_chain (launch_cp_superseq_chain, trellis64.hip): A in LDS (<true>) while
    (N^2 + 2N) * 8 <= 160 KiB -- N <= 142, above 64 KiB (N = 100, 142) through
    hipFuncSetAttribute -- and from L2 (<false>) from N = 143.  12 sequences, 300 elements, an
    empty and a one-element sequence; quantised ties decide path elements."""
    rng = np.random.default_rng(800 + n)
    pi = _quantised(rng, n)
    a = _quantised(rng, (n, n))
    b = _quantised(rng, (n, V))
    if n > 3:
        a[rng.random((n, n)) < 0.2] = -np.inf
    else:
        a[0, 1] = -np.inf
    lengths = [40, 0, 1, 33, 17, 64, 2, 31, 50, 8, 29, 25]
    assert sum(lengths) == 300
    off = synth.offsets_from_lengths(lengths)
    obs = rng.integers(0, V, size=300).astype(np.int32)
    ref = O.cp_superseq_f64(pi, a, b, off, obs)
    assert ref[1] > -np.inf
    # a tie decides: a chain that took the last index among equal candidates would differ
    first = np.zeros(300, bool)
    first[off[:-1][np.diff(off) > 0]] = True
    d = pi + b[:, obs[0]]
    ties = 0
    for t in range(1, 300):
        c = d[:, None] + (np.broadcast_to(pi, (n, n)) if first[t] else a)
        j = ref[0][t]
        ties += int((c[:, j] == c[:, j].max()).sum() > 1 and c[:, j].max() > -np.inf)
        d = c.max(axis=0) + b[:, obs[t]]
    assert ties > 0, "no tie on the oracle's path"
    h = cv.HMM(pi, a, b)
    base = cv.decode_superseq_cp(h, off, obs)
    _same_chain(base, ref, f"chain N={n} default keys vs the oracle")
    with h.tuned(chain_old=1):
        got = cv.decode_superseq_cp(h, off, obs)
        assert not cv.last_superseq_stats(h)["parallel"]
    _same_chain(got, ref, f"chain N={n} chain_old=1 vs the oracle")
    _same_chain(got, base, f"chain N={n} chain_old=1 vs the default keys")


# ---- 6. trellis_fwd2_f32, two barriers per step: f32_onebar = 0 --------------------------------
@pytest.mark.parametrize("kind", ["random", "quant"])
@pytest.mark.parametrize("n", [65, 128, 200, 256])
def test_f32_pair_kernel_two_barriers(gpu, n, kind):
    """f32_onebar = 0: trellis_fwd2_np (trellis.hip) launches trellis_fwd2_f32<NP, false, false>.
    test_pair_kernel_equal_and_ragged's lengths (most sequences pair with an equal-length
    neighbour, an odd leftover per length, T = 1 and 2) and nine equal ones, against the f32
    oracle."""
    if kind == "random":
        pi, a, b = synth.random_hmm(n, V, seed=n, zero_frac=0.02)
        b[:, BAD] = -np.inf
    else:
        pi, a, b = _model(n, "quant", seed=900 + n)
    rng = np.random.default_rng(n)
    h = cv.HMM(pi, a, b)
    for what, lengths in (("ragged", rng.choice([1, 2, 3, 17, 64], size=37)), ("equal", np.full(9, 33))):
        off, obs = _ragged(seed=900 + n, lengths=[int(x) for x in lengths], bad_at=(5, 11, 16))
        ref = O.decode_batch(pi, a, b, off, obs, O.VITERBI, np.float32)
        st = np.asarray(ref[2])
        assert (st == L.SEQ_INFEASIBLE).any() and (st == L.SEQ_OK).any(), st
        base = cv.decode_batch(h, off, obs, dtype="f32", rescore_f64=False)
        _same(base, ref, f"f32 N={n} {kind} {what} default keys vs the oracle")
        with h.tuned(f32_onebar=0):
            got = cv.decode_batch(h, off, obs, dtype="f32", rescore_f64=False)
            assert cv.last_timing(h)["kernel"] == "trellis"
        _same(got, ref, f"f32 N={n} {kind} {what} f32_onebar=0 vs the oracle")
        _same(got, base, f"f32 N={n} {kind} {what} f32_onebar=0 vs the default keys")


@pytest.mark.parametrize("n", [40, 128, 200])
def test_f32_pipeline_depth(gpu, n):
    """max_chunks (the f32 trellis's chunks over two streams, 1..64; anything else is 8): one
    chunk, two, the most, and values outside the range, with and without a workspace cap that
    forces several chunks -- the f32 oracle's bits every time."""
    pi, a, b = _model(n, "quant", seed=950 + n)
    rng = np.random.default_rng(950 + n)
    off, obs = _ragged(seed=951 + n, lengths=[int(x) for x in rng.integers(0, 70, size=150)], bad_at=(5, 77, 149))
    ref = O.decode_batch(pi, a, b, off, obs, O.VITERBI, np.float32)
    h = cv.HMM(pi, a, b)
    for ws in (0, 256 * 4 * 300):
        base = cv.decode_batch(h, off, obs, dtype="f32", rescore_f64=False, workspace_bytes=ws)
        _same(base, ref, f"f32 N={n} ws={ws} default depth vs the oracle")
        for k in (1, 2, 64, 1000, -1):
            with h.tuned(max_chunks=k):
                got = cv.decode_batch(h, off, obs, dtype="f32", rescore_f64=False, workspace_bytes=ws)
                assert cv.last_timing(h)["kernel"] == "trellis"
            _same(got, ref, f"f32 N={n} ws={ws} max_chunks={k} vs the oracle")
            _same(got, base, f"f32 N={n} ws={ws} max_chunks={k} vs the default depth")


# ---- 7. scheduling-only keys --------------------------------------------------------------------
def test_generic_issue_priority(gpu):
    """generic_prio = 1: generic_fwd_ms waves at issue priority 3 (launch_generic_fwd)."""
    n = 300
    pi, a, b = _model(n, "quant", seed=1000)
    off, obs = _ragged(seed=1001)
    h = cv.HMM(pi, a, b)
    for assoc in ("viterbi", "cp"):
        ref = O.decode_batch(pi, a, b, off, obs, ASSOC[assoc], np.float64)
        with h.tuned(generic_prio=1):
            got = cv.decode_batch(h, off, obs, dtype="f64", assoc=assoc, kernel="generic", rescore_f64=False)
            assert cv.last_timing(h)["kernel"] == "generic"
        _same(got, ref, f"generic_prio=1 {assoc} vs the oracle")
        base = cv.decode_batch(h, off, obs, dtype="f64", assoc=assoc, kernel="generic", rescore_f64=False)
        _same(got, base, f"generic_prio=1 {assoc} vs the default key")


@pytest.mark.parametrize("prio", [0, 1])
def test_chain_speculation_issue_priority(gpu, prio):
    """chain_spec_prio with chain_par_force = 3 at N = 256: every third sequence is re-decoded
    speculatively beside a forward pass, at the default issue priority or a raised one."""
    n = 256
    pi, a, b = _model(n, "quant", seed=1100)
    lengths = [int(x) for x in np.random.default_rng(1101).integers(1, 70, size=40)]
    lengths[2], lengths[7] = 0, 1
    off, obs = _ragged(seed=1102, lengths=lengths, bad_at=())
    ref = O.cp_superseq_f64(pi, a, b, off, obs)
    assert ref[1] > -np.inf
    h = cv.HMM(pi, a, b)
    with h.tuned(chain_par_force=3, chain_spec_prio=prio):
        got = cv.decode_superseq_cp(h, off, obs)
        st = cv.last_superseq_stats(h)
    assert st["parallel"] and st["spec_batches"] >= 1 and st["speculated"] >= 1, st
    _same_chain(got, ref, f"chain_spec_prio={prio} vs the oracle")


@pytest.fixture(scope="module")
def many_short():
    """3,500 short sequences, 210,000 elements at N = 6: enough for three host workers in the
    element scans (65,536 elements each: parallel_ranges) and the per-sequence ones (1,024)."""
    n, nseq = 6, 3500
    pi, a, b = _model(n, "quant", seed=1200)
    a[np.isinf(a)] = -1.5
    rng = np.random.default_rng(1201)
    lengths = rng.integers(55, 66, size=nseq)
    off, obs = _ragged(seed=1202, lengths=[int(x) for x in lengths], bad_at=(5, 1700, 3499))
    comp = synth.constraint_components(off, seed=1203, ncomp=3, prob=0.5)
    for k in (5, 1700, 3499):  # the infeasible sequences stay unconstrained
        comp[off[k]:off[k + 1]] = -1
    ref = O.decode_batch(pi, a, b, off, obs, O.VITERBI, np.float64)
    states, forced = O.constrained_forced(pi, a, b, off, obs, comp, np.float64)
    cref = O.decode_batch(pi, a, b, off, obs, O.VITERBI, np.float64, forced=forced)
    return pi, a, b, off, obs, comp, ref, states, cref


@pytest.mark.parametrize("threads", [1, 3])
def test_host_threads(gpu, many_short, threads):
    """host_threads = 1 / 3 on a host-pointer decode_batch and a decode_constrained call."""
    pi, a, b, off, obs, comp, ref, states, cref = many_short
    assert int(off[-1]) >= 3 * 65536 and len(off) - 1 >= 3 * 1024
    h = cv.HMM(pi, a, b)
    base = cv.decode_batch(h, off, obs, dtype="f64", rescore_f64=False)
    cbase = cv.decode_constrained(h, off, obs, comp)
    with h.tuned(host_threads=threads):
        got = cv.decode_batch(h, off, obs, dtype="f64", rescore_f64=False)
        cgot = cv.decode_constrained(h, off, obs, comp)
    _same(got, ref, f"host_threads={threads} decode_batch vs the oracle")
    _same(got, base, f"host_threads={threads} decode_batch vs the default key")
    for c, s in states.items():
        assert cgot[3][c] == s, (c, cgot[3][c], s)
    ok = np.asarray(cref[2]) == L.SEQ_OK
    assert np.array_equal(cgot[0], cref[0]) and np.array_equal(cgot[2], cref[2])
    assert np.array_equal(cgot[1][ok].view(np.uint64), cref[1][ok].view(np.uint64))
    _same(cgot[:3], cbase[:3], f"host_threads={threads} decode_constrained vs the default key")
    assert np.array_equal(cgot[3], cbase[3])
    assert np.float64(cgot[4]).view(np.uint64) == np.float64(cbase[4]).view(np.uint64)


# ---- 8. unlisted values ---------------------------------------------------------------------------
FAMILIES = ("t64_", "generic_", "wide_", "ext_wide_", "chain_", "f32_")
VALUES = (-1, 3, 5, 7, 1000)


def _source_keys():
    """The key table of csrc/tuning.cpp, read as text: the library is not built when the tests
    are collected (test_families_cover_the_kernel_keys holds it against cv.tuning_keys())."""
    import os
    import re

    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "consistent-viterbi_amd", "csrc",
                       "tuning.cpp")
    return re.findall(r"CVK_KEY\((\w+)\)", open(src).read().split("#define CVK_KEY", 1)[1])


KEYS = [k for k in _source_keys() if k.startswith(FAMILIES)]


@pytest.fixture(scope="module", params=[256, 300])
def unlisted_case(request):
    n = request.param
    pi, a, b = _model(n, "quant", seed=1300 + n)
    off, obs = _ragged(seed=1301 + n)
    offc, obsc = _ragged(seed=1302 + n, bad_at=())
    refs = {assoc: O.decode_batch(pi, a, b, off, obs, ASSOC[assoc], np.float64) for assoc in ("viterbi", "cp")}
    chain = O.cp_superseq_f64(pi, a, b, offc, obsc)
    assert chain[1] > -np.inf
    return n, cv.HMM(pi, a, b), off, obs, offc, obsc, refs, chain


def test_families_cover_the_kernel_keys():
    assert KEYS == [k for k in cv.tuning_keys() if k.startswith(FAMILIES)]
    assert len(KEYS) >= 40 and {"t64_bt_pf", "t64_cp_w", "generic_s", "wide_s", "chain_old", "f32_onebar"} <= set(KEYS)


@pytest.mark.parametrize("key", KEYS)
def test_unlisted_values_never_break_a_decode(gpu, unlisted_case, key):
    """Every integer key of the f64 trellis, the generic / wide kernels and the chain at values
    its header line does not list: cv_hmm_set_tuning rejects the value (EINVAL) or the decodes --
    plain (AUTO, and the f64 trellis asked for by name), CP, the chain -- succeed and equal the
    oracle.  Never an error at launch time."""
    n, h, off, obs, offc, obsc, refs, chain = unlisted_case
    old = h.tuning(key)
    try:
        for v in VALUES:
            try:
                h.set_tuning(**{key: v})
            except cv.CVError as e:
                assert "EINVAL" in str(e), e
                continue
            what = f"N={n} {key}={v}"
            for kernel in ("auto", "trellis_f64"):
                got = cv.decode_batch(h, off, obs, dtype="f64", kernel=kernel, rescore_f64=False)
                _same(got, refs["viterbi"], f"{what} {kernel} vs the oracle")
            got = cv.decode_batch(h, off, obs, dtype="f64", assoc="cp", rescore_f64=False)
            _same(got, refs["cp"], f"{what} cp vs the oracle")
            _same_chain(cv.decode_superseq_cp(h, offc, obsc), chain, f"{what} chain vs the oracle")
    finally:
        h.set_tuning(**{key: old})
