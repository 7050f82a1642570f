"""CFN export (cfn.rs:11-205): cv_solver_write_cfn against the Python
restatement oracle/cfn_oracle.py, byte for byte.

CPU: the oracle's longest path against brute-force enumeration of state sequences (an
independent statement of cfn.rs:11-34), Rust `{}` float formatting on known cases, and the
numpy checker (write_cfn_text_np, what tests/test_gpu_cfn.py checks large problems with)
against the Python loops bit for bit and against the same enumeration.
GPU: the file the library writes equals the oracle's text for random super-sequences with
sequence crossings, repeated components, -inf transitions/emissions and every component
active; error statuses where the reference would panic."""
import itertools
import math

import numpy as np
import pytest

import cfn_oracle as CO
from cviterbi import cli, synth

RUST = [(0.1, "0.1"), (1.0, "1"), (-0.0, "-0"), (0.0, "0"), (1e-7, "0.0000001"), (1e21, "1000000000000000000000"),
        (123.456, "123.456"), (-1.5e-5, "-0.000015"), (-12.25, "-12.25"), (2.0 ** 60, "1152921504606847000"),
        (-math.inf, "-inf"), (math.inf, "inf"), (float("nan"), "NaN"), (5e-324, "0." + "0" * 323 + "5"),
        # the values tests/test_gpu_cfn.py sends through the library's formatter
        (-1.0, "-1"), (-0.1, "-0.1"), (-1e-7, "-0.0000001"), (-(2.0 ** 60), "-1152921504606847000"),
        (-1e21, "-1000000000000000000000"), (-1e300, "-1" + "0" * 300), (-5e-324, "-0." + "0" * 323 + "5"),
        (-(2.0 ** -1022), "-0." + "0" * 307 + "22250738585072014"), (-2.5, "-2.5")]


@pytest.mark.parametrize("x,s", RUST)
def test_rust_float_display(x, s):
    assert CO.rust_display(x) == s
    assert cli.rust_f64(x) == s


def _brute_longest(pi, a, b, value, comp, first, t_from, n_from, t_to, n_to):
    """max over every state sequence on (t_from, t_to] of the left-to-right f64 sum
    ((score + transition) + emission per step) with constrained elements forced."""
    N = len(pi)
    best = -math.inf
    steps = list(range(t_from + 1, t_to + 1))
    for states in itertools.product(range(N), repeat=len(steps)):
        prev, score, ok = n_from, 0.0, True
        for t, s in zip(steps, states):
            if comp[t] >= 0 and s != (n_from if t < t_to else n_to):
                ok = False
                break
            score = score + (pi[s] if first[t] else a[prev][s]) + b[s][value[t]]
            prev = s
        if ok:
            best = max(best, score)
    return best


def test_oracle_longest_path_vs_enumeration():
    pi, a, b = synth.random_hmm(3, 4, seed=3)
    pi, a, b = pi.tolist(), a.tolist(), b.tolist()
    a[1][2] = -math.inf
    value = [0, 3, 1, 2, 0, 1]
    first = [1, 0, 0, 1, 0, 0]
    comp = [0, -1, 0, -1, -1, 1]
    # the numpy checker's rows, whole and in blocks of two start states
    rows = [CO.segment_rows_np(pi, a, b, value, comp, first, 0, 5, block=blk) for blk in (None, 2)]
    for n1 in range(3):
        for n2 in range(3):
            got = CO.longest_path(pi, a, b, value, comp, first, 0, n1, 5, n2)
            ref = _brute_longest(pi, a, b, value, comp, first, 0, n1, 5, n2)
            # f64 rounding is monotone, so the DP's greedy max equals the best path sum exactly
            assert got == ref, (n1, n2)
            for r in rows:
                assert r[n1, n2] == ref, (n1, n2)
    # a segment whose free run follows a free run (dense rows) and one of a single step
    for t_from, t_to, cmp in ((2, 5, comp), (0, 1, [0, 1, -1, -1, -1, -1]), (1, 5, [-1, 0, 0, -1, 0, 1])):
        r = CO.segment_rows_np(pi, a, b, value, cmp, first, t_from, t_to)
        for n1 in range(3):
            for n2 in range(3):
                assert r[n1, n2] == _brute_longest(pi, a, b, value, cmp, first, t_from, n1, t_to, n2), (t_from, n1, n2)


# ---- problems for the two checkers and for tests/test_gpu_cfn.py ---------------------------
# A layout is one string per sequence: '.' = free element, a digit = the element's tag.
# recompute_constraints reorders the sequences, so both layouts hold their properties in any
# order.  A: k = 3, every sequence starts tagged and ends tagged on a boundary (f_time = 0,
# l_time = len - 1, every sequence start inside a one-step segment).  B: k = 2, every sequence
# starts and ends free (a start chain, end jobs, free runs of 2 and 3 across sequence starts).
# A free element followed by a boundary or by another free element costs the checker an N^3
# step (6 in A, 7 in B); one followed by a forced element costs N^2.
LAYOUT_A = ["0.0.10", "01", "1.1.0.021", "10.01", "2..2.0.012", "00.1.2.0.01"]
LAYOUT_B = [".0.0.", ".", ".010.0.", ".0.01010.0.", ".010.", ".0.0.10."]


def sweep_model(n, v, seed, neg=True):
    """Dense random model; with neg (and n >= 2), -inf in a tenth of the off-diagonal arcs, in
    a[1][1], a[0][n-1], pi[1], b[n//2][0] and a twentieth of b."""
    pi, a, b = synth.random_hmm(n, v, seed=seed)
    if neg and n >= 2:
        rng = np.random.default_rng(seed + 1)
        mask = rng.random((n, n)) < 0.1
        np.fill_diagonal(mask, False)
        a[mask] = -np.inf
        a[1, 1] = a[0, n - 1] = -np.inf
        b[rng.random((n, v)) < 0.05] = -np.inf
        b[n // 2, 0] = -np.inf
        pi[1] = -np.inf
    return pi, a, b


def layout_obs(layout, v, seed):
    """Observations per sequence: random, but 0 at the first tagged element of each sequence
    (with b[n//2][0] = -inf the start row then has a -inf entry whichever sequence comes first)."""
    rng = np.random.default_rng(seed)
    obs = [[int(x) for x in rng.integers(0, v, size=len(s))] for s in layout]
    for o, s in zip(obs, layout):
        tagged = [t for t, ch in enumerate(s) if ch != "."]
        if tagged:
            o[tagged[0]] = 0
    return obs


def layout_arrays(layout, obs):
    """(value, comp, first) of the sequences in the given order, tags as component ids."""
    value = [x for o in obs for x in o]
    comp = [-1 if ch == "." else int(ch) for s in layout for ch in s]
    first = [int(t == 0) for s in layout for t in range(len(s))]
    return value, comp, first


def features(pi, a, b, value, comp, first, rows):
    """What a problem exercises, from its arrays and the checker's rows (write_cfn_text_np)."""
    bnd = rows["bnd"]
    L = len(value)
    pairs = {(bnd[i][1], bnd[i + 1][1]) for i in range(len(bnd) - 1)}
    btimes = {t for t, _ in bnd}
    forced = [t for t in range(bnd[0][0], bnd[-1][0]) if comp[t] >= 0 and t not in btimes]
    free_run = longest = 0
    for c in comp:
        free_run = free_run + 1 if c < 0 else 0
        longest = max(longest, free_run)
    return {
        "neg_a": bool(np.isneginf(a).any()), "neg_b": bool(np.isneginf(b).any()), "neg_pi": bool(np.isneginf(pi).any()),
        "crossing": any(any(first[t] for t in range(bnd[i][0] + 1, bnd[i + 1][0] + 1)) for i in range(len(bnd) - 1)),
        "both_orientations": any((c2, c1) in pairs for c1, c2 in pairs),
        "forced_inside": bool(forced),
        "f_time_0": bnd[0][0] == 0, "l_time_last": bnd[-1][0] == L - 1, "l_time_before_last": bnd[-1][0] < L - 1,
        "bound_in_unary": bool(np.isneginf(rows["start"]).any() or np.isneginf(rows["end"]).any()),
        "longest_free_run": longest,
    }


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def _cpu_problems():
    """(name, pi, a, b, value, comp, first): the two layouts and four random ones per N."""
    for n in (1, 2, 3, 5, 9):
        v = 3
        for name, layout in (("A", LAYOUT_A), ("B", LAYOUT_B)):
            pi, a, b = sweep_model(n, v, seed=100 + n)
            yield (f"{name}{n}", pi, a, b) + layout_arrays(layout, layout_obs(layout, v, seed=n))
        for seed in range(4):
            rng = np.random.default_rng(1000 * n + seed)
            pi, a, b = sweep_model(n, v, seed=200 + 10 * n + seed, neg=seed != 3)
            k = 2 + seed % 2
            lens = rng.integers(1, 6, size=int(rng.integers(2, 6)))
            comp = [int(rng.integers(0, k)) if rng.random() < 0.45 else -1 for _ in range(int(lens.sum()))]
            if seed % 2 == 0:
                comp[0] = 0
            if seed < 2:
                comp[-1] = k - 1
            if max(comp) < 0:
                comp[len(comp) // 2] = 0
            ids = sorted({c for c in comp if c >= 0})  # every id below k in use: the tables are indexed by it
            comp = [ids.index(c) if c >= 0 else -1 for c in comp]
            first = [int(t == 0) for ln in lens for t in range(int(ln))]
            yield (f"r{n}.{seed}", pi, a, b, [int(x) for x in rng.integers(0, v, size=len(comp))], comp, first)


def test_numpy_checker_equals_python_checker():
    """write_cfn_text_np against write_cfn_text byte for byte, and its rows against
    longest_path / unary_start / unary_end bit for bit, on 30 seeded problems that between
    them hold every feature the export distinguishes (asserted, not left to the seeds)."""
    seen = {}
    count = 0
    for q, (name, pi, a, b, value, comp, first) in enumerate(_cpu_problems()):
        lists = (pi.tolist(), a.tolist(), b.tolist(), value, comp, first)
        ref = CO.write_cfn_text(*lists)
        # arrays or lists in, whole or in blocks of two start states
        got, rows = CO.write_cfn_text_np(pi, a, b, value, comp, first, block=2 if q % 2 else None, return_rows=True)
        assert got == ref, name
        assert CO.write_cfn_text_np(*lists) == ref, name
        n = len(pi)
        bnd = rows["bnd"]
        assert len(rows["seg"]) == len(bnd) - 1
        for i, seg in enumerate(rows["seg"]):
            want = [[CO.longest_path(*lists, bnd[i][0], n1, bnd[i + 1][0], n2) for n2 in range(n)] for n1 in range(n)]
            assert np.array_equal(_bits(seg), _bits(want)), (name, i)
        assert np.array_equal(_bits(rows["start"]), _bits(CO.unary_start(*lists, bnd[0][0]))), name
        assert np.array_equal(_bits(rows["end"]), _bits(CO.unary_end(*lists, bnd[-1][0]))), name
        for key, val in features(pi, a, b, value, comp, first, rows).items():
            seen[key] = max(seen.get(key, 0), val)
        count += 1
    assert count >= 30
    for key in ("neg_a", "neg_b", "neg_pi", "crossing", "both_orientations", "forced_inside", "f_time_0",
                "l_time_last", "l_time_before_last", "bound_in_unary"):
        assert seen[key], key


def test_zero_sum_table_is_left_out():
    """cfn.rs:196 writes a pair table when its sum is non-zero: a table holding +1 and -1 is left
    out, and its minimum still enters the bound."""
    inf = math.inf
    args = ([-0.5, -0.25], [[1.0, -inf], [-inf, -1.0]], [[0.0], [0.0]], [0, 0], [0, 1], [1, 0])
    for text in (CO.write_cfn_text(*args), CO.write_cfn_text_np(*args)):
        assert "f0_1" not in text
        assert "mustbe: >-2}" in text
        assert "f0: { scope: [n0], costs: [-0.5, -0.25] }" in text
    assert CO.sum_left_to_right([1e16, 1.0, -1e16]) == 0.0  # 1e16 + 1 rounds to 1e16: left to right, uncompensated


def _problem(n, v, nseq, ncomp, seed, neg=False):
    import cviterbi as cv

    pi, a, b = synth.random_hmm(n, v, seed=seed)
    if neg:
        a[0, n - 1] = -np.inf
        b[n - 1, 0] = -np.inf
    rng = np.random.default_rng(seed)
    seqs = [[(int(x), 0) for x in rng.integers(0, v, size=int(t))] for t in rng.integers(1, 9, size=nseq)]
    tags = [[(int(rng.integers(0, ncomp)) if rng.random() < 0.3 else None) for _ in s] for s in seqs]
    free = [(i, t) for i, s in enumerate(seqs) for t in range(len(s)) if tags[i][t] is None]
    for c, j in zip(range(ncomp), rng.permutation(len(free))):  # every component at least once
        i, t = free[j]
        tags[i][t] = c
    h = cv.HMM(pi, a, b.reshape(n, v, 1), bdims=(v, 1))
    ss = cv.SuperSequence(seqs, cv.Constraints.from_tags(tags), h)
    ss.recompute_constraints(1.0)
    return pi, a, b, h, ss


def _oracle_text(pi, a, b, ss):
    comp = np.where(ss.active == 1, ss.component, -1).tolist()
    return CO.write_cfn_text(pi.tolist(), a.tolist(), b.tolist(), ss.value.tolist(), comp, (ss.t == 0).astype(int).tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("n,v,nseq,ncomp,neg", [(2, 3, 4, 2, False), (3, 5, 6, 3, True), (7, 6, 8, 3, False),
                                                (16, 9, 5, 4, True)])
def test_gpu_cfn_matches_oracle(gpu, tmp_path, n, v, nseq, ncomp, neg):
    import cviterbi as cv

    pi, a, b, h, ss = _problem(n, v, nseq, ncomp, seed=10 * n + nseq, neg=neg)
    assert ss.number_constraints() == ncomp  # every component has an active position
    s = cv.GpuSolver(h, ss, "gpu")
    path = tmp_path / "problem.cfn"
    ms = s.write_cfn(path)
    assert ms >= 0
    got = path.read_text()
    ref = _oracle_text(pi, a, b, ss)
    assert got == ref
    comp = np.where(ss.active == 1, ss.component, -1)
    assert CO.write_cfn_text_np(pi, a, b, ss.value, comp, ss.t == 0) == ref


@pytest.mark.gpu
def test_gpu_cfn_errors(gpu, tmp_path):
    import cviterbi as cv

    pi, a, b = synth.random_hmm(3, 4, seed=1)
    h = cv.HMM(pi, a, b.reshape(3, 4, 1), bdims=(4, 1))
    seqs = [[(0, 0), (1, 0)], [(2, 0)]]
    ss = cv.SuperSequence(seqs, cv.Constraints.from_tags([[None, None], [None]]), h)
    with pytest.raises(cv.CVError):  # no constraint: the reference unwraps an empty list
        cv.GpuSolver(h, ss, "gpu").write_cfn(tmp_path / "x.cfn")
    # component 1 active, component 0 without active position: cost tables sized by the
    # number of active components, indexed by component id (out of bounds in the reference)
    ss = cv.SuperSequence(seqs, cv.Constraints.from_tags([[0, 1], [None]]), h)
    ss.active[ss.component == 0] = 0
    with pytest.raises(cv.CVError):
        cv.GpuSolver(h, ss, "gpu").write_cfn(tmp_path / "y.cfn")
