"""cv_solver_write_cfn where its kernel (cfn_rows_f64, csrc/kernels/cfn.hip) and its host half
can go wrong: the file the library writes equals the numpy checker's text
(oracle/cfn_oracle.py write_cfn_text_np, held against the Python loops and brute force in
tests/test_cfn.py) byte for byte.  No tolerances.

  state-count sweep   the strided state loop (256 threads, N to 513: threads that own 1, 2 and
                      3 states, forced states at index 0 and >= 256, N = 1)
  N = 4,097           dynamic LDS above 64 KiB (hipFuncSetAttribute)
  two slices          more jobs than one 256 MiB slice of output rows holds
  formatter           append_rust_f64's three layouts, subnormals, 2^60, 1e21, 1e300
  zero-sum table      cfn.rs:196 tests the table's sum, not its entries
  limit               N > 10,240 is CV_EUNSUPPORTED before anything is uploaded or launched

Super-sequences are built from tags and recompute_constraints(1.0), which also reorders the
sequences (utils.rs:105-165); what a problem exercises is therefore read from the arrays the
solver gets and asserted, never assumed from the layout.  N = 10,240 (all 160 KiB of LDS) is
left out: the library's work grows with N^3 (0.84 s at N = 4,097 on an MI355X, so about 13 s)
and its model is 839 MB three times over (caller, library, device)."""
import math
import time

import numpy as np
import pytest

import cfn_oracle as CO
from cviterbi import _lib as L
from cviterbi import synth
from test_cfn import LAYOUT_A, LAYOUT_B, RUST, features, layout_obs, sweep_model

SLICE_BYTES = 256 << 20  # cv_solver_write_cfn: output rows per launch


def build(pi, a, b, layout, obs):
    import cviterbi as cv

    n, v = b.shape
    seqs = [[(x, 0) for x in o] for o in obs]
    tags = [[None if ch == "." else int(ch) for ch in s] for s in layout]
    h = cv.HMM(pi, a, b.reshape(n, v, 1), bdims=(v, 1))
    ss = cv.SuperSequence(seqs, cv.Constraints.from_tags(tags), h)
    ss.recompute_constraints(1.0)
    assert ss.number_constraints() == len({ch for s in layout for ch in s if ch != "."})
    return h, ss


def arrays(ss):
    comp = np.where(ss.active == 1, ss.component, -1)
    return ss.value.tolist(), comp.tolist(), (ss.t == 0).astype(int).tolist()


def first_difference(got, ref):
    q = next((i for i, (x, y) in enumerate(zip(got, ref)) if x != y), min(len(got), len(ref)))
    line = got.count("\n", 0, q)
    entry = got.count(",", got.rfind("\n", 0, q) + 1, q)
    return f"lengths {len(got)} / {len(ref)}; first difference at byte {q}: line {line}, entry {entry}: " \
           f"{got[max(0, q - 30):q + 30]!r} vs {ref[max(0, q - 30):q + 30]!r}"


def check(h, ss, pi, a, b, tmp_path, label):
    """Library file == checker text; returns (text, checker rows)."""
    import cviterbi as cv

    value, comp, first = arrays(ss)
    path = tmp_path / "problem.cfn"
    t0 = time.perf_counter()
    cv.GpuSolver(h, ss, "gpu").write_cfn(path)
    t1 = time.perf_counter()
    ref, rows = CO.write_cfn_text_np(pi, a, b, value, comp, first, return_rows=True)
    t2 = time.perf_counter()
    print(f"\ncfn {label}: library {t1 - t0:.2f} s, checker {t2 - t1:.2f} s, {len(ref)} bytes")
    got = path.read_text()
    same = got == ref
    assert same, first_difference(got, ref)
    return got, rows


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["A", "B"])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 300, 513])
def test_gpu_cfn_state_sweep(gpu, tmp_path, n, variant):
    """Every thread-to-state split of the kernel's strided loops.  Variant A: three components,
    f_time = 0 and l_time = len - 1; variant B: two components, a start chain and end jobs.
    Both: -inf arcs, emissions and pi (N >= 2), segments across sequence starts, both
    orientations of a pair, forced elements inside segments, a unary entry replaced by the
    bound, free runs of at most 3.  Every start state is a job, so each forced step is taken
    with the forced state at index 0 and (N >= 257) at indices a thread reaches on its second
    trip; the rows of such a segment are asserted finite there, so the step counts."""
    v = 4
    layout = LAYOUT_A if variant == "A" else LAYOUT_B
    pi, a, b = sweep_model(n, v, seed=7 * n + (variant == "B"))
    h, ss = build(pi, a, b, layout, layout_obs(layout, v, seed=n))
    value, comp, first = arrays(ss)
    assert len(ss.orig_sizes) == 6 and 1 <= min(ss.orig_sizes) and max(ss.orig_sizes) <= 12
    _, rows = check(h, ss, pi, a, b, tmp_path, f"N={n} {variant}")
    f = features(pi, a, b, value, comp, first, rows)
    assert f["crossing"] and f["both_orientations"] and f["forced_inside"]
    assert f["longest_free_run"] <= 3
    assert f["f_time_0"] == (variant == "A") and f["l_time_last"] == (variant == "A")
    assert f["l_time_before_last"] == (variant == "B")
    if n >= 2:
        assert f["neg_a"] and f["neg_b"] and f["neg_pi"] and f["bound_in_unary"]
    bnd = rows["bnd"]
    inside = [i for i in range(len(bnd) - 1) if any(c >= 0 for c in comp[bnd[i][0] + 1:bnd[i + 1][0]])]
    assert inside
    if n >= 3:  # at N = 2 sweep_model leaves state 1 unreachable and little else finite
        assert any(np.isfinite(rows["seg"][i][0]).any() for i in inside)  # forced state 0
    if n >= 257:
        assert any(np.isfinite(rows["seg"][i][256:]).any() for i in inside)  # forced state >= 256


@pytest.mark.gpu
def test_gpu_cfn_lds_above_64k(gpu, tmp_path):
    """N = 4,097: two rows are 65,552 bytes of dynamic LDS.  One component, so no N^2 table is
    written: the file is the start chain (four free steps across a sequence start, one
    workgroup) plus the end cost of every state (free and forced elements alternating)."""
    n, v = 4097, 3
    pi, a, b = sweep_model(n, v, seed=4097, neg=False)
    mask = np.random.default_rng(1).random((n, n)) < 0.1
    np.fill_diagonal(mask, False)
    a[mask] = -np.inf
    pi[1] = -np.inf
    layout = ["..", "..0.0.", "0.0."]
    h, ss = build(pi, a, b, layout, layout_obs(layout, v, seed=3))
    value, comp, first = arrays(ss)
    assert 2 * n * 8 > 64 * 1024
    assert comp == [-1, -1, -1, -1, 0, -1, 0, -1, 0, -1, 0, -1]
    assert first == [1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 0]
    got, rows = check(h, ss, pi, a, b, tmp_path, "N=4097")
    assert rows["bnd"] == [(4, 0)] and "f0_" not in got
    # state 1 cannot start a sequence (pi[1] = -inf) and its end chain crosses a sequence start
    assert np.isfinite(rows["start"]).all() and (np.isfinite(rows["end"]) == (np.arange(n) != 1)).all()


@pytest.mark.gpu
def test_gpu_cfn_two_slices(gpu, tmp_path):
    """More jobs than one slice of output rows: the second launch uploads its jobs from offset
    j0 and its rows land at j0 * N.  402 boundaries at N = 300; the rows of the last segments
    (those of the last sequence, with free runs and forced elements), the end jobs and the
    start job come from the second slice."""
    n, v = 300, 4
    pi, a, b = sweep_model(n, v, seed=300)
    b = synth.random_hmm(n, v, seed=301)[2]  # finite emissions, equal sort keys: the sequences keep their order
    layout = ["01" * 9 + "."] * 22 + ["01.0.1..0.01.1."]
    h, ss = build(pi, a, b, layout, layout_obs(layout, v, seed=5))
    value, comp, first = arrays(ss)
    assert len(layout) >= 20
    bnd = CO.boundaries(comp)
    assert len(bnd) >= 374 and bnd[-1][0] < len(value) - 1
    per = SLICE_BYTES // (8 * n)
    jobs = (len(bnd) - 1) * n + n + 1
    assert per == 111848 and per < jobs <= 2 * per
    whole = -(-per // n)  # the first segment whose rows all come from the second slice
    assert any(bnd[i + 1][0] - bnd[i][0] >= 3 for i in range(whole, len(bnd) - 1))
    assert any(c >= 0 for i in range(whole, len(bnd) - 1) for c in comp[bnd[i][0] + 1:bnd[i + 1][0]])
    _, rows = check(h, ss, pi, a, b, tmp_path, "two slices")
    assert np.isfinite(rows["seg"][-1]).any() and np.isfinite(rows["end"]).any()


# every layout of append_rust_f64: point <= 0 (-0.1, -1e-7, -1.5e-5, the subnormals), point >=
# digits (-1, -2^60, -1e21, -1e300), a point inside the digits (-12.25); -inf entries are
# dropped from a table (it keeps 0) and replaced by the bound in a unary line
VALUES = [-1.0, -0.1, -1e-7, -1.5e-5, -12.25, -(2.0 ** 60), -1e21, -1e300, -5e-324, -(2.0 ** -1022), -math.inf]
DISPLAY = {x: s for x, s in RUST if x == x}


def _two_adjacent(pi, a, tmp_path, label):
    n = len(pi)
    b = np.zeros((n, 1))
    h, ss = build(np.array(pi), np.array(a), b, ["01"], [[0, 0]])
    assert arrays(ss) == ([0, 0], [0, 1], [1, 0])
    return check(h, ss, np.array(pi), np.array(a), b, tmp_path, label)[0]


@pytest.mark.gpu
def test_gpu_cfn_formatter_pair_table(gpu, tmp_path):
    """b = 0 and two adjacent constrained elements: the pair table is a[n1][n2] itself."""
    a = np.array(VALUES + [-2.5, -0.75, -3.0, -0.5, -123.456]).reshape(4, 4)
    got = _two_adjacent([-0.5, -0.25, -2.0, -3.0], a, tmp_path, "formatter a")
    line = next(ln for ln in got.split("\n") if ln.startswith("\t\tf0_1:"))
    want = [DISPLAY[x] if x != -math.inf else "0" for x in VALUES] + ["-2.5", "-0.75", "-3", "-0.5", "-123.456"]
    assert line == "\t\tf0_1: { scope: [n0, n1], costs: [" + ", ".join(want) + "] },"
    assert "mustbe: >" + DISPLAY[-1e300] + "}" in got  # -1 + -1e300


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [0, 1, 2])
def test_gpu_cfn_formatter_start_cost(gpu, tmp_path, chunk):
    """The same values through pi: with f_time = 0 the first component's unary line is pi + 0."""
    pi = (VALUES + [-2.5])[4 * chunk:4 * chunk + 4]
    got = _two_adjacent(pi, np.full((4, 4), -0.5), tmp_path, f"formatter pi {chunk}")
    want = [DISPLAY[x] if x != -math.inf else "-1.5" for x in pi]  # the bound: -1 + -0.5
    assert "\t\tf0: { scope: [n0], costs: [" + ", ".join(want) + "] }, \n" in got


@pytest.mark.gpu
def test_gpu_cfn_zero_sum_table(gpu, tmp_path):
    """A model with positive log entries can make a table of +1 and -1: its sum is
    0, so cfn.rs:196 leaves the line out, and its minimum still enters the bound."""
    inf = math.inf
    got = _two_adjacent([-0.5, -0.25], [[1.0, -inf], [-inf, -1.0]], tmp_path, "zero sum")
    assert "f0_1" not in got
    assert "mustbe: >-2}" in got


@pytest.mark.gpu
def test_gpu_cfn_state_limit(gpu, tmp_path):
    """N = 10,241: two rows no longer fit the LDS.  Refused by the host check, before any
    upload or launch, with a status that names the cause."""
    import cviterbi as cv

    n = 10241
    pi, a, b = np.zeros(n), np.zeros((n, n)), np.zeros((n, 1))
    h, ss = build(pi, a, b, ["0.1"], [[0, 0, 0]])
    path = tmp_path / "big.cfn"
    with pytest.raises(cv.CVError) as e:
        cv.GpuSolver(h, ss, "gpu").write_cfn(path)
    assert e.value.status == L.CV_EUNSUPPORTED
    assert "10240" in str(e.value)
    assert not path.exists()
