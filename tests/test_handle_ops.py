"""No GPU: the call sequence of tests/test_gpu_handle_reuse.py makes every ordered pair of a
model's operations adjacent, and the catalogue and its inputs are what that test relies on."""
import numpy as np
import pytest

import handle_ops as H


@pytest.mark.parametrize("n", [1, 2, 3, 7, 26, 33])
def test_pair_circuit_covers_every_ordered_pair_once(n):
    c = H.pair_circuit(n)
    assert len(c) == n * n + 1 and c[0] == c[-1] == 0
    pairs = list(zip(c, c[1:]))
    assert len(set(pairs)) == n * n == len(pairs)
    assert set(pairs) == {(x, y) for x in range(n) for y in range(n)}
    assert c == H.pair_circuit(n)  # deterministic


@pytest.mark.parametrize("name", list(H.MODELS))
def test_segments_of_a_model_lose_no_pair(name):
    ops = H.op_names(name)
    n = len(ops)
    assert len(set(ops)) == n >= 25
    segs = H.circuit_segments(n)
    assert all(2 <= len(s) <= H.SEGMENT_CALLS + 1 for s in segs)
    for prev, cur in zip(segs, segs[1:]):
        assert cur[0] == prev[-1]  # warmed by the previous segment's last operation
    pairs = [p for s in segs for p in zip(s, s[1:])]
    assert len(pairs) == n * n and set(pairs) == {(x, y) for x in range(n) for y in range(n)}


def test_catalogue_follows_the_documented_limits():
    for name, (n, _) in H.MODELS.items():
        ops = set(H.op_names(name))
        assert ("f32_trellis" in ops) == ("f32_nowave" in ops) == ("constrained_f32" in ops) == (n <= 256)
        assert ("f64_fixed_first_1" in ops) == ("f64_fixed_first_0" in ops) == (224 < n <= 256)
        assert set(H.EXPECT_FAIL) <= ops and set(H.F64_ASSOC) <= ops
        assert set(H.DECODE_OPS) & ops == {o for o in ops if o in H.DECODE_OPS}


@pytest.mark.parametrize("name", list(H.MODELS))
def test_inputs(name):
    small, large = H.inputs(name, "small"), H.inputs(name, "large")
    assert small.lengths.tolist() == [0, 1, 2, 9, 5, 1, 17]
    assert len(large.lengths) == 150 and large.lengths.max() == 48 and large.lengths[75] == 0
    for x in (small, large):
        assert x is H.inputs(name, x.batch)  # built once
        assert x.obs_ok.max() < H.IMPOSSIBLE and x.obs.max() < H.V and x.obs.min() >= 0
        bad = np.nonzero((x.obs_bad < 0) | (x.obs_bad >= H.V))[0]
        assert len(bad) == 1 and x.off[x.bad_seq] <= bad[0] < x.off[x.bad_seq + 1]
        assert (x.obs == H.IMPOSSIBLE).any() == (x.kind == "quantised")
        assert np.array_equal(x.emis, x.b.T[x.obs]) and x.emis.shape == (x.total, x.n)
        # about half of the sequences constrained, one component twice in one sequence
        per_seq = [x.comp[x.off[s]:x.off[s + 1]] for s in range(len(x.lengths))]
        held = [int((c >= 0).sum()) for c in per_seq]
        assert 0.3 * len(held) <= sum(h > 0 for h in held) <= 0.7 * len(held)
        twice = [c[c >= 0] for c in per_seq if (c >= 0).sum() == 2]
        assert any(len(set(c.tolist())) == 1 for c in twice)
        assert x.comp.max() < H.NCOMP and ((x.forced >= -1) & (x.forced < x.n)).all() and (x.forced >= 0).any()


def test_first_difference_names_the_output_and_index():
    ref = (np.arange(6, dtype=np.int32), np.array([1.0, -np.inf]))
    assert H.first_difference((ref[0].copy(), ref[1].copy()), ref) is None
    got = (ref[0].copy(), np.array([1.0, np.nan]))
    assert "output 1: first difference at flat index 1" in H.first_difference(got, ref)
    assert "expected int32" in H.first_difference((ref[0].astype(np.int64), ref[1]), ref)
    assert H.first_difference(H.Failed((np.array([1], np.int32),)), ref).startswith("Failed")
    assert H.first_difference((np.array([0.0]),), (np.array([-0.0]),)) is not None  # bytes, not values
