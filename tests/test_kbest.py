"""CPU: the K-best (list) Viterbi feature's host-side checks -- the symbols and Python wrappers
exist, the argument checks that need no device, the numpy specification (tests/kbest_ref.py)
against exhaustive enumeration on tiny models, and hipcc builds the new kernel file for gfx950
with the lists of kbest_fwd in registers (no scratch, no spill up to KT = 8)."""
import os
import re
import subprocess

import numpy as np
import pytest

import cviterbi as cv
from conftest import ROOT, has_gpu
from cviterbi import _lib as L
from kbest_ref import brute_force, fold_score, kbest_ref, quantised_model, random_logprobs

KS = [1, 2, 3, 4, 8]


def test_symbols_and_wrappers_exist():
    lib = L.lib()
    for name in ("cv_kbest_batch", "cv_kbest_batch_device"):
        assert name in L.EXPORTS
        assert getattr(lib, name) is not None
    assert callable(cv.kbest_batch) and callable(cv.kbest_batch_device)


def test_null_arguments_and_bad_k_are_einval():
    pi, a, b = random_logprobs(4, 3, seed=1)
    h = cv.HMM(pi, a, b)
    off = np.array([0, 2], np.int64)
    obs = np.array([0, 1], np.int32)
    path, score = np.zeros((16, 2), np.int32), np.zeros((1, 16))
    cnt, st8 = np.zeros(1, np.int32), np.zeros(1, np.uint8)
    p = lambda x: x.ctypes.data
    lib = L.lib()
    good = [h.handle, 1, p(off), p(obs), 2, None, p(path), p(score), p(cnt), p(st8)]
    for k in (0, 17, -1):
        args = list(good)
        args[4] = k
        assert lib.cv_kbest_batch(*args) == L.CV_EINVAL, k
    for hole in (0, 2, 3, 6, 7, 8, 9):
        args = list(good)
        args[hole] = None
        assert lib.cv_kbest_batch(*args) == L.CV_EINVAL, hole
    dev = [h.handle, 1, None, p(off), p(obs), 2, None, p(path), p(score), p(cnt), p(st8)]
    for k in (0, 17):
        args = list(dev)
        args[5] = k
        assert lib.cv_kbest_batch_device(*args) == L.CV_EINVAL, k
    for hole in (0, 3, 4, 7, 8, 9, 10):
        args = list(dev)
        args[hole] = None
        assert lib.cv_kbest_batch_device(*args) == L.CV_EINVAL, hole
    with pytest.raises(cv.CVError) as e:
        cv.kbest_batch(h, off, obs, 17)
    assert e.value.status == L.CV_EINVAL


@pytest.mark.skipif(has_gpu(), reason="checks the no-device error path")
def test_kbest_without_device_fails_loudly():
    pi, a, b = random_logprobs(4, 3, seed=1)
    h = cv.HMM(pi, a, b)
    with pytest.raises(cv.CVError) as e:
        cv.kbest_batch(h, [0, 3], np.array([1, 2, 0], np.int32), 4)
    assert e.value.status == L.CV_EDEVICE


def _models(kind, n, v, seed):
    if kind == "random":
        return random_logprobs(n, v, seed)
    return quantised_model(n, v, seed, inf_arcs=(kind == "ties_inf"))


def check_against_brute_force(pi, a, b, obs, K, got, forced=None):
    """got = (paths[K, T], scores[K], count): the score list is the brute-force top-K multiset,
    the paths are distinct paths whose fold is their score, unused ranks are -1 / -inf."""
    paths, scores, count = got
    ref_scores, _ = brute_force(pi, a, b, obs, forced)
    assert count == min(K, len(ref_scores)), (count, len(ref_scores))
    assert np.array_equal(scores[:count], ref_scores[:count])
    assert np.all(scores[count:] == -np.inf) and np.all(paths[count:] == -1)
    seen = set()
    for r in range(count):
        p = tuple(int(s) for s in paths[r])
        assert p not in seen, (r, p)
        seen.add(p)
        assert fold_score(pi, a, b, obs, p) == scores[r], (r, p)
        if forced is not None:
            assert all(f < 0 or f == s for f, s in zip(forced, p))


@pytest.mark.parametrize("kind", ["random", "ties", "ties_inf"])
def test_kbest_ref_matches_brute_force(kind):
    rng = np.random.default_rng(11)
    cases = short = 0
    for N in range(1, 5):
        for T in range(1, 6):
            pi, a, b = _models(kind, N, 3, seed=100 * N + T)
            obs = rng.integers(0, 3, size=T).astype(np.int32)
            forced = None
            if T >= 3 and N >= 2:  # one case in two with a partial tag
                forced = np.full(T, -1)
                forced[T // 2] = int(rng.integers(0, N))
            for frc in (None, forced) if forced is not None else (None,):
                ref8 = kbest_ref(pi, a, b, obs, 8, frc)
                for K in KS:
                    got = kbest_ref(pi, a, b, obs, K, frc)
                    check_against_brute_force(pi, a, b, obs, K, got, frc)
                    # the K' < K result is a prefix of the K result
                    c = min(K, ref8[2])
                    assert got[2] == c
                    assert np.array_equal(got[0][:c], ref8[0][:c]) and np.array_equal(got[1][:c], ref8[1][:c])
                    cases += 1
                    short += got[2] < K
            # rank 0 is the first-index Viterbi path: max with strict >, first index among equals
            if kbest_ref(pi, a, b, obs, 1)[2]:
                assert np.array_equal(kbest_ref(pi, a, b, obs, 1)[0][0], first_index_viterbi(pi, a, b, obs))
    assert cases >= 5 * 20 and short > 0


def first_index_viterbi(pi, a, b, obs):
    """The plain f64 Viterbi recurrence (the generic decode kernel's: strict >, first index)."""
    N = len(pi)
    d = pi + b[:, obs[0]]
    psi = np.zeros((len(obs), N), np.int64)
    with np.errstate(invalid="ignore"):
        for t in range(1, len(obs)):
            nd = np.empty(N)
            for j in range(N):
                x = d + a[:, j]
                psi[t, j] = int(np.argmax(x))  # the first index of the maximum
                nd[j] = x[psi[t, j]] + b[j, obs[t]]
            d = nd
    s = int(np.argmax(d))
    path = []
    for t in range(len(obs) - 1, -1, -1):
        path.append(s)
        s = psi[t, s]
    return np.array(path[::-1], np.int32)


def test_hipcc_builds_kbest_for_gfx950(tmp_path):
    """The new kernel file compiles for gfx950; the compiler's resource remarks show the lists of
    kbest_fwd in registers: no scratch and no spilled VGPR up to KT = 8 (KT = 16 is printed)."""
    src = os.path.join(ROOT, "consistent-viterbi_amd", "csrc", "kernels", "kbest.hip")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "-ffp-contract=off", "-fno-honor-nans", "--offload-arch=gfx950",
                        "--cuda-device-only", "-c", src, "-o", str(tmp_path / "kbest.o"),
                        "-Rpass-analysis=kernel-resource-usage"],  # the Makefile's flags of kbest.o
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert os.path.getsize(tmp_path / "kbest.o") > 0
    blocks = re.split(r"Function Name: ", r.stderr)[1:]
    seen = set()
    for blk in blocks:
        name = blk.split()[0]
        m = re.search(r"kbest_fwdILi(\d+)ELi(\d+)E", name)
        if not m:
            continue
        kt, s = int(m.group(1)), int(m.group(2))
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blk).group(1))
        spill = int(re.search(r"VGPRs Spill: (\d+)", blk).group(1))
        vgprs = int(re.search(r"VGPRs: (\d+)", blk).group(1))
        print(f"kbest_fwd<KT={kt}, S={s}>: {vgprs} VGPRs, scratch {scratch} bytes/lane, {spill} VGPRs spilled")
        seen.add((kt, s))
        if kt <= 8:
            assert scratch == 0 and spill == 0, name
    assert seen == {(2, 4), (2, 2), (2, 1), (4, 2), (4, 1), (8, 2), (8, 1), (16, 1)}, seen
