"""CPU: the dense-emission decode's host-side checks -- the symbols and Python wrappers exist,
the argument checks that need no device, the pinned specification (the C oracle and the numpy
oracle agree on the discrete model equivalent to a score matrix, tests/emis_ref.py), and hipcc
builds emis.hip for gfx950 with emis_prepare_f64 free of scratch and spills."""
import os
import re
import subprocess

import numpy as np
import pytest

import c_oracle
import cviterbi as cv
import np_oracle
from conftest import ROOT, has_gpu
from cviterbi import _lib as L
from emis_ref import LENGTHS, as_discrete, model, scores

ASSOCS = {"viterbi": c_oracle.VITERBI, "cp": c_oracle.CP, "dp": c_oracle.DP, "decode": c_oracle.DECODE}


def test_symbols_and_wrappers_exist():
    lib = L.lib()
    for name in ("cv_decode_emissions", "cv_decode_emissions_device"):
        assert name in L.EXPORTS
        assert getattr(lib, name) is not None
    assert callable(cv.decode_emissions) and callable(cv.decode_emissions_device)


def _call_args(N=4):
    pi, a, b0 = model(N)
    h = cv.HMM(pi, a, b0)
    off = np.array([0, 2], np.int64)
    E = np.zeros((2, N))
    path, score, st8 = np.zeros(2, np.int32), np.zeros(1), np.zeros(1, np.uint8)
    p = lambda x: x.ctypes.data
    keep = (off, E, path, score, st8)
    host = [h.handle, 1, p(off), p(E), N, None, p(path), p(score), p(st8)]
    dev = [h.handle, 1, None, p(off), p(E), N, None, p(path), p(score), p(st8)]
    return h, keep, host, dev


def test_null_arguments_and_short_rows_are_einval():
    h, keep, host, dev = _call_args()
    lib = L.lib()
    for hole in (0, 2, 3, 6, 7, 8):
        args = list(host)
        args[hole] = None
        assert lib.cv_decode_emissions(*args) == L.CV_EINVAL, hole
    for hole in (0, 3, 4, 7, 8, 9):
        args = list(dev)
        args[hole] = None
        assert lib.cv_decode_emissions_device(*args) == L.CV_EINVAL, hole
    for ld in (3, 0, -1):  # ld < N = 4
        args = list(host)
        args[4] = ld
        assert lib.cv_decode_emissions(*args) == L.CV_EINVAL, ld
        args = list(dev)
        args[5] = ld
        assert lib.cv_decode_emissions_device(*args) == L.CV_EINVAL, ld


def test_f32_and_the_f32_trellis_are_unsupported():
    import ctypes

    h, keep, host, dev = _call_args()
    lib = L.lib()
    for o in (L.opts(L.DTYPE_F32, L.ASSOC_VITERBI, L.KERNEL_AUTO),
              L.opts(L.DTYPE_F64, L.ASSOC_VITERBI, L.KERNEL_TRELLIS)):
        args = list(host)
        args[5] = ctypes.byref(o)
        assert lib.cv_decode_emissions(*args) == L.CV_EUNSUPPORTED
        args = list(dev)
        args[6] = ctypes.byref(o)
        assert lib.cv_decode_emissions_device(*args) == L.CV_EUNSUPPORTED
    with pytest.raises(cv.CVError) as e:
        cv.decode_emissions(h, keep[0], keep[1], kernel="trellis")
    assert e.value.status == L.CV_EUNSUPPORTED


@pytest.mark.skipif(has_gpu(), reason="checks the no-device error path")
def test_emissions_without_device_fail_loudly():
    h, keep, host, dev = _call_args()
    with pytest.raises(cv.CVError) as e:
        cv.decode_emissions(h, keep[0], keep[1])
    assert e.value.status == L.CV_EDEVICE
    assert L.lib().cv_decode_emissions_device(*dev) == L.CV_EDEVICE


def test_wrapper_passes_the_row_stride():
    """decode_emissions hands a row-strided array over as it is (ld = stride) and copies any
    other layout; checked on the arguments it would pass, no device needed."""
    from cviterbi import emissions

    seen = {}

    real = L.lib

    class FakeLib:
        def cv_decode_emissions(self, handle, nseq, off, emis, ld, *rest):
            seen["ld"], seen["ptr"] = ld, emis.value
            return L.CV_OK

        def __getattr__(self, name):
            return getattr(real(), name)

    pi, a, b0 = model(4)
    h = cv.HMM(pi, a, b0)
    wide = np.zeros((6, 7))
    L.lib = lambda: FakeLib()
    try:
        emissions.decode_emissions(h, [0, 6], wide[:, :5])
        assert seen == {"ld": 7, "ptr": wide.ctypes.data}
        emissions.decode_emissions(h, [0, 6], wide[:, 1:5])  # 8 bytes off the 16-byte alignment
        assert seen == {"ld": 7, "ptr": wide.ctypes.data + 8}
        emissions.decode_emissions(h, [0, 6], wide[:, ::2])  # column stride: copied
        assert seen["ld"] == 4 and seen["ptr"] != wide.ctypes.data
        emissions.decode_emissions(h, [0, 6], wide.astype(np.float32))  # dtype: copied
        assert seen["ld"] == 7
        with pytest.raises(ValueError):
            emissions.decode_emissions(h, [0, 7], wide)  # more elements than rows
        with pytest.raises(ValueError):
            emissions.decode_emissions(h, [0, 6], wide[:, :3])  # fewer columns than states, ld = 7 >= N
    finally:
        L.lib = real


@pytest.mark.parametrize("N", [1, 3, 47, 65, 257])
def test_the_two_oracles_agree_on_the_equivalent_model(N):
    """The pinned specification: positive values, 10% -inf entries, an all -inf sequence and an
    empty one, all four associations."""
    pi, a, _ = model(N)
    off, E = scores(N, LENGTHS)
    assert (E > 0).any() and np.isneginf(E).any() and off[4] == off[5]
    b, obs = as_discrete(E, N)
    assert b.shape == (N, len(E)) and np.array_equal(obs, np.arange(len(E)))
    for name, assoc in ASSOCS.items():
        c = c_oracle.decode_batch(pi, a, b, off, obs, assoc)
        with np.errstate(invalid="ignore"):
            n = np_oracle.decode_batch(pi, a, b, off, obs, assoc)
        for what, x, y in zip(("path", "score", "status"), c, n):
            assert np.array_equal(x, y, equal_nan=True), (name, what)
        assert c[2][2] == L.SEQ_INFEASIBLE and c[2][4] == L.SEQ_EMPTY and c[2][0] in (L.SEQ_OK, L.SEQ_INFEASIBLE)


def test_hipcc_builds_emis_for_gfx950(tmp_path):
    """emis.hip compiles for gfx950 with the Makefile's flags of emis.o; the compiler's resource
    remarks show emis_prepare_f64 without scratch and without a spilled VGPR."""
    src = os.path.join(ROOT, "consistent-viterbi_amd", "csrc", "kernels", "emis.hip")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950",
                        "--cuda-device-only", "-c", src, "-o", str(tmp_path / "emis.o"),
                        "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert os.path.getsize(tmp_path / "emis.o") > 0
    seen = 0
    for blk in re.split(r"Function Name: ", r.stderr)[1:]:
        name = blk.split()[0]
        if "emis_prepare_f64" not in name:
            continue
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blk).group(1))
        spill = int(re.search(r"VGPRs Spill: (\d+)", blk).group(1))
        vgprs = int(re.search(r"VGPRs: (\d+)", blk).group(1))
        print(f"{name}: {vgprs} VGPRs, scratch {scratch} bytes/lane, {spill} VGPRs spilled")
        assert scratch == 0 and spill == 0, name
        seen += 1
    assert seen == 2  # the 16-byte and the 8-byte store variants
