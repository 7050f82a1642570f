"""GPU: the argument contract of the 14 evaluation entries (posterior, sampling, expected counts,
likelihood gradients, expected emission counts; host and _device), called through cviterbi._lib.

One model (N = 3, V = 4) and one batch of four sequences of lengths 0, 1, 2, 9.  For every entry:
the valid call, nseq < 0, every pointer argument null in turn, dtype f32, the trellis kernels, an
association other than VITERBI, ld < N, ld_grad < N with a gradient buffer, draws = 0, and the
empty batch with default options and with dtype f32 -- the returned status and the message the
call left in cv_last_error ("" when it set none), and for the entries with count outputs whether
the empty batch zeroed them.

EXPECTED is what the library returned before the family's host code moved to csrc/evaluate.cpp:
the matrix was recorded from that build by observe() and is kept here as a literal table, so any
restructuring of the entries reproduces every status and text.  Two asymmetries are part of it:
cv_posterior_batch and cv_sample_batch return CV_OK for an empty batch without reading the
options, and only they (and their _device twins) check the options after selecting the device.
"""
import ctypes

import numpy as np
import pytest

import cviterbi as cv
from cviterbi import _lib as L
from cviterbi import synth

pytestmark = pytest.mark.gpu

N, V, DRAWS = 3, 4, 2
LENGTHS = (0, 1, 2, 9)
LD, LD_GRAD = N + 2, N + 1
SENTINEL = 7.0

# argument names in the order of each signature; "offh" is a _device entry's host copy of the offsets
ENTRIES = {
    "cv_posterior_batch": "h nseq off obs opts loglik path gamma status",
    "cv_posterior_batch_device": "h nseq offh off obs opts loglik path gamma status",
    "cv_sample_batch": "h nseq off obs draws seed seq_base opts spath score loglik status",
    "cv_sample_batch_device": "h nseq offh off obs draws seed seq_base opts spath score loglik status",
    "cv_posterior_emissions": "h nseq off emis ld opts loglik path gamma status",
    "cv_posterior_emissions_device": "h nseq offh off emis ld opts loglik path gamma status",
    "cv_expected_counts": "h nseq off obs opts loglik pi a gamma status",
    "cv_expected_counts_device": "h nseq offh off obs opts loglik pi a gamma status",
    "cv_expected_counts_emissions": "h nseq off emis ld opts loglik pi a gamma status",
    "cv_expected_counts_emissions_device": "h nseq offh off emis ld opts loglik pi a gamma status",
    "cv_loglik_grad_emissions": "h nseq off emis ld weight opts loglik pi a egrad ld_grad status",
    "cv_loglik_grad_emissions_device": "h nseq offh off emis ld weight opts loglik pi a egrad ld_grad status",
    "cv_expected_counts_model": "h nseq off obs weight opts loglik pi a b gamma status",
    "cv_expected_counts_model_device": "h nseq offh off obs weight opts loglik pi a b gamma status",
}
SCALARS = {"nseq": len(LENGTHS), "ld": LD, "ld_grad": LD_GRAD, "draws": DRAWS, "seed": 5, "seq_base": 0}
COUNTS = ("pi", "a", "b")
MARKER = b"bad argument"  # what cv_hmm_set_tuning(NULL, ...) leaves in cv_last_error; no entry says it


def _arrays():
    rng = np.random.default_rng(11)
    off = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    total, nseq = int(off[-1]), len(LENGTHS)
    return {
        "off": off,
        "obs": rng.integers(0, V, size=total).astype(np.int32),
        "emis": np.log10(rng.uniform(0.1, 1.0, size=(total, LD))),
        "weight": rng.uniform(0.5, 2.0, size=nseq),
        "loglik": np.zeros(nseq), "status": np.zeros(nseq, np.uint8),
        "path": np.zeros(total, np.int32), "spath": np.zeros(DRAWS * total, np.int32),
        "score": np.zeros(DRAWS * nseq), "gamma": np.zeros((total, N)), "egrad": np.zeros((total, LD_GRAD)),
        "pi": np.zeros(N), "a": np.zeros((N, N)), "b": np.zeros((N, V)),
    }


class Buffers:
    """The arguments of one entry: numpy arrays for a host entry, torch tensors on the GPU for a
    _device entry (whose offh stays a numpy array)."""

    def __init__(self, device):
        import torch

        self.torch = torch
        self.device = device
        host = _arrays()
        self.arr = {k: torch.from_numpy(v).cuda() for k, v in host.items()} if device else host
        self.arr["offh"] = host["off"]

    def ptr(self, name):
        x = self.arr[name]
        return x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr()

    def fill_counts(self):
        for k in COUNTS:
            self.arr[k][...] = SENTINEL

    def counts_zero(self, names):
        if self.device:
            self.torch.cuda.synchronize()
        return all(bool((self.arr[k] == 0).all()) for k in names)


def _call(lib, handle, name, bufs, null=None, opts=None, **scalars):
    """(status, the message the call set or "")."""
    o = L.opts(dtype=L.DTYPE_F64)
    for k, v in (opts or {}).items():
        setattr(o, k, v)
    args = []
    for a in ENTRIES[name].split():
        if a == "h":
            args.append(handle)
        elif a == "opts":
            args.append(ctypes.byref(o))
        elif a in SCALARS:
            args.append(scalars.get(a, SCALARS[a]))
        else:
            args.append(None if a == null else bufs.ptr(a))
    lib.cv_hmm_set_tuning(None, None, 0)
    assert lib.cv_last_error() == MARKER
    st = getattr(lib, name)(*args)
    if bufs.device:
        bufs.torch.cuda.synchronize()
    msg = lib.cv_last_error()
    return st, "" if msg == MARKER else msg.decode()


def observe(name, hmm):
    """Every case of one entry -> {case: (status, message[, zeroed])}."""
    lib = L.lib()
    spec = ENTRIES[name].split()
    bufs = Buffers(name.endswith("_device"))
    h = hmm.handle
    out = {"valid": _call(lib, h, name, bufs), "nseq<0": _call(lib, h, name, bufs, nseq=-1)}
    for a in spec:
        if a not in SCALARS and a not in ("h", "opts"):
            out["null " + a] = _call(lib, h, name, bufs, null=a)
    out["dtype f32"] = _call(lib, h, name, bufs, opts={"dtype": L.DTYPE_F32})
    out["kernel trellis"] = _call(lib, h, name, bufs, opts={"kernel": L.KERNEL_TRELLIS})
    out["kernel trellis_f64"] = _call(lib, h, name, bufs, opts={"kernel": L.KERNEL_TRELLIS_F64})
    out["assoc cp"] = _call(lib, h, name, bufs, opts={"assoc": L.ASSOC_CP})
    if "ld" in spec:
        out["ld<N"] = _call(lib, h, name, bufs, ld=N - 1)
    if "ld_grad" in spec:
        out["ld_grad<N"] = _call(lib, h, name, bufs, ld_grad=N - 1)
        out["ld_grad<N null egrad"] = _call(lib, h, name, bufs, null="egrad", ld_grad=N - 1)
    if "draws" in spec:
        out["draws=0"] = _call(lib, h, name, bufs, draws=0)
    counts = [k for k in COUNTS if k in spec]
    for case, o in (("empty", None), ("empty dtype f32", {"dtype": L.DTYPE_F32})):
        bufs.fill_counts()
        res = _call(lib, h, name, bufs, opts=o, nseq=0)
        out[case] = res + (bufs.counts_zero(counts),) if counts else res
    return out


_NULL = (1, "null argument")
_NULLD = (1, "null device buffer")
_F32 = (7, "the posterior path is f64 only")
_K1 = (1, "posterior kernel must be AUTO or GENERIC (kernel 1)")
_K3 = (1, "posterior kernel must be AUTO or GENERIC (kernel 3)")
_CP = (1, "the posterior path reads the model as the VITERBI association (assoc 1)")
_LD = (1, "ld = 2 is less than N = 3")
_LDG = (1, "ld_grad = 2 is less than N = 3")
_DRAWS = (1, "draws = 0 outside [1, 64]")
_NSEQ = (1, "nseq < 0")
_OK = (0, "")

EXPECTED = {
    "cv_posterior_batch": {
        "valid": _OK,
        "nseq<0": _NULL,
        "null off": _NULL,
        "null obs": _NULL,
        "null loglik": _NULL,
        "null path": _OK,
        "null gamma": _OK,
        "null status": _NULL,
        "dtype f32": _F32,
        "kernel trellis": _K1,
        "kernel trellis_f64": _K3,
        "assoc cp": _CP,
        "empty": _OK,
        "empty dtype f32": _OK,
    },
    "cv_posterior_batch_device": {
        "valid": _OK,
        "nseq<0": _NSEQ,
        "null offh": _OK,
        "null off": _NULLD,
        "null obs": _NULLD,
        "null loglik": _NULLD,
        "null path": _OK,
        "null gamma": _OK,
        "null status": _NULLD,
        "dtype f32": _F32,
        "kernel trellis": _K1,
        "kernel trellis_f64": _K3,
        "assoc cp": _CP,
        "empty": _OK,
        "empty dtype f32": _F32,
    },
    "cv_sample_batch": {
        "valid": _OK,
        "nseq<0": _NULL,
        "null off": _NULL,
        "null obs": _NULL,
        "null spath": _NULL,
        "null score": _OK,
        "null loglik": _OK,
        "null status": _NULL,
        "dtype f32": _F32,
        "kernel trellis": _K1,
        "kernel trellis_f64": _K3,
        "assoc cp": _CP,
        "draws=0": _DRAWS,
        "empty": _OK,
        "empty dtype f32": _OK,
    },
    "cv_sample_batch_device": {
        "valid": _OK,
        "nseq<0": _NSEQ,
        "null offh": _OK,
        "null off": _NULLD,
        "null obs": _NULLD,
        "null spath": _NULLD,
        "null score": _OK,
        "null loglik": _OK,
        "null status": _NULLD,
        "dtype f32": _F32,
        "kernel trellis": _K1,
        "kernel trellis_f64": _K3,
        "assoc cp": _CP,
        "draws=0": _DRAWS,
        "empty": _OK,
        "empty dtype f32": _F32,
    },
    "cv_posterior_emissions": {
        "valid": _OK,
        "nseq<0": _NULL,
        "null off": _NULL,
        "null emis": _NULL,
        "null loglik": _NULL,
        "null path": _OK,
        "null gamma": _OK,
        "null status": _NULL,
        "dtype f32": _F32,
        "kernel trellis": _K1,
        "kernel trellis_f64": _K3,
        "assoc cp": _CP,
        "ld<N": _LD,
        "empty": _OK,
        "empty dtype f32": _F32,
    },
    "cv_posterior_emissions_device": {
        "valid": _OK,
        "nseq<0": _NSEQ,
        "null offh": _OK,
        "null off": _NULLD,
        "null emis": _NULLD,
        "null loglik": _NULLD,
        "null path": _OK,
        "null gamma": _OK,
        "null status": _NULLD,
        "dtype f32": _F32,
        "kernel trellis": _K1,
        "kernel trellis_f64": _K3,
        "assoc cp": _CP,
        "ld<N": _LD,
        "empty": _OK,
        "empty dtype f32": _F32,
    },
    "cv_expected_counts": {
        "valid": _OK,
        "nseq<0": _NULL,
        "null off": _NULL,
        "null obs": _NULL,
        "null loglik": _NULL,
        "null pi": _NULL,
        "null a": _NULL,
        "null gamma": _OK,
        "null status": _NULL,
        "dtype f32": _F32,
        "kernel trellis": _K1,
        "kernel trellis_f64": _K3,
        "assoc cp": _CP,
        "empty": _OK + (True,),
        "empty dtype f32": _F32 + (False,),
    },
    "cv_expected_counts_device": {
        "valid": _OK,
        "nseq<0": _NSEQ,
        "null offh": _OK,
        "null off": _NULLD,
        "null obs": _NULLD,
        "null loglik": _NULLD,
        "null pi": _NULLD,
        "null a": _NULLD,
        "null gamma": _OK,
        "null status": _NULLD,
        "dtype f32": _F32,
        "kernel trellis": _K1,
        "kernel trellis_f64": _K3,
        "assoc cp": _CP,
        "empty": _OK + (True,),
        "empty dtype f32": _F32 + (False,),
    },
    "cv_expected_counts_emissions": {
        "valid": _OK,
        "nseq<0": _NULL,
        "null off": _NULL,
        "null emis": _NULL,
        "null loglik": _NULL,
        "null pi": _NULL,
        "null a": _NULL,
        "null gamma": _OK,
        "null status": _NULL,
        "dtype f32": _F32,
        "kernel trellis": _K1,
        "kernel trellis_f64": _K3,
        "assoc cp": _CP,
        "ld<N": _LD,
        "empty": _OK + (True,),
        "empty dtype f32": _F32 + (False,),
    },
    "cv_expected_counts_emissions_device": {
        "valid": _OK,
        "nseq<0": _NSEQ,
        "null offh": _OK,
        "null off": _NULLD,
        "null emis": _NULLD,
        "null loglik": _NULLD,
        "null pi": _NULLD,
        "null a": _NULLD,
        "null gamma": _OK,
        "null status": _NULLD,
        "dtype f32": _F32,
        "kernel trellis": _K1,
        "kernel trellis_f64": _K3,
        "assoc cp": _CP,
        "ld<N": _LD,
        "empty": _OK + (True,),
        "empty dtype f32": _F32 + (False,),
    },
    "cv_loglik_grad_emissions": {
        "valid": _OK,
        "nseq<0": _NULL,
        "null off": _NULL,
        "null emis": _NULL,
        "null weight": _OK,
        "null loglik": _NULL,
        "null pi": _NULL,
        "null a": _NULL,
        "null egrad": _OK,
        "null status": _NULL,
        "dtype f32": _F32,
        "kernel trellis": _K1,
        "kernel trellis_f64": _K3,
        "assoc cp": _CP,
        "ld<N": _LD,
        "ld_grad<N": _LDG,
        "ld_grad<N null egrad": _OK,
        "empty": _OK + (True,),
        "empty dtype f32": _F32 + (False,),
    },
    "cv_loglik_grad_emissions_device": {
        "valid": _OK,
        "nseq<0": _NSEQ,
        "null offh": _OK,
        "null off": _NULLD,
        "null emis": _NULLD,
        "null weight": _OK,
        "null loglik": _NULLD,
        "null pi": _NULLD,
        "null a": _NULLD,
        "null egrad": _OK,
        "null status": _NULLD,
        "dtype f32": _F32,
        "kernel trellis": _K1,
        "kernel trellis_f64": _K3,
        "assoc cp": _CP,
        "ld<N": _LD,
        "ld_grad<N": _LDG,
        "ld_grad<N null egrad": _OK,
        "empty": _OK + (True,),
        "empty dtype f32": _F32 + (False,),
    },
    "cv_expected_counts_model": {
        "valid": _OK,
        "nseq<0": _NULL,
        "null off": _NULL,
        "null obs": _NULL,
        "null weight": _OK,
        "null loglik": _NULL,
        "null pi": _NULL,
        "null a": _NULL,
        "null b": _NULL,
        "null gamma": _OK,
        "null status": _NULL,
        "dtype f32": _F32,
        "kernel trellis": _K1,
        "kernel trellis_f64": _K3,
        "assoc cp": _CP,
        "empty": _OK + (True,),
        "empty dtype f32": _F32 + (False,),
    },
    "cv_expected_counts_model_device": {
        "valid": _OK,
        "nseq<0": _NSEQ,
        "null offh": _OK,
        "null off": _NULLD,
        "null obs": _NULLD,
        "null weight": _OK,
        "null loglik": _NULLD,
        "null pi": _NULLD,
        "null a": _NULLD,
        "null b": _NULLD,
        "null gamma": _OK,
        "null status": _NULLD,
        "dtype f32": _F32,
        "kernel trellis": _K1,
        "kernel trellis_f64": _K3,
        "assoc cp": _CP,
        "empty": _OK + (True,),
        "empty dtype f32": _F32 + (False,),
    },
}


@pytest.fixture(scope="module")
def hmm(gpu):
    pi, a, b = synth.random_hmm(N, V, seed=3)
    return cv.HMM(pi, a, b, device=gpu)


@pytest.mark.parametrize("name", list(ENTRIES))
def test_entry_contract(name, hmm):
    got = observe(name, hmm)
    for case, res in got.items():
        print(name, case, res)
    assert got == EXPECTED[name]
