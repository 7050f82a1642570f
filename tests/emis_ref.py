"""Reference for the decode of caller-supplied emission scores (cv_decode_emissions*).

The specification is a substitution: decoding the dense scores E[e][j] is decoding the discrete
model b[j][e] = E[e][j] with the observation of element e being e itself.  So the expected
result of a dense decode is oracle/c_oracle.decode_batch (or, on the GPU, the product's own
cv.decode_batch) on the pair this module builds -- no second recurrence is written down here.
"""
import numpy as np

from cviterbi import synth

LENGTHS = [33, 1, 2, 5, 0, 64]


def as_discrete(E, N):
    """(b [N, len(E)], obs = arange(len(E))): the discrete model equivalent to the scores E."""
    E = np.asarray(E, np.float64)
    return E[:, :N].T.copy(), np.arange(len(E), dtype=np.int32)


def offsets_of(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def model(N, seed=None):
    """(pi, a, b0): log10 tables of a random N-state model; b0 [N, 2] is what the handle is
    created with and a dense decode must ignore."""
    return synth.random_hmm(N, 2, seed=5000 + N if seed is None else seed)


def scores(N, lengths=LENGTHS, seed=None, ninf_frac=0.1, dead=2):
    """E [sum T, N] ~ normal(0, 3) (positive and negative values), `ninf_frac` of the entries
    -inf, and the sequence of index `dead` (None: none) all -inf (INFEASIBLE)."""
    off = offsets_of(lengths)
    rng = np.random.default_rng(7000 + N if seed is None else seed)
    E = rng.normal(0.0, 3.0, size=(int(off[-1]), N))
    E[rng.random(E.shape) < ninf_frac] = -np.inf
    if dead is not None:
        E[off[dead]:off[dead + 1]] = -np.inf
    return off, E
