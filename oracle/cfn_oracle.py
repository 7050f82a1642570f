"""Pure-Python restatement of the reference's CFN export (viterbi_solver/cfn.rs:11-205).

TEST INFRASTRUCTURE ONLY: the checker for cv_solver_write_cfn, imported by tests/ only.
Parity unpinned against the Rust binary (it cannot be built here; main.rs:108 leaves the
CFN branch disabled and the reference ships no CFN fixture); pinned by the structure and
float-format cases in tests/test_cfn.py.  write_cfn_text and the functions above it are plain
Python loops (small problems only); write_cfn_text_np below restates the same export in numpy
for thousands of states and is held against the loops bit for bit and against brute-force
enumeration (tests/test_cfn.py).

The super-sequence is given element-wise: value[e] (flat observation index), comp[e] (the
active constraint component, -1 = none: MetaElements::is_constrained), first[e] (t == 0:
MetaElements::transitions returns the constant pi vector, utils.rs:32-38).  pi[N], a[N][N],
b[N][V] are log10 (the HMM as decoded).  All arithmetic is Python float (IEEE f64), in the
reference's order: (row + transitions) elementwise, max, then + emission.
"""
from __future__ import annotations

import math
from decimal import Decimal

import numpy as np

NEG = -math.inf


def rust_display(x: float) -> str:
    """Rust `format!("{}", f64)`: shortest round-trip digits, positional, inf / -inf / NaN."""
    if x != x:
        return "NaN"
    if math.isinf(x):
        return "inf" if x > 0 else "-inf"
    s = repr(float(x))  # the shortest round-trip digits; positional already for 1e-4 <= |x| < 1e16
    if "e" in s:
        s = format(Decimal(s), "f")
    if "." in s:
        s = s.rstrip("0").rstrip(".")
    return s


def _trans(pi, a, first, i, n):
    return pi[n] if first else a[i][n]


def _step(pi, a, b, row, value, first, states):
    """One element: for each n in `states`, max_i(row[i] + trans_i(n)) + b[n][value]."""
    N = len(pi)
    out = [NEG] * N
    for n in states:
        m = NEG
        for i in range(N):
            x = row[i] + _trans(pi, a, first, i, n)
            if x > m:
                m = x
        out[n] = m + b[n][value]
    return out


def longest_path(pi, a, b, value, comp, first, t_from, n_from, t_to, n_to):
    """cfn.rs:11-34."""
    N = len(pi)
    row = [NEG] * N
    row[n_from] = 0.0
    for t in range(t_from + 1, t_to + 1):
        if comp[t] >= 0:
            n = n_from if t < t_to else n_to
            row = _step(pi, a, b, row, value[t], first[t], [n])
        else:
            row = _step(pi, a, b, row, value[t], first[t], range(N))
    return max(row)


def unary_start(pi, a, b, value, comp, first, t_limit):
    """cfn.rs:36-53 (init_probs = pi + b[:, value[0]], hmm.rs:215-218)."""
    N = len(pi)
    row = [pi[n] + b[n][value[0]] for n in range(N)]
    for t in range(1, t_limit + 1):
        row = _step(pi, a, b, row, value[t], first[t], range(N))
    return row


def unary_end(pi, a, b, value, comp, first, t_start):
    """cfn.rs:55-80."""
    N = len(pi)
    L = len(value)
    if t_start == L - 1:
        return [0.0] * N
    out = []
    for n in range(N):
        row = [NEG] * N
        row[n] = 0.0
        for t in range(t_start + 1, L):
            if comp[t] >= 0:
                row = _step(pi, a, b, row, value[t], first[t], [n])
            else:
                row = _step(pi, a, b, row, value[t], first[t], range(N))
        out.append(max(row))
    return out


def write_cfn_text(pi, a, b, value, comp, first) -> str:
    """cfn.rs:82-205: the text of the .cfn file."""
    N = len(pi)
    L = len(value)
    bnd = []
    last = None
    for t in range(L):
        if comp[t] >= 0:
            c = comp[t]
            if last is None or c != last:
                bnd.append((t, c))
            last = c
    k = len({c for c in comp if c >= 0})  # number_constraints (utils.rs:200-202)
    tables = [[[[0.0] * N for _ in range(N)] for _ in range(k)] for _ in range(k)]
    for i in range(len(bnd) - 1):
        tf, cf = bnd[i]
        tt, ct = bnd[i + 1]
        for n1 in range(N):
            for n2 in range(N):
                cost = longest_path(pi, a, b, value, comp, first, tf, n1, tt, n2)
                if cost != NEG:
                    x = tables[cf][ct][n1][n2]
                    tables[cf][ct][n1][n2] = cost if x == 0.0 else x + cost
                    y = tables[ct][cf][n2][n1]
                    tables[ct][cf][n2][n1] = cost if y == 0.0 else y + cost
    unary = [[0.0] * N for _ in range(k)]
    f_time, f_cid = bnd[0]
    l_time, l_cid = bnd[-1]
    start = unary_start(pi, a, b, value, comp, first, f_time)
    unary[f_cid] = [u + s for u, s in zip(unary[f_cid], start)]
    end = unary_end(pi, a, b, value, comp, first, l_time)
    unary[l_cid] = [u + e for u, e in zip(unary[l_cid], end)]
    lb = -1.0
    for k1 in range(k):
        for k2 in range(k1 + 1, k):
            lb += min(min(r) for r in tables[k1][k2])
    for kk in range(k):
        unary[kk] = [lb if u == NEG else u for u in unary[kk]]

    def vec(v):
        return "[" + "".join(f"{rust_display(x)}{']' if q == len(v) - 1 else ','} " for q, x in enumerate(v))

    out = "{\n\tproblem: { name: consistent_viterbi, mustbe: >" + rust_display(lb) + "},\n"
    out += "\tvariables: {"
    dom = "[" + ",".join(f"s{i}" for i in range(N)) + "]"
    for i in range(k):
        out += f"n{i}: {dom}{',' if i != k - 1 else '},' + chr(10)}"
    out += "\tfunctions: {\n"
    for i in range(k):
        out += f"\t\tf{i}: {{ scope: [n{i}], costs: " + vec(unary[i]) + "}, \n"
        for j in range(i + 1, k):
            flat = [x for r in tables[i][j] for x in r]
            if sum_left_to_right(flat) != 0.0:
                out += f"\t\tf{i}_{j}: {{ scope: [n{i}, n{j}], costs: " + vec(flat) + "},\n"
    out += "\t}\n}"
    return out


def sum_left_to_right(flat) -> float:
    """tcost.sum() != 0.0 (cfn.rs:196), pinned here as the plain left-to-right f64 sum from 0.0.
    The built-in sum() is not that (compensated since Python 3.12), and neither is ndarray's
    (unrolled partial sums).  The order matters only for a mixed-sign table whose sum rounds to
    zero in one order and not in another: tables of log probabilities (entries <= 0) sum to zero
    only when every entry is zero, and [[1, 0], [0, -1]] sums to zero in every order."""
    s = 0.0
    for x in flat:
        s = s + x
    return s


# ---- the same export in numpy ------------------------------------------------------------
# A second restatement, vectorised so that problems of thousands of states can be checked.
# f64 only, the same order per step ((row + transitions) elementwise, max, + emission), the
# same first-t rule and forced-state rules.  Model entries are never +inf or NaN (the library's
# constructor rejects them) and the sums below stay below +inf, so no NaN arises and a max over
# f64 values does not depend on the order its candidates are met in.
#
# Shortcut 1 (all n_to at once).  longest_path's last step computes one column n_to of the
# free step (every other column stays -inf, so the final max(row) is that column), and the
# value of column n_to is max_i(row[i] + trans_i(n_to)) + b[n_to][value]: nothing in it depends
# on which n_to was asked for.  So one free step at t_to yields the costs to all n_to.
#
# Shortcut 2 (finite predecessors only).  A candidate row[i] + trans = -inf never passes
# `x > m` from m = -inf, and what passes is then an order-free max over the finite candidates;
# if none is finite the result is -inf, which is also what the restricted expression gives.
# A job's row starts with one finite entry (its start state s) and has at most that one finite
# entry again after every forced step (the forced state is s).  While the row is in that shape
# it is kept as the scalar x = row[s]: a forced step is (x + trans_s(s)) + b[s], a free step is
# (x + trans_s(n)) + b[n] for every n -- O(N) per job where the literal loop is O(N^2).
_TMP_ELEMS = 1 << 22  # elements of the largest temporary (32 MiB of f64)


class _Problem:
    def __init__(self, pi, a, b, value, comp, first):
        self.pi = np.ascontiguousarray(pi, np.float64)
        self.a = np.ascontiguousarray(a, np.float64)
        self.b = np.ascontiguousarray(b, np.float64)
        self.N = int(self.pi.shape[0])
        self.b = self.b.reshape(self.N, -1)
        self.value = [int(v) for v in value]
        self.comp = [int(c) for c in comp]
        self.first = [bool(f) for f in first]
        self.L = len(self.value)

    # -- one element for a block of jobs with start states st[B] ---------------------------
    def forced_one(self, st, x, t):
        tr = self.pi[st] if self.first[t] else self.a[st, st]
        return (x + tr) + self.b[st, self.value[t]]

    def free_one(self, st, x, t):
        tr = np.broadcast_to(self.pi, (len(st), self.N)) if self.first[t] else self.a[st]
        return (x[:, None] + tr) + self.b[:, self.value[t]][None, :]

    def forced_dense(self, st, R, t):
        tr = self.pi[st][:, None] if self.first[t] else self.a[:, st].T
        return (R + tr).max(axis=1) + self.b[st, self.value[t]]

    def free_dense(self, R, t):
        N, B = self.N, R.shape[0]
        T = np.broadcast_to(self.pi, (N, N)) if self.first[t] else self.a
        out = np.full((B, N), NEG)
        step = max(1, _TMP_ELEMS // (B * N))
        for i0 in range(0, N, step):
            i1 = min(N, i0 + step)
            np.maximum(out, (R[:, i0:i1, None] + T[None, i0:i1, :]).max(axis=1), out=out)
        return out + self.b[:, self.value[t]][None, :]

    def run(self, st, t_begin, t_last):
        """Elements t_begin+1 .. t_last for the jobs that start at (t_begin, st[r]) with score
        0, constrained elements forced to st[r].  Returns (x, None) while the rows hold their
        one entry at st, else (None, R)."""
        x, R = np.zeros(len(st)), None
        for t in range(t_begin + 1, t_last + 1):
            if self.comp[t] >= 0:
                x = self.forced_one(st, x, t) if R is None else self.forced_dense(st, R, t)
                R = None
            else:
                R = self.free_one(st, x, t) if R is None else self.free_dense(R, t)
                x = None
        return x, R

    def blocks(self, block=None):
        per = block or max(1, min(self.N, _TMP_ELEMS // self.N))
        for s0 in range(0, self.N, per):
            yield np.arange(s0, min(self.N, s0 + per))

    def segment_block(self, st, t_from, t_to):
        """longest_path(t_from, st[r], t_to, n) for every n: [B, N]."""
        x, R = self.run(st, t_from, t_to - 1)
        return self.free_one(st, x, t_to) if R is None else self.free_dense(R, t_to)

    def end_block(self, st, t_start):
        if t_start == self.L - 1:
            return np.zeros(len(st))
        x, R = self.run(st, t_start, self.L - 1)
        return x if R is None else R.max(axis=1)

    def start_row(self, t_limit):
        R = (self.pi + self.b[:, self.value[0]])[None, :]
        for t in range(1, t_limit + 1):
            R = self.free_dense(R, t)
        return R[0]



def boundaries(comp):
    """cfn.rs:88-110: (t, component) wherever the active component differs from the last one."""
    bnd, last = [], None
    for t, c in enumerate(comp):
        if c >= 0:
            if last is None or c != last:
                bnd.append((t, int(c)))
            last = c
    return bnd


def segment_rows_np(pi, a, b, value, comp, first, t_from, t_to, block=None):
    """[n_from, n_to] = longest_path(..., t_from, n_from, t_to, n_to) as an [N, N] f64 array."""
    p = _Problem(pi, a, b, value, comp, first)
    return np.concatenate([p.segment_block(st, t_from, t_to) for st in p.blocks(block)], axis=0)


def write_cfn_text_np(pi, a, b, value, comp, first, block=None, return_rows=False):
    """write_cfn_text in numpy: the same inputs (lists or arrays), the same text.  Start states
    go through in blocks of `block` (default: 32 MiB of rows), so peak memory is the model, the
    k*k tables and a few block-sized temporaries.  With return_rows, also returns
    {"bnd": [(t, component)], "seg": [[N, N] array per boundary pair, [n_from, n_to]],
     "end": [N], "start": [N]} -- the rows the tables and unary costs are built from."""
    p = _Problem(pi, a, b, value, comp, first)
    N = p.N
    bnd = boundaries(p.comp)
    k = len({c for c in p.comp if c >= 0})
    tables = np.zeros((k, k, N, N))
    rows = {"bnd": bnd, "seg": [], "end": None, "start": None}

    def acc(T, M):
        np.copyto(T, np.where(T == 0.0, M, T + M), where=(M != NEG))

    for i in range(len(bnd) - 1):
        (tf, cf), (tt, ct) = bnd[i], bnd[i + 1]
        keep = []
        for st in p.blocks(block):
            M = p.segment_block(st, tf, tt)
            acc(tables[cf, ct, st[0]:st[-1] + 1, :], M)
            acc(tables[ct, cf, :, st[0]:st[-1] + 1], M.T)
            if return_rows:
                keep.append(M)
        if return_rows:
            rows["seg"].append(np.concatenate(keep, axis=0))
    unary = np.zeros((k, N))
    (f_time, f_cid), (l_time, l_cid) = bnd[0], bnd[-1]
    start = p.start_row(f_time)
    end = np.concatenate([p.end_block(st, l_time) for st in p.blocks(block)])
    rows["start"], rows["end"] = start, end
    unary[f_cid] = unary[f_cid] + start
    unary[l_cid] = unary[l_cid] + end
    lb = -1.0
    for k1 in range(k):
        for k2 in range(k1 + 1, k):
            lb += float(tables[k1, k2].min())
    unary[unary == NEG] = lb

    def vec(v):
        return "[" + ", ".join(rust_display(x) for x in v.tolist()) + "] "

    out = ["{\n\tproblem: { name: consistent_viterbi, mustbe: >" + rust_display(lb) + "},\n\tvariables: {"]
    dom = "[" + ",".join(f"s{i}" for i in range(N)) + "]"
    out.append(",".join(f"n{i}: {dom}" for i in range(k)) + "},\n\tfunctions: {\n")
    for i in range(k):
        out.append(f"\t\tf{i}: {{ scope: [n{i}], costs: " + vec(unary[i]) + "}, \n")
        for j in range(i + 1, k):
            flat = tables[i, j].ravel()
            if sum_left_to_right(flat.tolist()) != 0.0:
                out.append(f"\t\tf{i}_{j}: {{ scope: [n{i}, n{j}], costs: " + vec(flat) + "},\n")
    out.append("\t}\n}")
    text = "".join(out)
    return (text, rows) if return_rows else text
