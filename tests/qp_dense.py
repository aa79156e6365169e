"""QPs whose Q has long columns (a plain module, no fixtures): the inputs of
tests/test_qp_dense.py and tests/test_gpu_qp_dense.py, and of
tools/qp_dense_time.py's problems in the large.

A column of Q with at least IPO_HIP_Q_LONG entries (default 256) is summed by
one wave instead of one thread (csrc/dev_common.h launch_q_long).  No case of
tests/test_qp_solver.py has such a column; these do:

  "factor"  a factor-model covariance F F' / 4 + diag, F n x 4: every column
            has n entries, all of them long from n = 256;
  "arrow"   three dense rows and columns in an otherwise diagonal Q,
            diagonally dominant (hence PSD): columns 0-2 have n - 2 entries,
            the others 4.

make_qp_dense repeats qp_ref.make_qp's draws in their order, so A, the
interior point, b and c - Q x* are make_qp's for the same (m, n, seed); only
Q differs.
"""
import numpy as np

import ipo_amd
import qp_ref

DENSE_KINDS = ("factor", "arrow")

# (m, n, kind) -> seed: the first from 0 that test_qp_solver._stable accepts
# (tests/test_qp_dense.py holds each to it).  Shapes with m < n were unstable
# at every seed tried ((40, 300, arrow) 1-39, (40, 320, factor) 0-11), as
# test_qp_solver.py found for (40, 200).
DENSE_SEEDS = {
    (300, 257, "factor"): 0,
    (400, 320, "factor"): 1,
    (300, 260, "arrow"): 1,
    (330, 321, "arrow"): 1,
}


def make_q_dense(n, kind, seed):
    """(kQ, iQ, Q) of the module docstring's kinds, symmetric bit for bit."""
    if kind == "factor":
        rng = np.random.default_rng([seed, n, 7])
        F = rng.uniform(-1.0, 1.0, (n, 4))
        M = np.triu(F @ F.T / 4 + np.diag(rng.uniform(0.1, 2.0, n)))
        return qp_ref.csc_of(M + np.triu(M, 1).T)
    if kind == "arrow":
        rng = np.random.default_rng([seed, n, 8])
        M = np.zeros((n, n))
        M[:3, :] = rng.uniform(-0.1, 0.1, (3, n))
        M[:, :3] = 0.0
        M = M + M.T
        M[np.diag_indices(n)] = np.abs(M).sum(0) + rng.uniform(0.5, 1.5, n)
        return qp_ref.csc_of(M)
    raise ValueError(kind)


def make_qp_dense(m, n, kind, seed):
    """qp_ref.make_qp(m, n, ., seed) with make_q_dense's Q."""
    rng = np.random.default_rng([seed, m, n])
    M = np.zeros((m, n))
    M[0, :] = rng.uniform(0.5, 1.5, n)
    for i in range(1, m):
        M[i, i % n] = rng.uniform(0.5, 1.5) * rng.choice([-1.0, 1.0])
    if m > 1:
        for j in range(n):
            for i in rng.integers(1, m, 2):
                M[i, j] = rng.uniform(0.5, 1.5) * rng.choice([-1.0, 1.0])
    q = make_q_dense(n, kind, seed)
    xs, zs = rng.uniform(0.5, 1.5, n), rng.uniform(0.5, 1.5, n)
    ys, ws = rng.uniform(0.5, 1.5, m), rng.uniform(0.5, 1.5, m)
    b = M @ xs + ws
    c = M.T @ ys - zs + qp_ref.q_dense(n, q) @ xs
    kA, iA, A = qp_ref.csc_of(M)
    return ipo_amd.SolverForm(m, n, kA, iA, A, b, c, 0.0, q=q)


def dense_problem(m, n, kind):
    return make_qp_dense(m, n, kind, DENSE_SEEDS[(m, n, kind)])


def column_lengths(q):
    return np.diff(np.asarray(q[0]))
