"""QPs with long columns of Q, host side: the conditions on the inputs of
tests/test_gpu_qp_dense.py, as tests/test_qp_solver.py states them for its
own cases (its module docstring: rounding stability).

  * every case of qp_dense.DENSE_SEEDS passes test_qp_solver._stable with the
    dense back end included (status 0 in all nine rounding variants, iteration
    counts within 1, growth <= 5, floor < 1e-6), and its fp64 certificate is
    <= 1e-6;
  * its Q has the column lengths the GPU tests count on;
  * no case of test_qp_solver's SMALL_SEEDS / NETLIB_SEEDS has a column of Q of
    kLongQCol = 256 entries: the default IPO_HIP_Q_LONG changes none of their
    results.
"""
import numpy as np
import pytest

import qp_dense
import qp_ref
import test_qp_solver
from test_qp_solver import NETLIB_SEEDS, SMALL_SEEDS, netlib_problem, small_problem

LONG_Q_COL = 256      # csrc/kkt_knobs.h kLongQCol


@pytest.mark.parametrize("m,n,kind", sorted(qp_dense.DENSE_SEEDS))
def test_reference_converges_on_dense_cases(m, n, kind):
    p = qp_dense.dense_problem(m, n, kind)
    r = test_qp_solver._stable(p, True)
    pr, du, gap, lo = qp_ref.certificate(p, r["x"], r["y"], r["w"], r["z"])
    print(f"({m}, {n}, {kind}): {r['iters']} iterations, certificate {pr:.2e} {du:.2e} {gap:.2e}")
    assert pr <= 1e-6 and du <= 1e-6 and gap <= 1e-6 and lo > 0


@pytest.mark.parametrize("m,n,kind", sorted(qp_dense.DENSE_SEEDS))
def test_dense_cases_have_long_columns(m, n, kind):
    q = qp_dense.dense_problem(m, n, kind).q
    lens = qp_dense.column_lengths(q)
    M = qp_ref.q_dense(n, q)
    assert np.array_equal(M, M.T)
    if kind == "factor":
        assert np.all(lens == n) and n >= LONG_Q_COL
    else:
        assert np.all(lens[:3] == n - 2) and np.all(lens[3:] == 4) and n - 2 >= LONG_Q_COL
        d = np.abs(np.diag(M))
        assert np.all(d > np.abs(M).sum(0) - d)         # diagonally dominant: PSD


def test_existing_cases_have_no_long_column():
    longest = {}
    for key in sorted(SMALL_SEEDS):
        longest[key] = int(qp_dense.column_lengths(small_problem(*key).q).max())
    for name in sorted(NETLIB_SEEDS):
        longest[name] = int(qp_dense.column_lengths(netlib_problem(name).q).max())
    assert max(longest.values()) < LONG_Q_COL, longest
    assert longest[(40, 240, "lowrank")] == 240
