"""The start rule "mehrotra", host side: what tests/test_gpu_start_rule.py
relies on of its yardstick tests/pc_mehrotra_ref.py.  Without a GPU.

The least-squares point satisfies its defining equalities, every entry of the
start is > 0 on every case the GPU tests name, the b = c = 0 problem gives all
ones, and the restated pc iteration (pc_start_ref.solve_pc) from the start
ends optimal on every feasible case.  Its line counts, recorded here beside
the counts from "every variable 1000" (LINES; measured on the CPU, dense or
oracle back end as pc_mehrotra_ref.CASES says): the start saves three to
seven lines, and stocfor1 is a case it makes worse.
"""
import numpy as np
import pytest

import pc_mehrotra_ref as mr
import pc_start_ref as ps
import test_pc
from qp_ref import _mats

# name -> (lines from the rule's start, lines from the default start)
LINES = {
    "lp 3x5": (7, 14), "lp 1x64": (12, 15), "lp 63x65": (12, 19), "lp 200x40": (14, 20),
    "banded 63x65": (10, 17), "gaps 20x30": (10, 17), "lowrank 40x200": (14, 21), "diag 1x64": (9, 15),
    "afiro": (13, 16), "stocfor1": (23, 20), "afiro with Q": (14, 18),
}
# the toys of test_pc.toy_problems: the status they keep, and the lines it
# takes from the rule's start (the three without a solution take 11 from the
# default start: the blow-up tests compare a line with the one before, and a
# start on the problem's own scale leaves them less to see)
TOYS = {"infeasible_sum": (4, 17), "infeasible_bound": (4, 100), "unbounded": (2, 22), "bounded_by_q": (0, 7)}


def relerr(r, v):
    return np.abs(r).max() / max(1.0, np.abs(v).max())


@pytest.mark.parametrize("name", sorted(mr.CASES))
def test_least_squares_equalities(name):
    """Step 2's A x~ + w~ = b on every case, step 3's A'y~ - z~ = c on the
    LPs, to 1e-10 relative, before the shifts."""
    p, backend = mr.problem(name)
    A, Q = _mats(p)
    x, y, w, z = mr.least_squares(p, backend)
    rp, rd = relerr(A @ x + w - p.b, p.b), relerr(A.T @ y - z - p.c, p.c)
    print(name, rp, rd)
    assert rp <= 1e-10
    if Q is None:
        assert rd <= 1e-10
    else:
        # with Q the second solve's equality is A'y~ - (I + Q) z~ = c
        assert relerr(A.T @ y - z - Q @ z - p.c, p.c) <= 1e-10


@pytest.mark.parametrize("name", sorted(mr.CASES))
def test_start_is_positive_and_the_run_from_it_ends_optimal(name):
    p, s, run = mr.reference(name)
    assert all(np.all(np.isfinite(v)) and np.all(v > 0) for v in s)
    assert s[0].shape == s[3].shape == (p.n,) and s[1].shape == s[2].shape == (p.m,)
    default = ps.solve_pc(p, mr.CASES[name][2])
    print(name, run["status"], run["iters"], default["status"], default["iters"])
    assert run["status"] == 0 and default["status"] == 0
    assert abs(run["iters"] - LINES[name][0]) <= 1 and abs(default["iters"] - LINES[name][1]) <= 1


def test_zero_problem_gives_all_ones():
    p, backend = mr.problem(mr.ZERO)
    for v in mr.start(p, backend):
        assert np.array_equal(v, np.ones(v.size))


def test_shifts():
    """Steps 4 and 5 on a point worked by hand: min(x, w) = -2 gives
    delta_p = 3, min(y, z) = 1 gives delta_d = 0; then x = (4, 1), w = (5),
    y = (2), z = (1, 3): g = 4 + 3 + 10 = 17, Sp = 10, Sd = 6."""
    dp, dd, ep, ed = mr.shifts(np.array([1.0, -2.0]), np.array([2.0]), np.array([2.0]), np.array([1.0, 3.0]))
    assert (dp, dd) == (3.0, 0.0) and ep == 17.0 / 12.0 and ed == 17.0 / 20.0


@pytest.mark.parametrize("name", sorted(TOYS))
def test_toys_keep_their_status(name):
    p, status = test_pc.toy_problems()[name]
    assert status == TOYS[name][0]
    s = mr.start(p, "dense")
    assert all(np.all(v > 0) for v in s)
    r = ps.solve_pc(p, "dense", start=s)
    print(name, r["status"], r["iters"])
    assert r["status"] == status and abs(r["iters"] - TOYS[name][1]) <= 1
