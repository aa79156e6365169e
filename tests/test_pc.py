"""The predictor-corrector solver (method "pc"), host side: the conditions
on the inputs of tests/test_gpu_pc.py, and what its yardstick tests/pc_ref.py
is chosen for.  Without a GPU.

Cases.  Every problem tests/test_gpu_pc.py holds the device run to a
reference run on is named here (SMALL_CASES, LP_SHAPES, NETLIB_LPS,
test_qp_solver.NETLIB_SEEDS, DENSE_CASES, the two MPS files, FREE_LP), and
the reference ends optimal on it under its rounding variants -- the scheme
of test_qp_solver.variant_runs: the oracle back end with its factor's
elimination sums in plain, reverse and sorted order, each with A x, A'y and
Q x summed in the stored and in a random order, and for the small cases the
dense back end in three orders.  Line counts within 1 of each other; the
fp64 certificate of every variant's solution at most 1e-6.  The seeds are
test_qp_solver.SMALL_SEEDS' (scanned there for method "qp") and, for the
cases intpt's give-up tests could not take, 0, 1 and 2 unscanned; the
shapes with q removed take seed 0.  A problem without Q is solved on the
LP's own K by the oracle back end (pc_ref._OracleLp), as method "pc" does.

Replaced, each by another of its class.  What remains of give-ups with the
guard in place is the linear solve breaking down on a nearly dependent
system late in a solve, in one elimination order and not in another:
  * blend: 2 or 4 after 17-20 lines in four of the six oracle variants;
    adlittle (71 x 97) stands in.  share2b: optimal in all six, after 22 to
    30 lines; stocfor1 (180 x 111) stands in.  The stand-ins are the first
    of adlittle, sc205, scagr7, stocfor1, recipe, beaconfd (small netlib LPs
    in no other list here) that pass, sc205 set aside: the reference is
    stable on it (22 lines in all six variants), but on the device the
    refined KKT solve of this matrix leaves a larger dual residual than the
    oracle's in the middle of a run under intpt already (line 24 of 33:
    3.5e-5 against 7.2e-6, the dual objective 1.5e-3 apart at a tolerance
    of 7.6e-4), so it misses the line bar of test_gpu_pc.py with the
    existing method as with pc (line 16 of 22: 2.9e-4 against 2.3e-6; the
    worst line 69 times its tolerance; same line count, final objectives
    7e-8 apart).  That is KktDevice's, which method pc does not touch.  scagr7,
    recipe and beaconfd give up in two of their six variants; boeing2, the
    one problem left in rounding_stability.json's intpt-stable set, runs
    to the iteration limit under pc_ref.
  * the free-column LP: capri, the first of test_gpu_ipm.FREE_FAST, ends 2
    after 20 lines in two variants and modszk1 spreads over 32-34 lines;
    stair (optimal after 25 lines in all six) stands in.
(The grid-stride case of the GPU tests is held to its certificate alone, not
to a reference run, and is not run here.)

The guard.  intpt gives up when a printed residual norm exceeds ten times
the previous one.  A predictor-corrector takes full steps early, which
leaves both residuals at their rounding floor, and there the ratio of two
consecutive norms is noise.  pc asks in addition that the norm stand above
1e-6 (1 + its value on line 0).  test_relative_guard shows why the bound is
relative: with the solutions carrying Gaussian noise of 1e-13 max |solution|
per entry, the dual residual of (1, 64, diag) seed 1 rises from 3e-8 to
0.7e-6 .. 1.2e-6 on line 4, depending on the draw (3 of the first 40 noise
seeds cross 1e-6: 10, 13 and 31), and a plain 1e-6 in the bound's place then
ends "dual infeasible" on a problem that is feasible by construction.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import ipo_amd
import oracle_lib
import pc_ref
import qp_dense
import qp_ref
from conftest import REPO, mps_path
from test_qp_solver import NETLIB_SEEDS, SMALL_SEEDS, netlib_problem, write_qp_mps

# (m, n, kind, seed): test_qp_solver's cases at its seeds, then the cases
# method "qp" has no stable seed for (test_qp_solver's docstring) and the
# one-row shape, at seeds taken as they come
HARD_CASES = ([(3, 5, "gaps", s) for s in (0, 1, 2)] + [(40, 200, "diag", s) for s in (0, 1, 2)]
              + [(40, 200, "lowrank", s) for s in (0, 1, 2)] + [(1, 64, k, 0) for k in qp_ref.Q_KINDS])
SMALL_CASES = sorted((m, n, kind, seed) for (m, n, kind), seed in SMALL_SEEDS.items()) + HARD_CASES
# (m, n, seed) of the shapes run with q removed
LP_SHAPES = ((3, 5, 0), (20, 30, 0), (63, 65, 0), (40, 200, 0), (200, 40, 0), (1, 64, 0))
# adlittle for blend, stocfor1 for share2b (module docstring)
NETLIB_LPS = ("afiro", "sc50a", "sc50b", "sc105", "kb2", "sctap1", "adlittle", "stocfor1", "scsd1")
DENSE_CASES = ((300, 257, "factor"), (300, 260, "arrow"))
FREE_LP = "stair"       # free columns: test_free_vars.FREE, test_gpu_ipm.FREE_FAST

OPT = json.load(open(os.path.join(REPO, "tests", "golden", "netlib_optima.json")))["problems"]


def small_case(m, n, kind, seed):
    return qp_ref.make_qp(m, n, kind, seed)


def lp_shape(m, n, seed):
    """make_qp(m, n, "diag", seed) with q removed: Q x* stays in c, another feasible bounded LP."""
    p = qp_ref.make_qp(m, n, "diag", seed)
    return ipo_amd.SolverForm(p.m, p.n, p.kA, p.iA, p.A, p.b, p.c, p.f)


def netlib_lp(name):
    return ipo_amd.load_mps(mps_path(name))


def free_lp(name):
    return ipo_amd.load_mps(mps_path(name), free="split")


def netlib_distance(name, ref):
    """How far the reference run's last line ends from the netlib optimum,
    relative (the printed objective is -sense times the file's)."""
    o = OPT[name]
    target = -o["sense"] * o["optimum"]
    return max(abs(ref["rows"][-1][1] - target), abs(ref["rows"][-1][3] - target)) / max(1.0, abs(target)), target


# ---------------------------------------------------------------- toy problems
def _form(M, b, c, q=None):
    kA, iA, A = qp_ref.csc_of(np.array(M, np.float64))
    return ipo_amd.SolverForm(len(b), len(c), kA, iA, A, np.array(b, np.float64), np.array(c, np.float64), 0.0, q=q)


def toy_problems():
    """(problem, status): x1 + x2 <= 1 with x1 + x2 >= 2, and x1 <= 1 with
    x1 >= 2 beside a free row (both infeasible; 4, the status intpt ends them
    with); max x1 + x2, x1 - x2 <= 1 (unbounded; 2, as intpt); and the last
    with - |x|^2 / 2 in the objective: x = (1, 1), objective 1."""
    return {
        "infeasible_sum": (_form([[1.0, 1.0], [-1.0, -1.0]], [1.0, -2.0], [1.0, 1.0]), 4),
        "infeasible_bound": (_form([[1.0, 0.0], [-1.0, 0.0], [0.0, 1.0]], [1.0, -2.0, 3.0], [1.0, 2.0]), 4),
        "unbounded": (_form([[1.0, -1.0]], [1.0], [1.0, 1.0]), 2),
        "bounded_by_q": (_form([[1.0, -1.0]], [1.0], [1.0, 1.0], q=qp_ref.csc_of(np.eye(2))), 0),
    }


# ---------------------------------------------------------------- stability of the reference
def variant_runs(p, dense):
    """pc_ref under its rounding variants (module docstring), plain run first."""
    L = oracle_lib.lib()
    runs = []
    try:
        for perturb in (0, 1, 2):
            L.orc_set_perturb(perturb)
            runs += [pc_ref.solve_pc(p, "oracle", shuffle=sh) for sh in (None, 1)]
    finally:
        L.orc_set_perturb(0)
    if dense:
        runs = [pc_ref.solve_pc(p, "dense", shuffle=sh) for sh in (None, 1, 2)] + runs
    return runs


def _stable(p, dense):
    runs = variant_runs(p, dense)
    certs = [qp_ref.certificate(p, r["x"], r["y"], r["w"], r["z"]) for r in runs]
    print([(r["status"], r["iters"]) for r in runs], f"worst certificate entry {max(max(c[:3]) for c in certs):.3e}")
    assert all(r["status"] == 0 for r in runs), [(r["status"], r["iters"]) for r in runs]
    assert max(r["iters"] for r in runs) - min(r["iters"] for r in runs) <= 1
    for pr, du, gap, lo in certs:
        assert pr <= 1e-6 and du <= 1e-6 and gap <= 1e-6 and lo > 0, (pr, du, gap, lo)
    return runs


@pytest.mark.parametrize("m,n,kind,seed", SMALL_CASES)
def test_reference_stable_on_small_cases(m, n, kind, seed):
    _stable(small_case(m, n, kind, seed), True)


@pytest.mark.parametrize("m,n,seed", LP_SHAPES)
def test_reference_stable_on_lp_shapes(m, n, seed):
    _stable(lp_shape(m, n, seed), True)


@pytest.mark.parametrize("name", NETLIB_LPS)
def test_reference_stable_on_netlib_lps(name):
    """Also prints the distance test_gpu_pc.py's bar on the final objective is
    made of: where the plain oracle run (pc_ref.reference's) ends from the
    netlib optimum."""
    p = netlib_lp(name)
    runs = _stable(p, False)
    dist, target = netlib_distance(name, runs[0])
    print(f"{name}: reference ends {dist:.3e} (relative) from the netlib optimum {target!r}")
    assert dist <= 1e-5            # test_oracle_optima's bar for the reference's own methods


@pytest.mark.parametrize("name", sorted(NETLIB_SEEDS))
def test_reference_stable_on_netlib_patterns(name):
    _stable(netlib_problem(name), False)


@pytest.mark.parametrize("m,n,kind", DENSE_CASES)
def test_reference_stable_on_long_columns(m, n, kind):
    _stable(qp_dense.dense_problem(m, n, kind), True)


@pytest.mark.parametrize("sense", ["MIN", "MAX"])
def test_reference_stable_on_the_mps_files(tmp_path, sense):
    _stable(ipo_amd.load_mps_qp(write_qp_mps(tmp_path, sense)), True)


def test_reference_stable_on_the_free_column_lp():
    _stable(free_lp(FREE_LP), False)


# ---------------------------------------------------------------- what pc is for
@pytest.mark.parametrize("m,n,kind", sorted(SMALL_SEEDS))
def test_fewer_lines_than_qp(m, n, kind):
    p, ref = pc_ref.reference((m, n, kind, SMALL_SEEDS[(m, n, kind)]), small_case, "dense")
    q = qp_ref.solve_qp(p, "dense")
    print(ref["iters"], q["iters"])
    assert ref["status"] == q["status"] == 0 and ref["iters"] < q["iters"]


def test_cases_intpt_could_not_take():
    """Every HARD_CASES problem ends optimal; method "qp"'s iteration gives up
    ("primal infeasible") on some of these feasible problems."""
    gave_up = []
    for key in HARD_CASES:
        p, ref = pc_ref.reference(key, small_case, "dense")
        assert ref["status"] == 0, key
        if qp_ref.solve_qp(p, "dense")["status"] == 2:
            gave_up.append(key)
    print("qp_ref ends status 2 on", gave_up)
    assert gave_up


@pytest.mark.parametrize("name", sorted(toy_problems()))
def test_toy_problems(name):
    p, status = toy_problems()[name]
    r = pc_ref.solve_pc(p, "dense")
    print(r["status"], r["iters"], r["rows"][-1])
    assert r["status"] == status
    if status == 0:
        assert abs(r["rows"][-1][1] - 1.0) <= 1e-6 and abs(r["rows"][-1][3] - 1.0) <= 1e-6
        assert np.allclose(r["x"], [1.0, 1.0], atol=1e-6)


NOISE_SEED = 10      # the first draw that crosses 1e-6 (module docstring)


def test_relative_guard():
    p = qp_ref.make_qp(1, 64, "diag", 1)
    runs = {g: pc_ref.solve_pc(p, pc_ref.Noisy(qp_ref._Dense(p), NOISE_SEED), guard=g) for g in ("relative", "absolute")}
    for g, r in runs.items():
        print(g, r["status"], r["iters"], [f"{row[4]:.1e}" for row in r["rows"][:8]])
    assert runs["relative"]["status"] == 0
    assert runs["absolute"]["status"] == 4 and runs["absolute"]["rows"][-1][0] <= 6
    # whatever the draw, the rule as specified ends optimal on the same line
    exact = pc_ref.solve_pc(p, "dense")
    for seed in range(NOISE_SEED):
        r = pc_ref.solve_pc(p, pc_ref.Noisy(qp_ref._Dense(p), seed))
        assert r["status"] == 0 and r["iters"] == exact["iters"]


# ---------------------------------------------------------------- the ABI's refusals
def test_solve_qp_ex_refuses_lp_methods():
    """ipo_hip_solve_qp_ex takes methods 3 and 4; anything else is 7 with a
    message before any device call (this runs without a GPU)."""
    p = qp_ref.make_qp(3, 12, "diag", 0)
    L = ipo_amd.lib()
    kA, iA, A = (np.ascontiguousarray(a) for a in (p.kA, p.iA, p.A))
    kQ, iQ, Q = ipo_amd._q_arrays(p.q)
    x, z, y, w = np.zeros(p.n), np.zeros(p.n), np.zeros(p.m), np.zeros(p.m)
    for method in (0, 1, 2, 5, -1):
        st = ipo_amd.Stats()
        rc = L.ipo_hip_solve_qp_ex(method, p.m, p.n, p.nz, iA.ctypes.data, kA.ctypes.data, A.ctypes.data,
                                   p.b.ctypes.data, p.c.ctypes.data, 0.0, kQ.ctypes.data, iQ.ctypes.data, Q.ctypes.data,
                                   x.ctypes.data, y.ctypes.data, w.ctypes.data, z.ctypes.data, None, 0, 0, C.byref(st))
        assert rc == 7 and st.iters == 0 and "method" in ipo_amd.last_error()
    assert ipo_amd.METHODS["pc"] == 4 and "ipo_hip_solve_qp_ex" in ipo_amd.EXPORTED
