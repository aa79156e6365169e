"""The QP path-following solver (method "qp"), host side.

Method "qp" is an extension (the reference has no QP loop); its yardstick
is tests/qp_ref.py.  Here, without a GPU:

  * the QP normalisation (lp_io.cpp to_solver_form_qp through
    ipo_hip_mps_load_qp) against a transform computed by hand, on a MIN and
    a MAX file with a nonzero lower bound, upper bounds, an E row and a
    ranged row;
  * ipo_hip_solve_qp refuses an invalid Q with 7 and validate_q's message,
    before it touches a device;
  * the conditions on the inputs of tests/test_gpu_qp_solver.py: the
    reference iteration ends "optimal" on every case the GPU tests name, and
    does so under every rounding variant tried here (below).

Rounding stability.  intpt.c gives up when a printed residual norm grows
tenfold in one iteration (intpt.c:175-182).  Late in a solve the residuals
are what rounding and the refined solve's stopping rule (1e-10 of the
right-hand side, ldlt.c:401-416) leave of them, and whether such a value
exceeds ten times the previous one depends on the order of the sums: of 20
(shape, kind) pairs at the first seed tried, 7 ended "infeasible" in the
reference and others did so in one of its variants.  Such a case says
nothing about the device code.  Every case named here therefore ends
optimal, within one iteration of each other, in all of the reference's
variants: the oracle back end with its factor's elimination sums in plain,
reverse and sorted order (orc_set_perturb, as tools/order_stability.py does
for the LP methods), each with A x, A'y and Q x summed in the stored and in
a random order, and (small cases) the dense back end in three orders; with
no residual ever growing by more than STABLE_GROWTH = 5, half of what fires
the test; and the residual the refined solve may leave in each entry of the
last Newton system, 1e-10 (max |right-hand side| + 1) (ldlt.c:367-416;
qp_ref's "floor"), is below the stop rule's 1e-6 -- where it is not, whether
the stop rule is met at all is a matter of rounding (israel: 6.2e-5).
Seeds were scanned from 0 upwards for the first that meets this.  A case
that has none is replaced, not dropped: (3, 5, gaps) has none below 60 and
(4, 6, gaps) stands in; (40, 200, diag) and (40, 200, lowrank) have none
below 140, and (48, 200, diag) and (40, 240, lowrank) stand in; NETLIB_SEEDS
says what became of the netlib patterns.

The budget projection (max a'x - x'x / 2, sum x <= 1) has one row: its
primal residual is one rounding error, often exactly zero, and the give-up
test fires on the next nonzero value in most of the reference's variants
(which ones depends on the host's BLAS).  It is kept as the closed-form
case: the iteration without its give-up tests reaches x = e_4, y = 2, and
the device run is held to that run, to status 0 and to the closed form.
"""
import ctypes as C
import os

import numpy as np
import pytest

import ipo_amd
import oracle_lib
import qp_ref
from test_qp import _card, random_q

STABLE_GROWTH = 5.0

# (m, n, kind) -> seed (the module docstring's scan)
SMALL_SEEDS = {
    (3, 5, "diag"): 59, (3, 5, "banded"): 37, (3, 5, "lowrank"): 53,
    (20, 30, "diag"): 5, (20, 30, "banded"): 12, (20, 30, "lowrank"): 10, (20, 30, "gaps"): 2,
    (63, 65, "diag"): 12, (63, 65, "banded"): 12, (63, 65, "lowrank"): 1, (63, 65, "gaps"): 12,
    (40, 200, "banded"): 2, (40, 200, "gaps"): 5,
    # for (3, 5, gaps), (40, 200, diag) and (40, 200, lowrank): module docstring
    (4, 6, "gaps"): 3, (48, 200, "diag"): 1, (40, 240, "lowrank"): 37,
    (200, 40, "diag"): 0, (200, 40, "banded"): 0, (200, 40, "lowrank"): 0, (200, 40, "gaps"): 0,
}
# netlib patterns with a Q on their columns, (kind of Q, seed): the first
# seed that is stable in the sense above, make_q(n, "banded", seed) being
# random_q(n, seed).  afiro and sc50a have none below 60 (85 and 81 are the
# first).  israel (entries up to 1e6) has none: where every variant ends
# optimal (seed 23) its refined solve may leave 6.2e-5 per entry, above the
# stop rule's 1e-6, and elsewhere a variant ends 2 or 4; scsd1 (154 x 760)
# and kb2 stand in.  25fv47 with a diagonal Q has none below 40 (a residual
# at its floor grows tenfold in one variant or another); scsd6 (294 x 1350)
# takes the diagonal Q.
NETLIB_SEEDS = {"afiro": ("banded", 85), "sc50a": ("banded", 81), "blend": ("banded", 0), "share2b": ("banded", 1),
                "kb2": ("banded", 0), "scsd1": ("banded", 0), "scsd6": ("diag", 0)}


# ---------------------------------------------------------------- the MPS files
def qp_mps(sense):
    """MIN: minimise c'x + x'Qx / 2 with c = (1, 2, -1, 0.5) and test_qp's Q;
    MAX: maximise its negative (every objective and QUADS entry negated).
    0.25 <= x1 + x2 <= 4 (ranged L row), x1 + x4 >= 1, -x2 + x3 = 4,
    0.5 <= x1 <= 4, x3 <= 10.  Optimum x = (0.5, 0, 4, 0.5), objective
    9.0625: x1 at its lower bound, x4 from LIM2, x3 from MYEQN (gradient
    c + Q x = (1.875, 2.25, 5, 0.875): every reduced cost positive).  The
    right-hand side 4 of MYEQN is the stable one of those tried (7, 1 and 8
    end "dual infeasible" in some variant of the reference)."""
    s = 1.0 if sense == "MIN" else -1.0
    return (("" if sense == "MIN" else "MAX\n")
            + "NAME          QPSOLVE\nROWS\n N  COST\n L  LIM1\n G  LIM2\n E  MYEQN\nCOLUMNS\n"
            + _card("", "X1", "COST", s * 1.0, "LIM1", 1.0) + _card("", "X1", "LIM2", 1.0)
            + _card("", "X2", "COST", s * 2.0, "LIM1", 1.0) + _card("", "X2", "MYEQN", -1.0)
            + _card("", "X3", "COST", s * -1.0, "MYEQN", 1.0) + _card("", "X4", "COST", s * 0.5, "LIM2", 1.0)
            + "RHS\n" + _card("", "RHS", "LIM1", 4.0, "LIM2", 1.0) + _card("", "RHS", "MYEQN", 4.0)
            + "RANGES\n" + _card("", "RNG", "LIM1", 3.75)
            + "BOUNDS\n" + _card("UP", "BND", "X1", 4.0) + _card("LO", "BND", "X1", 0.5) + _card("UP", "BND", "X3", 10.0)
            + "QUADS\n" + _card("", "X1", "X1", s * 2.0, "X2", s * 0.5) + _card("", "X1", "X4", s * -0.25)
            + _card("", "X2", "X2", s * 3.0) + _card("", "X3", "X3", s * 1.5) + _card("", "X4", "X4", s * 1.0)
            + "ENDATA\n")


QP_C = np.array([1.0, 2.0, -1.0, 0.5])
QP_Q = np.array([[2.0, 0.5, 0.0, -0.25], [0.5, 3.0, 0.0, 0.0], [0.0, 0.0, 1.5, 0.0], [-0.25, 0.0, 0.0, 1.0]])
QP_L = np.array([0.5, 0.0, 0.0, 0.0])
QP_X = np.array([0.5, 0.0, 4.0, 0.5])
QP_OBJ = 9.0625


def write_qp_mps(tmp_path, sense):
    path = os.path.join(str(tmp_path), f"qp_{sense.lower()}.mps")
    with open(path, "w") as fh:
        fh.write(qp_mps(sense))
    return path


@pytest.mark.parametrize("sense", ["MIN", "MAX"])
def test_qp_normalisation_by_hand(tmp_path, sense):
    path = write_qp_mps(tmp_path, sense)
    qp, lp = ipo_amd.load_mps_qp(path), ipo_amd.load_mps(path)
    # rows, ranges and bounds exactly the LP transform's; the column count too
    assert (qp.m, qp.n) == (lp.m, lp.n) == (7, 4)      # 3 rows + the ranged row's copy + E's copy + 2 upper bounds
    for a, b in ((qp.kA, lp.kA), (qp.iA, lp.iA), (qp.A, lp.A), (qp.b, lp.b)):
        assert np.array_equal(a, b)
    # by hand: Q l = (1, 0.25, 0, -0.125), c + Q l = (2, 2.25, -1, 0.375),
    # c'l = 0.5, l'Q l / 2 = 0.25.  MIN negates c and f; the MAX file holds
    # -c and -Q and is not negated: the same solver form either way
    assert np.array_equal(QP_Q @ QP_L, [1.0, 0.25, 0.0, -0.125])
    assert np.array_equal(qp.c, [-2.0, -2.25, 1.0, -0.375])
    assert qp.f == -0.75
    assert np.array_equal(lp.c, -QP_C) and lp.f == -0.5          # the LP entry still ignores QUADS
    # Q_s = sense Q_file (sense 1 MIN, -1 MAX) = Q here in both files
    fileq = qp_ref.q_dense(4, ipo_amd.mps_quads(path))
    assert np.array_equal(fileq, QP_Q if sense == "MIN" else -QP_Q)
    assert np.array_equal(qp_ref.q_dense(4, qp.q), QP_Q)
    kQ, iQ, _ = qp.q
    assert all(np.all(np.diff(iQ[kQ[j]:kQ[j + 1]]) > 0) for j in range(4))


def test_load_qp_without_quads_is_the_lp(tmp_path):
    path = os.path.join(str(tmp_path), "lp.mps")
    with open(path, "w") as fh:
        fh.write(qp_mps("MIN").split("QUADS")[0] + "ENDATA\n")
    qp, lp = ipo_amd.load_mps_qp(path), ipo_amd.load_mps(path)
    assert np.array_equal(qp.c, lp.c) and qp.f == lp.f and np.array_equal(qp.b, lp.b)
    assert np.array_equal(qp.q[0], np.zeros(5, np.int32)) and qp.q[1].size == 0


def test_solve_qp_validates_q():
    """validate_q through ipo_hip_solve_qp: 7 and test_set_q_validates_input's
    messages, before any device call (this runs without a GPU)."""
    p = qp_ref.make_qp(3, 12, "diag", 0)
    L = ipo_amd.lib()
    kA, iA, A = (np.ascontiguousarray(a) for a in (p.kA, p.iA, p.A))
    x, z, y, w = np.zeros(p.n), np.zeros(p.n), np.zeros(p.m), np.zeros(p.m)

    def solve(kQ, iQ, Q):
        kQ, iQ, Q = (np.ascontiguousarray(kQ, np.int32), np.ascontiguousarray(iQ, np.int32),
                     np.ascontiguousarray(Q, np.float64))
        st = ipo_amd.Stats()
        rc = L.ipo_hip_solve_qp(p.m, p.n, p.nz, iA.ctypes.data, kA.ctypes.data, A.ctypes.data, p.b.ctypes.data,
                                p.c.ctypes.data, 0.0, kQ.ctypes.data, iQ.ctypes.data, Q.ctypes.data, x.ctypes.data,
                                y.ctypes.data, w.ctypes.data, z.ctypes.data, None, 0, 0, C.byref(st))
        return rc, ipo_amd.last_error()

    kQ, iQ, Q = random_q(12, 3)
    bad_row = iQ.copy(); bad_row[2] = 12
    rc, msg = solve(kQ, bad_row, Q)
    assert rc == 7 and "out of range" in msg
    j = next(j for j in range(12) if kQ[j + 1] - kQ[j] >= 2)
    unsorted = iQ.copy(); unsorted[kQ[j]], unsorted[kQ[j] + 1] = unsorted[kQ[j] + 1], unsorted[kQ[j]]
    rc, msg = solve(kQ, unsorted, Q)
    assert rc == 7 and "ascending" in msg
    asym = Q.copy()
    k = next(k for k in range(kQ[j], kQ[j + 1]) if iQ[k] != j)
    asym[k] += 1.0
    rc, msg = solve(kQ, iQ, asym)
    assert rc == 7 and "symmetric" in msg
    bad_k = kQ.copy(); bad_k[0] = 1
    rc, msg = solve(bad_k, iQ, Q)
    assert rc == 7 and "kQ[0]" in msg


# ---------------------------------------------------------------- conditions on the GPU tests' inputs
def small_problem(m, n, kind):
    return qp_ref.make_qp(m, n, kind, SMALL_SEEDS[(m, n, kind)])


def netlib_problem(name):
    from conftest import mps_path
    p = ipo_amd.load_mps(mps_path(name))
    kind, seed = NETLIB_SEEDS[name]
    return qp_ref.with_q(p, qp_ref.make_q(p.n, kind, seed))


def variant_runs(p, dense):
    """The reference under its rounding variants (module docstring), plain run first."""
    L = oracle_lib.lib()
    runs = []
    try:
        for perturb in (0, 1, 2):
            L.orc_set_perturb(perturb)
            runs += [qp_ref.solve_qp(p, "oracle", shuffle=sh) for sh in (None, 1)]
    finally:
        L.orc_set_perturb(0)
    if dense:
        runs = [qp_ref.solve_qp(p, "dense", shuffle=sh) for sh in (None, 1, 2)] + runs
    return runs


def _stable(p, dense):
    runs = variant_runs(p, dense)
    assert max(r["floor"] for r in runs) < 1e-6, [r["floor"] for r in runs]
    assert all(r["status"] == 0 for r in runs), [(r["status"], r["iters"]) for r in runs]
    assert max(r["growth"] for r in runs) <= STABLE_GROWTH, [r["growth"] for r in runs]
    assert max(r["iters"] for r in runs) - min(r["iters"] for r in runs) <= 1
    return runs[0]


@pytest.mark.parametrize("m,n,kind", sorted(SMALL_SEEDS))
def test_reference_converges_on_small_cases(m, n, kind):
    p = small_problem(m, n, kind)
    r = _stable(p, True)
    pr, du, gap, lo = qp_ref.certificate(p, r["x"], r["y"], r["w"], r["z"])
    assert pr <= 1e-6 and du <= 1e-6 and gap <= 1e-6 and lo > 0


@pytest.mark.parametrize("name", sorted(NETLIB_SEEDS))
def test_reference_converges_on_netlib_patterns(name):
    _stable(netlib_problem(name), False)


def test_budget_projection_closed_form():
    """The iteration reaches x = e_4, y = 2, objective 2.5; whether a run gets
    there or trips the growth test on the way is rounding (module docstring),
    so the closed form is checked on the iteration without its give-up tests."""
    p = qp_ref.budget_projection()
    runs = [qp_ref.solve_qp(p, be, shuffle=sh) for be in ("dense", "oracle") for sh in (None, 1, 2)]
    assert {r["status"] for r in runs} <= {0, 2}
    r = qp_ref.solve_qp(p, "dense", giveup=False)
    assert r["status"] == 0
    assert np.allclose(r["x"], [0, 0, 0, 1, 0], atol=1e-6) and abs(r["y"][0] - 2.0) <= 1e-6
    assert abs(r["rows"][-1][1] - 2.5) <= 2.5e-6 and abs(r["rows"][-1][3] - 2.5) <= 2.5e-6


@pytest.mark.parametrize("sense", ["MIN", "MAX"])
def test_reference_converges_on_the_mps_files(tmp_path, sense):
    p = ipo_amd.load_mps_qp(write_qp_mps(tmp_path, sense))
    r = _stable(p, True)
    assert np.allclose(r["x"] + QP_L, QP_X, atol=1e-6)
    # the printed objective is solver form's, -sense times the file's: -9.0625 for both files
    assert abs(r["rows"][-1][1] + QP_OBJ) <= 1e-6 * QP_OBJ
