"""The QP path-following solver (method "qp") on the GPU, against its
yardstick tests/qp_ref.py (the reference has no QP loop: an extension).

The cases, their seeds and why they were chosen (rounding-stable under the
reference's own variants) are tests/test_qp_solver.py's.  Against the
reference run of the same problem:
  * the same status (0) and the printed line count within +-1;
  * every printed line's objectives to DESIGN.md section 3's bar for intpt,
    max(1e-5 relative, 0.1 x the line's progress);
  * the final objectives to 1e-6 relative (the bar of tests/test_synth.py).
Independent of the method, the optimality certificate recomputed in fp64
from the downloaded x, y, w, z: both residual norms and z'x + y'w at most
2e-6 (the stop rule's 1e-6; the factor 2 covers the loop's single-precision
cast of the norms and the recomputation's rounding), every entry positive.
"""
import json
import os

import numpy as np
import pytest

import ipo_amd
import qp_ref
from conftest import mps_path
from test_gpu_ipm import parse, progress, rel
from test_qp_solver import (NETLIB_SEEDS, QP_L, QP_OBJ, QP_Q, QP_C, SMALL_SEEDS, netlib_problem, small_problem,
                            write_qp_mps)

pytestmark = pytest.mark.gpu

CERT = 2e-6


def check_certificate(p, x, y, w, z):
    pr, du, gap, lo = qp_ref.certificate(p, x, y, w, z)
    print(f"certificate: primal {pr:.3e} dual {du:.3e} gap {gap:.3e} min {lo:.3e}")
    assert pr <= CERT and du <= CERT and gap <= CERT and lo > 0, (pr, du, gap, lo)


def check_against(ref, out):
    rows, _ = parse(out["trace"])
    rrows = ref["rows"]
    print(f"status {out['status']} lines {len(rows)} (reference {ref['status']}, {len(rrows)}); last {rows[-1:]} "
          f"reference {rrows[-1]}")
    worst = 0.0
    for r, g in zip(rows, rrows):
        tol = max(1e-5, 0.1 * progress(g + (None,)))
        worst = max(worst, rel(r[1], g[1]) / tol, rel(r[3], g[3]) / tol)
    print(f"worst line distance / its tolerance: {worst:.3e}; final {rel(rows[-1][1], rrows[-1][1]):.3e} "
          f"{rel(rows[-1][3], rrows[-1][3]):.3e}")
    assert out["status"] == 0 and ref["status"] == 0
    assert abs(len(rows) - len(rrows)) <= 1
    for r, g in zip(rows, rrows):
        tol = max(1e-5, 0.1 * progress(g + (None,)))
        assert r[0] == g[0]
        assert rel(r[1], g[1]) <= tol and rel(r[3], g[3]) <= tol, (r, g)
    assert rel(rows[-1][1], rrows[-1][1]) <= 1e-6 and rel(rows[-1][3], rrows[-1][3]) <= 1e-6


@pytest.mark.parametrize("m,n,kind", sorted(SMALL_SEEDS))
def test_small_shapes_match_reference(m, n, kind):
    """63 x 65: one partly filled wave on either side of 64; banded / lowrank:
    off-diagonal Q (a non-bipartite KKT graph), lowrank singular and dense;
    gaps: empty columns of Q."""
    p, ref = qp_ref.reference((m, n, kind), small_problem, "dense")
    out = ipo_amd.solver(p, method="qp", trace=True)
    check_against(ref, out)
    check_certificate(p, out["x"], out["y"], out["w"], out["z"])


def test_budget_projection():
    """max a'x - x'x / 2, sum x <= 1: x = e_4, y = 2, objective 2.5, status 0.
    One row: the reference trips intpt's growth test on a residual that is
    a single rounding error, at a line that depends on the host's rounding
    (tests/test_qp_solver.py), so the lines are held to the reference
    iteration without its give-up tests, which runs to the stop rule."""
    p = qp_ref.budget_projection()
    ref = qp_ref.solve_qp(p, "dense", giveup=False)
    out = ipo_amd.solver(p, method="qp", trace=True)
    check_against(ref, out)
    rows, _ = parse(out["trace"])
    assert np.allclose(out["x"], [0, 0, 0, 1, 0], atol=1e-6) and abs(out["y"][0] - 2.0) <= 1e-6
    assert abs(rows[-1][1] - 2.5) <= 2.5e-6 and abs(rows[-1][3] - 2.5) <= 2.5e-6
    check_certificate(p, out["x"], out["y"], out["w"], out["z"])


_STAB = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "rounding_stability.json")))["intpt"]


@pytest.mark.parametrize("name", ["afiro", "sc50a", "sc50b", "sc105", "kb2", "sctap1"])
def test_empty_q_is_the_lp(name):
    """Method qp without Q on problems rounding_stability.json marks stable
    for intpt: the table's status, line count +-1 and final objectives to
    1e-6.  An empty Q is the LP and takes intpt's iteration on the LP's own
    factor, not the swapped one a Q needs: that table speaks of the LP's
    factor only -- with A' for A the
    reference's own restatement (qp_ref, oracle back end) ends sctap1 "dual
    infeasible" after 50 lines in all six of its rounding variants, on the
    growth test of intpt.c:175-182."""
    v = _STAB[name]
    assert v["stable"]
    status, text, st = ipo_amd.run_mps(mps_path(name), "qp")
    rows, stat = parse(text)
    print(stat, len(rows), rows[-1], v["oracle_iters"], v["oracle_last"])
    assert stat == v["oracle_status"] and status == 0
    assert abs(len(rows) - v["oracle_iters"]) <= 1
    assert rel(rows[-1][1], v["oracle_last"][1]) <= 1e-6 and rel(rows[-1][3], v["oracle_last"][2]) <= 1e-6


@pytest.mark.parametrize("name", sorted(NETLIB_SEEDS))
def test_netlib_patterns_with_q(name):
    p, ref = qp_ref.reference((name,), netlib_problem, "oracle")
    out = ipo_amd.solver(p, method="qp", trace=True)
    check_against(ref, out)
    check_certificate(p, out["x"], out["y"], out["w"], out["z"])


def test_grid_stride_certificate():
    """m + n = 270,000 > kRedBlocks kResThreads = 262,144: the residual
    kernel's loop takes a second pass; nested dissection with Q; below the
    2^19 segmented-dot threshold.  Certificate only."""
    p = ipo_amd.synth_random(m=60_000, n=210_000, per_col=4, band=256)
    d = np.random.default_rng(7).uniform(0.1, 2.0, p.n)
    q = (np.arange(p.n + 1, dtype=np.int32), np.arange(p.n, dtype=np.int32), d)
    qp = ipo_amd.SolverForm(p.m, p.n, p.kA, p.iA, p.A, p.b, p.c + d * p.xs, 0.0, q=q)
    out = ipo_amd.solver(qp, method="qp")
    print(out["status"], out["stats"]["iters"], out["stats"]["t_setup_s"], out["stats"]["t_solve_s"])
    assert out["status"] == 0
    check_certificate(qp, out["x"], out["y"], out["w"], out["z"])


@pytest.mark.parametrize("sense", ["MIN", "MAX"])
def test_through_the_mps_path(tmp_path, sense):
    """run_mps(path, "qp") on the CPU test's files: status 0, and the printed
    final objective is the file's objective c'x + x'Qx / 2 + f at the
    original-variable x of the .out report -- times -sense (sense 1 MIN, -1
    MAX), the sign every method here prints: solver form maximises, so a MIN
    file prints the negated objective (afiro: 464.75 for -464.75)."""
    path = write_qp_mps(tmp_path, sense)
    sol = os.path.join(str(tmp_path), "qp.out")
    status, text, st = ipo_amd.run_mps(path, method="qp", solfile=sol)
    rows, stat = parse(text)
    assert status == 0 and stat == "optimal solution"
    x = []
    with open(sol) as fh:
        lines = fh.read().splitlines()
    for ln in lines[2:lines.index("ROWS SECTION")]:
        x.append(float(ln.split()[2]))
    x = np.array(x)
    s = 1.0 if sense == "MIN" else -1.0
    obj = (s * QP_C) @ x + 0.5 * x @ ((s * QP_Q) @ x)            # the file's c and Q
    print(x, obj, rows[-1])
    assert abs(rows[-1][1] - (-s * obj)) <= 1e-6 * abs(obj)
    assert abs(obj - s * QP_OBJ) <= 1e-6 * QP_OBJ and np.all(x >= QP_L - 1e-6)


def test_refusals(tmp_path):
    """None of these starts a solve (no iteration in the statistics)."""
    p, _ = qp_ref.reference((20, 30, "diag"), small_problem, "dense")
    ctx = ipo_amd.Context(p)
    try:
        for method in ("hsd", "intpt", "hsdls"):
            st, stats, _ = ctx.run(method)
            assert st == 7 and stats["iters"] == 0 and "qp" in ipo_amd.last_error()
        with pytest.raises(ipo_amd.IpoHipError, match="qp"):
            ipo_amd.solver(p, method="intpt")
    finally:
        ctx.close()
    from test_gpu_shard import DIMS
    loc = ipo_amd.shard_block_angular(ipo_amd.synth_block_angular(*DIMS), 1, 0)
    sh = ipo_amd.ShardContext(loc)
    try:
        st, stats, _ = sh.run("qp")
        assert st == 7 and stats["iters"] == 0 and "shard" in ipo_amd.last_error()
    finally:
        sh.close()
    status, text, stats = ipo_amd.run_mps(write_qp_mps(tmp_path, "MIN"), method="qp", free="split")
    assert status == 7 and stats["iters"] == 0 and "split" in ipo_amd.last_error().lower()
    assert "Iter" not in text


def test_two_runs_on_one_context_identical():
    p, _ = qp_ref.reference((63, 65, "banded"), small_problem, "dense")
    ctx = ipo_amd.Context(p)
    try:
        st1, s1, _ = ctx.run("qp")
        a = ctx.solution()
        st2, s2, _ = ctx.run("qp")
        b = ctx.solution()
    finally:
        ctx.close()
    assert st1 == st2 == 0 and s1["iters"] == s2["iters"]
    for u, v in zip(a, b):
        assert np.array_equal(u, v)


def test_qp_on_a_plain_context_is_the_empty_q():
    """Method 3 on a context without Q is the QP with an empty Q, on the
    context's LP factor; the LP methods on the same context are untouched."""
    p = ipo_amd.load_mps(mps_path("afiro"))
    ctx = ipo_amd.Context(p)
    try:
        st0, s0, t0 = ctx.run("intpt", trace=True)
        st1, s1, t1 = ctx.run("qp", trace=True)
        st2, s2, t2 = ctx.run("intpt", trace=True)
    finally:
        ctx.close()
    assert st0 == st1 == st2 == 0 and t0 == t2
    r0, r1 = parse(t0)[0], parse(t1)[0]
    assert abs(len(r0) - len(r1)) <= 1 and rel(r1[-1][1], r0[-1][1]) <= 1e-6
