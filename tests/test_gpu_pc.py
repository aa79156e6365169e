"""The predictor-corrector solver (method "pc") on the GPU, against its
yardstick tests/pc_ref.py (an extension: not in the reference).

The cases and why they were chosen (the reference ends optimal on each under
its own rounding variants) are tests/test_pc.py's.  The bars are
tests/test_gpu_qp_solver.py's: status 0, the printed line count within +-1
of the reference run's, every line's objectives to max(1e-5, 0.1 x the
line's progress), the final objectives to 1e-6, and the fp64 certificate of
the downloaded x, y, w, z at most 2e-6 with every entry positive.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import ipo_amd
import pc_ref
import qp_dense
from conftest import PKG, REPO, mps_path
from test_gpu_ipm import parse, rel
from test_gpu_qp_solver import check_against, check_certificate
from test_pc import (DENSE_CASES, FREE_LP, LP_SHAPES, NETLIB_LPS, SMALL_CASES, free_lp, lp_shape, netlib_distance,
                     netlib_lp, small_case)
from test_qp_solver import NETLIB_SEEDS, QP_C, QP_L, QP_OBJ, QP_Q, netlib_problem, write_qp_mps

pytestmark = pytest.mark.gpu


def solve_and_check(p, ref):
    out = ipo_amd.solver(p, method="pc", trace=True)
    check_against(ref, out)
    check_certificate(p, out["x"], out["y"], out["w"], out["z"])
    return out


@pytest.mark.parametrize("m,n,kind,seed", SMALL_CASES)
def test_small_shapes_match_reference(m, n, kind, seed):
    """63 x 65: a partly filled wave on either side of 64; 1 x 64: a one-row
    residual; lowrank: a singular dense Q; gaps: empty columns of Q.  The
    swapped factor."""
    p, ref = pc_ref.reference((m, n, kind, seed), small_case, "dense")
    solve_and_check(p, ref)


@pytest.mark.parametrize("m,n,seed", LP_SHAPES)
def test_empty_q_is_the_lp(m, n, seed):
    """The same shapes without q: the LP orientation of every new kernel."""
    p, ref = pc_ref.reference((m, n, seed), lp_shape, "dense")
    solve_and_check(p, ref)


@pytest.mark.parametrize("name", NETLIB_LPS)
def test_netlib_lps(name):
    """run_mps(path, "pc") against the oracle-backed reference run, and its
    final objectives against the netlib optimum: within twice the distance
    at which the reference run itself ends from it (test_pc.py prints it),
    floor 1e-6."""
    p, ref = pc_ref.reference((name,), netlib_lp, "oracle")
    status, text, st = ipo_amd.run_mps(mps_path(name), "pc")
    rows, stat = parse(text)
    assert stat == "optimal solution"
    check_against(ref, {"status": status, "trace": text})
    dist, target = netlib_distance(name, ref)
    bar = max(1e-6, 2 * dist)
    print(f"netlib optimum {target!r}: reference {dist:.3e}, device {rel(rows[-1][1], target):.3e} "
          f"{rel(rows[-1][3], target):.3e}, bar {bar:.3e}")
    assert rel(rows[-1][1], target) <= bar and rel(rows[-1][3], target) <= bar
    out = ipo_amd.solver(p, method="pc")
    assert out["status"] == 0
    check_certificate(p, out["x"], out["y"], out["w"], out["z"])


@pytest.mark.parametrize("name", sorted(NETLIB_SEEDS))
def test_netlib_patterns_with_q(name):
    p, ref = pc_ref.reference((name,), netlib_problem, "oracle")
    solve_and_check(p, ref)


@pytest.mark.parametrize("knob", [None, "0"])
@pytest.mark.parametrize("m,n,kind", DENSE_CASES)
def test_long_columns(monkeypatch, m, n, kind, knob):
    """Q's long columns summed by one wave each before the residual kernel,
    and (IPO_HIP_Q_LONG=0) by one thread: certificate and line count."""
    if knob is None:
        monkeypatch.delenv("IPO_HIP_Q_LONG", raising=False)
    else:
        monkeypatch.setenv("IPO_HIP_Q_LONG", knob)
    p, ref = pc_ref.reference((m, n, kind), qp_dense.dense_problem, "dense")
    ctx = ipo_amd.Context(p)
    try:
        assert ctx.q_long() == (0 if knob == "0" else n if kind == "factor" else 3)
        st, _, text = ctx.run("pc", trace=True)
        x, y, w, z = ctx.solution()
    finally:
        ctx.close()
    lines = len(parse(text)[0])
    print(st, lines, ref["iters"])
    assert st == 0 and ref["status"] == 0 and abs(lines - ref["iters"]) <= 1
    check_certificate(p, x, y, w, z)


def test_grid_stride_certificate():
    """m + n = 70,000 > kRedBlocks x 256 = 65,536: the direction kernels'
    loops take a second pass.  Certificate only."""
    p = ipo_amd.synth_random(m=20_000, n=50_000, per_col=4, band=256)
    d = np.random.default_rng(7).uniform(0.1, 2.0, p.n)
    q = (np.arange(p.n + 1, dtype=np.int32), np.arange(p.n, dtype=np.int32), d)
    qp = ipo_amd.SolverForm(p.m, p.n, p.kA, p.iA, p.A, p.b, p.c + d * p.xs, 0.0, q=q)
    out = ipo_amd.solver(qp, method="pc")
    print(out["status"], out["stats"]["iters"], out["stats"]["t_setup_s"], out["stats"]["t_solve_s"])
    assert out["status"] == 0
    check_certificate(qp, out["x"], out["y"], out["w"], out["z"])


# ---------------------------------------------------------------- work per iteration
@pytest.mark.parametrize("with_q", [True, False])
def test_one_factor_two_solves_an_iteration(with_q):
    p = small_case(63, 65, "banded", 12) if with_q else lp_shape(63, 65, 0)
    out = ipo_amd.solver(p, method="pc", trace=True)
    s, lines = out["stats"], len(parse(out["trace"])[0])
    print(lines, s["factors"], s["solves"])
    assert out["status"] == 0
    assert s["factors"] == lines - 1               # the last line stops before its Newton system
    assert s["solves"] == 2 * s["factors"]


@pytest.mark.parametrize("with_q", [True, False])
def test_two_runs_on_one_context_identical(with_q):
    p = small_case(63, 65, "banded", 12) if with_q else lp_shape(63, 65, 0)
    ctx = ipo_amd.Context(p)
    try:
        st1, s1, t1 = ctx.run("pc", trace=True)
        a = ctx.solution()
        st2, s2, t2 = ctx.run("pc", trace=True)
        b = ctx.solution()
    finally:
        ctx.close()
    assert st1 == st2 == 0 and s1["iters"] == s2["iters"] and t1 == t2
    for u, v in zip(a, b):
        assert np.array_equal(u, v)


def test_intpt_unchanged_by_a_pc_run_between():
    ctx = ipo_amd.Context(netlib_lp("afiro"))
    try:
        st0, _, t0 = ctx.run("intpt", trace=True)
        a = ctx.solution()
        st1, _, t1 = ctx.run("pc", trace=True)
        st2, _, t2 = ctx.run("intpt", trace=True)
        b = ctx.solution()
    finally:
        ctx.close()
    assert st0 == st1 == st2 == 0 and t0 == t2 and t1 != t0
    for u, v in zip(a, b):
        assert np.array_equal(u, v)


def test_qp_unchanged_by_a_pc_run_between():
    ctx = ipo_amd.Context(small_case(63, 65, "banded", 12))
    try:
        st0, _, t0 = ctx.run("qp", trace=True)
        a = ctx.solution()
        st1, _, t1 = ctx.run("pc", trace=True)
        st2, _, t2 = ctx.run("qp", trace=True)
        b = ctx.solution()
    finally:
        ctx.close()
    assert st0 == st1 == st2 == 0 and t0 == t2 and t1 != t0
    for u, v in zip(a, b):
        assert np.array_equal(u, v)


# ---------------------------------------------------------------- refusals and front ends
def test_refusals(tmp_path):
    """Neither starts a solve (no iteration in the statistics)."""
    from test_gpu_shard import DIMS
    loc = ipo_amd.shard_block_angular(ipo_amd.synth_block_angular(*DIMS), 1, 0)
    sh = ipo_amd.ShardContext(loc)
    try:
        st, stats, _ = sh.run("pc")
        assert st == 7 and stats["iters"] == 0 and "shard" in ipo_amd.last_error()
    finally:
        sh.close()
    status, text, stats = ipo_amd.run_mps(write_qp_mps(tmp_path, "MIN"), method="pc", free="split")
    assert status == 7 and stats["iters"] == 0 and "split" in ipo_amd.last_error().lower()
    assert "Iter" not in text
    # the LP methods on a problem with q are still refused, and say which methods it takes
    p = small_case(20, 30, "diag", 5)
    with pytest.raises(ipo_amd.IpoHipError, match="qp"):
        ipo_amd.solver(p, method="intpt")
    ctx = ipo_amd.Context(p)
    try:
        st, stats, _ = ctx.run("hsd")
        assert st == 7 and stats["iters"] == 0 and "qp" in ipo_amd.last_error()
    finally:
        ctx.close()


def test_split_free_columns_without_quads():
    """free="split" on an LP with free columns: pc takes the LP transform and
    ends optimal, on the reference run's line count and final objectives.
    (Not held line by line: the worst line stood 4.1 times its tolerance
    from the oracle-backed run, 4.7 % against 3.7 % of the dual objective.)"""
    p, ref = pc_ref.reference((FREE_LP,), free_lp, "oracle")
    status, text, st = ipo_amd.run_mps(mps_path(FREE_LP), "pc", free="split")
    rows, stat = parse(text)
    rrows = ref["rows"]
    print(status, len(rows), len(rrows), rows[-1], rrows[-1])
    assert status == 0 and stat == "optimal solution" and ref["status"] == 0
    assert f"m = {p.m},n = {p.n},nz = {p.nz}\n" in text              # the split problem's dimensions
    assert abs(len(rows) - len(rrows)) <= 1
    assert rel(rows[-1][1], rrows[-1][1]) <= 1e-6 and rel(rows[-1][3], rrows[-1][3]) <= 1e-6


@pytest.mark.parametrize("sense", ["MIN", "MAX"])
def test_through_the_mps_path(tmp_path, sense):
    """test_gpu_qp_solver.test_through_the_mps_path's files and objective check, by pc."""
    path = write_qp_mps(tmp_path, sense)
    sol = os.path.join(str(tmp_path), "qp.out")
    status, text, st = ipo_amd.run_mps(path, method="pc", solfile=sol)
    rows, stat = parse(text)
    assert status == 0 and stat == "optimal solution"
    with open(sol) as fh:
        lines = fh.read().splitlines()
    x = np.array([float(ln.split()[2]) for ln in lines[2:lines.index("ROWS SECTION")]])
    s = 1.0 if sense == "MIN" else -1.0
    obj = (s * QP_C) @ x + 0.5 * x @ ((s * QP_Q) @ x)            # the file's c and Q
    print(x, obj, rows[-1])
    assert abs(rows[-1][1] - (-s * obj)) <= 1e-6 * abs(obj)
    assert abs(obj - s * QP_OBJ) <= 1e-6 * QP_OBJ and np.all(x >= QP_L - 1e-6)


_SOLVER_CHILD = """
import ctypes as C, sys
import numpy as np
import ipo_amd
p = ipo_amd.load_mps(sys.argv[1])
m, n = p.m, p.n
x, y, w, z = np.zeros(n + m), np.zeros(n + m), np.zeros(m), np.zeros(n)
kA, iA = np.ascontiguousarray(p.kA, np.int32), np.ascontiguousarray(p.iA, np.int32)
st = ipo_amd.lib().solver(m, n, p.nz, iA.ctypes.data, kA.ctypes.data, p.A.ctypes.data, p.b.ctypes.data,
                          p.c.ctypes.data, float(p.f), x.ctypes.data, y.ctypes.data, w.ctypes.data, z.ctypes.data)
C.CDLL(None).fflush(None)
print("status", st, flush=True)
"""


def test_the_solver_symbol_by_environment():
    """IPO_HIP_METHOD=pc selects the method behind the literal solver()
    symbol (read when it is called; a fresh process, as a caller linking the
    library would be): intpt's banner, pc's lines."""
    p, ref = pc_ref.reference(("afiro",), netlib_lp, "oracle")
    env = dict(os.environ, IPO_HIP_METHOD="pc", PYTHONPATH=os.pathsep.join([PKG, os.path.join(REPO, "tests")]))
    r = subprocess.run([sys.executable, "-c", _SOLVER_CHILD, mps_path("afiro")], env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "status 0" in r.stdout.splitlines()[-1]
    assert "  Iter   |  Obj Value       Infeas   |  Obj Value       Infeas   |\n" in r.stdout      # intpt's banner: no mu column
    rows, _ = parse(r.stdout)
    assert abs(len(rows) - ref["iters"]) <= 1
    assert rel(rows[-1][1], ref["rows"][-1][1]) <= 1e-6 and rel(rows[-1][3], ref["rows"][-1][3]) <= 1e-6
