"""The start rule "mehrotra" on the GPU (Context.set_start_rule,
Context.start_point, IPO_HIP_START), against its
yardstick tests/pc_mehrotra_ref.py.

The cases are pc_mehrotra_ref.CASES (tests/test_start_rule.py checks on the
host that the reference start is positive on each and that the restated pc
iteration ends optimal from it).  The bars: the start itself to 1e-8 max
|vector|, test_gpu_qp's bar for a refined solution; a run under the rule to
test_gpu_pc.solve_and_check's status, line count, final objectives and
certificate; everything that compares two device runs, bit for bit.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import ipo_amd
import pc_mehrotra_ref as mr
import pc_start_ref as ps
from conftest import PKG, REPO, mps_path
from qp_ref import _mats
from test_gpu_ipm import parse, rel
from test_gpu_pc import _SOLVER_CHILD
from test_gpu_qp_solver import check_certificate
from test_gpu_resolve import lines, printed, run_all, same, values

pytestmark = pytest.mark.gpu

LP_CASE, QP_CASE = "lp 63x65", "banded 63x65"


def methods_of(name):
    return ("pc", "intpt", "qp") if name == LP_CASE else ("pc", "qp")


def device_start(p, rule="mehrotra"):
    ctx = ipo_amd.Context(p)
    try:
        return ctx.start_point(rule)
    finally:
        ctx.close()


def rule_runs(p, methods, **kw):
    """run_all of a fresh context under the rule."""
    ctx = ipo_amd.Context(p)
    try:
        ctx.set_start_rule("mehrotra")
        return run_all(ctx, methods, **kw)
    finally:
        ctx.close()


def line_close(got, want):
    """test_gpu_resolve.test_clamping's bar: a printed line against the line
    of an iterate recomputed in NumPy, to the printed digits (one unit of
    float32 in an objective, one unit of the last digit in a norm)."""
    for k, digits in ((1, 7), (2, 1), (3, 7), (4, 1)):
        ref = printed(want[k], digits)
        unit = 10.0 ** (np.floor(np.log10(abs(ref))) - digits) if ref != 0 else 0.0
        tol = 1.2e-7 * abs(ref) if digits == 7 else 1.0001 * unit
        assert abs(got[k] - ref) <= tol, (k, got[k], ref)


# ---------------------------------------------------------------- 1: the point
@pytest.mark.parametrize("name", sorted(mr.CASES))
def test_start_point_against_the_reference(name):
    p, want, _ = mr.reference(name)
    got = device_start(p)
    for nm, g, r in zip("xywz", got, want):
        err, scale = np.abs(g - r).max(), np.abs(r).max()
        print(f"{name} {nm}: max |device - reference| {err:.3e}, max |reference| {scale:.3e}")
    for g, r in zip(got, want):
        assert np.all(np.isfinite(g)) and np.all(g > 0)
        assert np.abs(g - r).max() <= 1e-8 * np.abs(r).max()


def test_zero_problem_gives_exactly_one():
    """b = 0 and c = 0: both solutions are zero, no shift, g = 0, so eps = 1."""
    p, _ = mr.problem(mr.ZERO)
    for v in device_start(p):
        assert np.array_equal(v, np.ones(v.size))
    for v in device_start(p, "default"):
        assert np.array_equal(v, np.full(v.size, 1000.0))


# ---------------------------------------------------------------- 2: rule = explicit point
@pytest.mark.parametrize("name", [LP_CASE, QP_CASE])
def test_the_rule_and_the_explicit_point_are_one(name):
    """set_start_rule("mehrotra") then run(m) prints what set_start(*start_point())
    then run(m) prints and leaves the same solution bits; a second run under
    the rule is the first."""
    p, _, _ = mr.reference(name)
    meths = methods_of(name)
    ctx = ipo_amd.Context(p)
    try:
        default = run_all(ctx, meths)
        ctx.set_start_rule("mehrotra")
        first = run_all(ctx, meths)
        second = run_all(ctx, meths)
        point = ctx.start_point("mehrotra")
        third = run_all(ctx, meths)                 # start_point changed nothing for the next run
        ctx.set_start(*point)
        explicit = run_all(ctx, meths)
    finally:
        ctx.close()
    for meth in meths:
        print(name, meth, first[meth][0], len(lines(first[meth][1])), len(lines(default[meth][1])))
        same(second[meth], first[meth])
        same(third[meth], first[meth])
        same(explicit[meth], first[meth])
        assert first[meth][1] != default[meth][1]


# ---------------------------------------------------------------- 3: line 0
@pytest.mark.parametrize("name", [LP_CASE, QP_CASE, "afiro"])
def test_line_0_under_the_rule(name):
    p, _, _ = mr.reference(name)
    ctx = ipo_amd.Context(p)
    try:
        start = ctx.start_point("mehrotra")
        ctx.set_start_rule("mehrotra")
        st, stats, text = ctx.run("pc", max_iter=1, trace=True)
    finally:
        ctx.close()
    want, _ = ps.line_of(p, *start)
    got = lines(text)
    print(got, want)
    assert st == 5 and len(got) == 1 and got[0][0] == 0
    line_close(got[0], want)


# ---------------------------------------------------------------- 4: the solve
@pytest.mark.parametrize("name", sorted(mr.CASES))
def test_pc_under_the_rule(name):
    """test_gpu_pc.solve_and_check's bars against the reference run from the
    reference start: status 0, the line count within 1, the final objectives
    to 1e-6, the fp64 certificate at most 2e-6 (check_certificate).  The
    start costs one factorisation and two solves."""
    p, _, ref = mr.reference(name)
    ctx = ipo_amd.Context(p)
    try:
        ctx.set_start_rule("mehrotra")
        st, stats, text = ctx.run("pc", trace=True)
        x, y, w, z = ctx.solution()
    finally:
        ctx.close()
    rows, rrows = lines(text), ref["rows"]
    print(f"{name}: status {st}, {len(rows)} lines (reference {ref['status']}, {len(rrows)}); last {rows[-1]} "
          f"reference {rrows[-1]}; factors {stats['factors']} solves {stats['solves']}")
    assert st == 0 and ref["status"] == 0
    assert abs(len(rows) - len(rrows)) <= 1
    assert rel(rows[-1][1], rrows[-1][1]) <= 1e-6 and rel(rows[-1][3], rrows[-1][3]) <= 1e-6
    check_certificate(p, x, y, w, z)
    systems = len(rows) - 1                        # the last line stops before its Newton system
    assert stats["factors"] == systems + 1 and stats["solves"] == 2 * systems + 2


# ---------------------------------------------------------------- 5: grid stride
def test_grid_stride():
    """m + n = 70,000 > kRedBlocks x 256 = 65,536 (test_gpu_pc's
    test_grid_stride_certificate's problem): the start's kernels take a second
    pass.  Every entry positive and finite; and with sp = delta_p + eps_p and
    sd = delta_d + eps_d the point is (x~ + sp, y~ + sd, w~ + sp, z~ + sd), so
        A x + w - b           = sp (A 1 + 1)
        A'y - (I + Q) z - c   = sd (A'1 - (I + Q) 1):
    each left side, recomputed in NumPy, is a multiple of its vector (the
    shift recovered by least squares) up to 1e-8 (max |right-hand side| + 1).
    The refined solves stop at a residual of 1e-10 (max |right-hand side| + 1)
    or when it no longer halves; the factor 100 is for the second reason."""
    p = ipo_amd.synth_random(m=20_000, n=50_000, per_col=4, band=256)
    d = np.random.default_rng(7).uniform(0.1, 2.0, p.n)
    q = (np.arange(p.n + 1, dtype=np.int32), np.arange(p.n, dtype=np.int32), d)
    qp = ipo_amd.SolverForm(p.m, p.n, p.kA, p.iA, p.A, p.b, p.c + d * p.xs, 0.0, q=q)
    x, y, w, z = device_start(qp)
    for v in (x, y, w, z):
        assert np.all(np.isfinite(v)) and np.all(v > 0)
    A, Q = _mats(qp)
    for nm, r, v, rhs in (("primal", A @ x + w - qp.b, A @ np.ones(p.n) + 1.0, qp.b),
                          ("dual", A.T @ y - z - Q @ z - qp.c, A.T @ np.ones(p.m) - 1.0 - Q @ np.ones(p.n), qp.c)):
        s = (r @ v) / (v @ v)
        left = np.abs(r - s * v).max()
        print(f"{nm}: shift {s:.6e}, what is left {left:.3e}, max |rhs| {np.abs(rhs).max():.3e}")
        assert s > 0 and left <= 1e-8 * (np.abs(rhs).max() + 1.0)


# ---------------------------------------------------------------- 6: after update
@pytest.mark.parametrize("name", [LP_CASE, QP_CASE])
def test_the_rule_after_update(name):
    """The rule is applied from the numbers then current: after update() to
    member 2 the run is a fresh context's under the rule on member 2."""
    p1, _, seed = ps.case(name)
    p2 = ps.second_member(p1, seed)
    want1, want2 = rule_runs(p1, ("pc",))["pc"], rule_runs(p2, ("pc",))["pc"]
    ctx = ipo_amd.Context(p1)
    try:
        ctx.set_start_rule("mehrotra")
        first = run_all(ctx, ("pc",))["pc"]
        ctx.update(**values(p2))
        second = run_all(ctx, ("pc",))["pc"]
    finally:
        ctx.close()
    same(first, want1)
    same(second, want2)
    assert want1[0] == want2[0] == 0 and want1[1] != want2[1]


# ---------------------------------------------------------------- 7: precedence and refusals
def test_precedence():
    p, _, _ = mr.reference(LP_CASE)
    rng = np.random.default_rng(5)
    point = [rng.uniform(0.5, 2.0, k) for k in (p.n, p.m, p.m, p.n)]
    ctx = ipo_amd.Context(p)
    try:
        default = run_all(ctx, ("pc",))["pc"]
        ctx.set_start(*point)
        held = run_all(ctx, ("pc",))["pc"]
        ctx.set_start_rule("mehrotra")
        rule = run_all(ctx, ("pc",))["pc"]                    # the rule cleared the held point
        ctx.set_start(*point)
        same(run_all(ctx, ("pc",))["pc"], held)               # rule, then a point: the point wins
        ctx.start_from_last(1.0)
        ctx.set_start_rule("mehrotra")
        same(run_all(ctx, ("pc",))["pc"], rule)               # start_from_last, then the rule: the rule wins
        ctx.clear_start()
        same(run_all(ctx, ("pc",))["pc"], default)            # the clear call: the default start
        ctx.set_start_rule("mehrotra")
        ctx.start_from_last(1.0)
        assert run_all(ctx, ("pc",))["pc"][1] != rule[1]      # the rule, then start_from_last: the iterate wins
        ctx.set_start_rule("default")
        same(run_all(ctx, ("pc",))["pc"], default)            # a rule, default too, clears the held point
    finally:
        ctx.close()
    assert len({default[1], held[1], rule[1]}) == 3


def test_refusals():
    from test_gpu_shard import DIMS
    p, _, _ = mr.reference(LP_CASE)
    ctx = ipo_amd.Context(p)
    try:
        ctx.set_start_rule("mehrotra")
        for meth in ("hsd", "hsdls"):
            st, stats, text = ctx.run(meth, trace=True)
            assert st == 7 and stats["iters"] == 0 and "start" in ipo_amd.last_error() and "Iter" not in text
        ctx.set_start_rule("default")
        assert ctx.run("hsd")[0] != 7 and ctx.run("hsdls")[0] != 7
        assert ipo_amd.lib().ipo_hip_ctx_set_start_rule(ctx.h, 2) == -1 and "rule" in ipo_amd.last_error()
        assert ipo_amd.lib().ipo_hip_ctx_start_point(ctx.h, -1, None, None, None, None) == -1
        with pytest.raises(ipo_amd.IpoHipError, match="rule"):
            ctx.set_start_rule("bogus")
        assert ctx.run("hsd")[0] != 7                         # the refused calls changed nothing
    finally:
        ctx.close()
    loc = ipo_amd.shard_block_angular(ipo_amd.synth_block_angular(*DIMS), 1, 0)
    sh = ipo_amd.ShardContext(loc)
    try:
        for rule in ("mehrotra", "default"):
            with pytest.raises(ipo_amd.IpoHipError, match="shard"):
                sh.set_start_rule(rule)
        with pytest.raises(ipo_amd.IpoHipError, match="shard"):
            sh.start_point("mehrotra")
    finally:
        sh.close()


# ---------------------------------------------------------------- 8: the environment
def test_the_solver_symbol_by_environment():
    """IPO_HIP_METHOD=pc IPO_HIP_START=mehrotra behind the literal solver()
    symbol, in a fresh process (test_gpu_pc's child): the lines of a context's
    run under the rule, line 0 included."""
    p, _, _ = mr.reference("afiro")
    want = rule_runs(p, ("pc",))["pc"]
    env = dict(os.environ, IPO_HIP_METHOD="pc", IPO_HIP_START="mehrotra",
               PYTHONPATH=os.pathsep.join([PKG, os.path.join(REPO, "tests")]))
    r = subprocess.run([sys.executable, "-c", _SOLVER_CHILD, mps_path("afiro")], env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "status 0" in r.stdout.splitlines()[-1]
    rows = parse(r.stdout)[0]
    print(rows[0], lines(want[1])[0])
    assert want[0] == 0 and rows == lines(want[1])
    line_close(rows[0], ps.line_of(p, *device_start(p))[0])


def test_the_environment_in_the_one_shot_entries(monkeypatch):
    """Read when the entry is called: an unknown value is 7 with a text, so is
    mehrotra with hsd and hsdls; contexts ignore the variable; run_mps under
    it ends on the objectives of the run without it."""
    p, _, _ = mr.reference(LP_CASE)
    monkeypatch.delenv("IPO_HIP_START", raising=False)
    plain = ipo_amd.solver(p, method="pc", trace=True)
    st0, text0, _ = ipo_amd.run_mps(mps_path("afiro"), "pc")
    monkeypatch.setenv("IPO_HIP_START", "bogus")
    out = ipo_amd.solver(p, method="pc", trace=True)
    assert out["status"] == 7 and out["stats"]["iters"] == 0 and "IPO_HIP_START" in ipo_amd.last_error()
    assert ipo_amd.run_mps(mps_path("afiro"), "pc")[0] == 7
    monkeypatch.setenv("IPO_HIP_START", "mehrotra")
    for meth in ("hsd", "hsdls"):
        out = ipo_amd.solver(p, method=meth, trace=True)
        assert out["status"] == 7 and out["stats"]["iters"] == 0 and "start" in ipo_amd.last_error()
        assert "Iter" not in out["trace"]
    under = ipo_amd.solver(p, method="pc", trace=True)
    want = rule_runs(p, ("pc",))["pc"]
    assert under["status"] == 0 and lines(under["trace"]) == lines(want[1]) and under["trace"] != plain["trace"]
    ctx = ipo_amd.Context(p)
    try:
        st, _, text = ctx.run("pc", trace=True)               # a context uses the call, not the variable
    finally:
        ctx.close()
    assert st == 0 and lines(text) == lines(plain["trace"])
    st1, text1, _ = ipo_amd.run_mps(mps_path("afiro"), "pc")
    a, b = parse(text0)[0], parse(text1)[0]
    print(len(a), len(b), a[-1], b[-1])
    assert st0 == st1 == 0 and a[0] != b[0]
    assert rel(b[-1][1], a[-1][1]) <= 1e-6 and rel(b[-1][3], a[-1][3]) <= 1e-6
    monkeypatch.setenv("IPO_HIP_START", "default")
    assert ipo_amd.solver(p, method="pc", trace=True)["trace"] == plain["trace"]


# ---------------------------------------------------------------- 9: nothing leaks
@pytest.mark.parametrize("meth", ["intpt", "pc"])
def test_default_traces_unchanged_by_a_rule_run_between(meth):
    """test_gpu_pc.test_intpt_unchanged_by_a_pc_run_between's shape."""
    ctx = ipo_amd.Context(mr.reference("afiro")[0])
    try:
        st0, _, t0 = ctx.run(meth, trace=True)
        a = ctx.solution()
        ctx.set_start_rule("mehrotra")
        st1, _, t1 = ctx.run("pc", trace=True)
        ctx.start_point("mehrotra")
        ctx.set_start_rule("default")
        st2, _, t2 = ctx.run(meth, trace=True)
        b = ctx.solution()
    finally:
        ctx.close()
    assert st0 == st1 == st2 == 0 and t0 == t2 and t1 != t0
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes()
