"""Re-solving on one context (Context.update, set_start, start_from_last) on
the GPU: new numbers on the creation's pattern give bit for bit what a fresh
context on them gives, refusals leave the context as it was, and a start
point replaces "every variable 1000" and nothing else.

The cases, the second member of each family, the restated iteration with a
start argument and the warm start's floor are tests/pc_start_ref.py's;
tests/test_resolve_ref.py checks on the host that the references end optimal
on every second member and from the warm start.
"""
import numpy as np
import pytest

import ipo_amd
import pc_start_ref as ps
from test_gpu_ipm import parse
from test_gpu_qp_solver import check_certificate

pytestmark = pytest.mark.gpu

ALL_CASES = ps.LP_CASES + ps.QP_CASES


def methods_of(name):
    return ("hsd", "intpt", "pc") if name in ps.LP_CASES else ("qp", "pc")


def members(name):
    p, _, seed = ps.case(name)
    return p, ps.second_member(p, seed)


def values(p):
    """update()'s arguments for every number of p."""
    d = dict(A=p.A, b=p.b, c=p.c, f=p.f)
    if p.q is not None:
        d["q"] = p.q[2]
    return d


def run_all(ctx, methods, **kw):
    """{method: (status, trace text, (x, y, w, z))} of one run each."""
    out = {}
    for meth in methods:
        st, _, text = ctx.run(meth, trace=True, **kw)
        out[meth] = (st, text, ctx.solution())
    return out


def same(a, b):
    """Status, every character of the trace, every bit of x, y, w, z."""
    assert a[0] == b[0] and a[1] == b[1]
    for u, v in zip(a[2], b[2]):
        assert u.tobytes() == v.tobytes()


def fresh_runs(p, methods, **kw):
    ctx = ipo_amd.Context(p)
    try:
        return run_all(ctx, methods, **kw)
    finally:
        ctx.close()


def lines(text):
    return parse(text)[0]


# ---------------------------------------------------------------- update
@pytest.mark.parametrize("name,knob", [(c, k) for c in ALL_CASES for k in (None, "IPO_HIP_AX_JDS")]
                         + [(c, "IPO_HIP_Q_LONG") for c in ps.QP_CASES])
def test_update_equals_fresh(monkeypatch, name, knob):
    """After update() to member 2 every method's run is a fresh context's on
    member 2, and updating back reproduces the first runs.  IPO_HIP_AX_JDS=1:
    A x through the RowAxPlan, whose slices the update regathers (at these
    sizes it is otherwise off); IPO_HIP_Q_LONG=1: every nonempty column of Q
    read by the wave path from the refreshed Q (the QPs)."""
    for k in ("IPO_HIP_AX_JDS", "IPO_HIP_Q_LONG"):
        monkeypatch.delenv(k, raising=False)
    if knob:
        monkeypatch.setenv(knob, "1")
    p1, p2 = members(name)
    meths = methods_of(name)
    want1, want2 = fresh_runs(p1, meths), fresh_runs(p2, meths)
    ctx = ipo_amd.Context(p1)
    try:
        if knob == "IPO_HIP_Q_LONG":
            assert ctx.q_long() == int(np.count_nonzero(np.diff(p1.q[0])))
        first = run_all(ctx, meths)
        ctx.update(**values(p2))
        second = run_all(ctx, meths)
        ctx.update(**values(p1))
        back = run_all(ctx, meths)
    finally:
        ctx.close()
    for meth in meths:
        print(name, knob, meth, want1[meth][0], len(lines(want1[meth][1])), want2[meth][0], len(lines(want2[meth][1])))
        same(first[meth], want1[meth])
        same(second[meth], want2[meth])
        same(back[meth], want1[meth])
        assert want1[meth][1] != want2[meth][1]          # the members do differ


@pytest.mark.parametrize("name,part", [(c, k) for c in ALL_CASES for k in ("b", "c and f")]
                         + [(c, "q") for c in ps.QP_CASES])
def test_partial_update(name, part):
    """Only b, only c and f, only Q: the rest keeps member 1's numbers."""
    p1, p2 = members(name)
    mixed = ipo_amd.SolverForm(p1.m, p1.n, p1.kA, p1.iA, p1.A, p2.b if part == "b" else p1.b,
                               p2.c if part == "c and f" else p1.c, p2.f if part == "c and f" else p1.f,
                               q=p2.q if part == "q" else p1.q)
    kw = dict(b=p2.b) if part == "b" else dict(c=p2.c, f=p2.f) if part == "c and f" else dict(q=p2.q[2])
    meths = methods_of(name)
    want, want1 = fresh_runs(mixed, meths), fresh_runs(p1, meths)
    ctx = ipo_amd.Context(p1)
    try:
        ctx.update(**kw)
        got = run_all(ctx, meths)
    finally:
        ctx.close()
    for meth in meths:
        same(got[meth], want[meth])
        assert want[meth][1] != want1[meth][1]


def test_update_refusals_are_atomic():
    """Each refusal raises with a text, and the next run is bitwise the run
    before the attempt -- also after part of the arrays passed validation."""
    p1, p2 = members("banded 63x65")
    kQ, iQ, Q = p1.q
    cols = np.repeat(np.arange(p1.n), np.diff(kQ))
    off = int(np.nonzero(iQ != cols)[0][0])
    badA, badb, badQ = p2.A.copy(), p2.b.copy(), p2.q[2].copy()
    badA[p1.nz // 2] = np.nan
    badb[-1] = np.inf
    badQ[off] *= 1.5                                   # one side of an off-diagonal pair
    ctx = ipo_amd.Context(p1)
    try:
        before = run_all(ctx, ("qp", "pc"))
        attempts = [(dict(A=badA, b=p2.b, c=p2.c, q=p2.q[2]), r"A\[%d\]" % (p1.nz // 2)),
                    (dict(A=p2.A, b=badb), r"b\[%d\]" % (p1.m - 1)),
                    (dict(A=p2.A, c=p2.c, q=badQ), "symmetric"),
                    (dict(q=np.where(np.arange(Q.size) == 3, -np.inf, Q)), r"Q\[3\]"),
                    (dict(f=float("nan")), "f is not finite")]
        for kw, text in attempts:
            with pytest.raises(ipo_amd.IpoHipError, match=text):
                ctx.update(**kw)
            assert ipo_amd.last_error()
            after = run_all(ctx, ("qp", "pc"))
            for meth in before:
                same(after[meth], before[meth])
        # and it still takes a good update
        ctx.update(**values(p2))
        same(run_all(ctx, ("pc",))["pc"], fresh_runs(p2, ("pc",))["pc"])
    finally:
        ctx.close()


def test_update_refuses_q_on_an_lp_context_and_any_update_on_a_shard():
    from test_gpu_shard import DIMS
    p1, p2 = members("lp 63x65")
    ctx = ipo_amd.Context(p1)
    try:
        before = run_all(ctx, ("intpt",))
        with pytest.raises(ipo_amd.IpoHipError, match="without Q"):
            ctx.update(b=p2.b, q=np.ones(p1.n))
        same(run_all(ctx, ("intpt",))["intpt"], before["intpt"])
    finally:
        ctx.close()
    loc = ipo_amd.shard_block_angular(ipo_amd.synth_block_angular(*DIMS), 1, 0)
    sh = ipo_amd.ShardContext(loc)
    try:
        before = run_all(sh, ("intpt",))
        for kw in (dict(b=loc.b * 1.1), dict(A=loc.A, c=loc.c), dict(f=1.0)):
            with pytest.raises(ipo_amd.IpoHipError, match="shard"):
                sh.update(**kw)
        same(run_all(sh, ("intpt",))["intpt"], before["intpt"])
        # every start entry is refused on a shard too
        x, y, w, z = sh.solution()
        with pytest.raises(ipo_amd.IpoHipError, match="shard"):
            sh.set_start(x + 1, y + 1, w + 1, z + 1)
        with pytest.raises(ipo_amd.IpoHipError, match="shard"):
            sh.start_from_last(1.0)
        with pytest.raises(ipo_amd.IpoHipError, match="shard"):
            sh.clear_start()
        same(run_all(sh, ("intpt",))["intpt"], before["intpt"])
    finally:
        sh.close()


# ---------------------------------------------------------------- start points
def start_methods(name):
    return ("intpt", "pc") if name in ps.LP_CASES else ("qp", "pc")


@pytest.mark.parametrize("name", ALL_CASES)
def test_default_start_made_explicit(name):
    p, _ = members(name)
    meths = start_methods(name)
    ctx = ipo_amd.Context(p)
    try:
        default = run_all(ctx, meths)
        ctx.set_start(np.full(p.n, 1000.0), np.full(p.m, 1000.0), np.full(p.m, 1000.0), np.full(p.n, 1000.0))
        explicit = run_all(ctx, meths)
        ctx.clear_start()
        cleared = run_all(ctx, meths)
    finally:
        ctx.close()
    for meth in meths:
        assert default[meth][0] == 0
        same(explicit[meth], default[meth])
        same(cleared[meth], default[meth])


# The cases of the continuation: all four, each by the methods that take a
# start.  They are cases on which the uninterrupted run has not raised
# eps_diag within its first five factorisations (small, well-conditioned
# systems and afiro): a run that had would go on with the raised value, the
# resumed one with the 1e-14 every run starts from, and the lines would part
# -- the equality below is also the evidence that none does.  All end
# optimal, which intpt's and qp's give-up tests need: they compare a line
# with the one before, and the resumed run's line 0 has none.
@pytest.mark.parametrize("name", ALL_CASES)
def test_continuation(name):
    """Stopped after five iterations (status 5) and resumed from the iterate
    it left, a run prints the uninterrupted run's lines 5 ... in every field
    but the iteration number and ends on the same solution bits."""
    p, _ = members(name)
    ctx = ipo_amd.Context(p)
    try:
        for meth in start_methods(name):
            st, _, whole = ctx.run(meth, trace=True)
            sol = ctx.solution()
            st5, _, head = ctx.run(meth, max_iter=5, trace=True)
            it5 = ctx.solution()
            assert st == 0 and st5 == 5 and lines(head) == lines(whole)[:5]
            ctx.start_from_last(0.5 * min(v.min() for v in it5))       # below every entry: the iterate itself
            st2, _, rest = ctx.run(meth, trace=True)
            ctx.clear_start()
            a, b = lines(rest), lines(whole)[5:]
            print(name, meth, len(lines(whole)), len(a))
            assert st2 == 0 and len(a) == len(b) and len(a) > 1
            for u, v in zip(a, b):
                assert u[0] == v[0] - 5 and u[1:] == v[1:]
            # the printed text too, the iteration number apart
            ta = [ln[8:] for ln in rest.splitlines() if ln[:8].strip().isdigit()]
            tb = [ln[8:] for ln in whole.splitlines() if ln[:8].strip().isdigit()][5:]
            assert ta == tb
            for u, v in zip(ctx.solution(), sol):
                assert u.tobytes() == v.tobytes()
    finally:
        ctx.close()


def printed(v, digits):
    """v as the trace prints it (%14.7e: digits = 7, %8.1e: 1) and read back."""
    return float(f"{v:.{digits}e}")


@pytest.mark.parametrize("name", ALL_CASES)
def test_clamping(name):
    """start_from_last(1.0) after a converged run, then one line: the line of
    np.maximum(solution, 1.0), to the printed digits.  The device sums in
    another order than NumPy, in fp64: that moves a value by parts in 1e16 of
    its terms, so the single-precision number printed can differ by one unit
    of float32 (6e-8 relative; 1.2e-7 allows for the decimal rounding of
    both), and a norm printed to two digits by one unit of its last."""
    p, _ = members(name)
    ctx = ipo_amd.Context(p)
    try:
        assert ctx.run("pc")[0] == 0
        sol = ctx.solution()
        ctx.start_from_last(1.0)
        st, stats, text = ctx.run("pc", max_iter=1, trace=True)
    finally:
        ctx.close()
    x, y, w, z = (np.maximum(v, 1.0) for v in sol)
    assert any((v < 1.0).any() for v in sol)                    # the floor did bite
    want, _ = ps.line_of(p, x, y, w, z)
    got = lines(text)
    print(got, want)
    assert st == 5 and len(got) == 1 and got[0][0] == 0
    for k, digits in ((1, 7), (2, 1), (3, 7), (4, 1)):
        ref = printed(want[k], digits)
        unit = 10.0 ** (np.floor(np.log10(abs(ref))) - digits) if ref != 0 else 0.0
        tol = 1.2e-7 * abs(ref) if digits == 7 else 1.0001 * unit
        assert abs(got[0][k] - ref) <= tol, (k, got[0][k], ref)


def test_start_refusals():
    p, _ = members("lp 63x65")
    ctx = ipo_amd.Context(p)
    try:
        with pytest.raises(ipo_amd.IpoHipError, match="no run"):
            ctx.start_from_last(1.0)
        default = run_all(ctx, ("intpt",))["intpt"]
        rng = np.random.default_rng(3)
        good = [rng.uniform(0.5, 2.0, k) for k in (p.n, p.m, p.m, p.n)]
        ctx.set_start(*good)
        held = run_all(ctx, ("intpt",))["intpt"]
        assert held[0] == 0 and held[1] != default[1]
        for which, pos, val, text in ((0, 5, 0.0, r"x\[5\]"), (1, p.m - 1, -1.0, r"y\[%d\]" % (p.m - 1)),
                                      (2, 0, np.nan, r"w\[0\]"), (3, 64, np.inf, r"z\[64\]")):
            bad = [v.copy() for v in good]
            bad[which][pos] = val
            with pytest.raises(ipo_amd.IpoHipError, match=text):
                ctx.set_start(*bad)
            same(run_all(ctx, ("intpt",))["intpt"], held)           # the earlier start survives
        for floor in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(ipo_amd.IpoHipError, match="floor"):
                ctx.start_from_last(floor)
        same(run_all(ctx, ("intpt",))["intpt"], held)
        # hsd and hsdls take no start: 7, an error text, no iteration
        for meth in ("hsd", "hsdls"):
            st, stats, text = ctx.run(meth, trace=True)
            assert st == 7 and stats["iters"] == 0 and "start" in ipo_amd.last_error() and "Iter" not in text
        ctx.clear_start()
        same(run_all(ctx, ("intpt",))["intpt"], default)
        assert ctx.run("hsd")[0] != 7
    finally:
        ctx.close()


def test_a_start_does_not_leak():
    """intpt, pc from a start, clear_start, intpt again: the two intpt runs
    are identical (test_gpu_pc.test_intpt_unchanged_by_a_pc_run_between's shape)."""
    p, _ = members("afiro")
    ctx = ipo_amd.Context(p)
    try:
        st0, _, t0 = ctx.run("intpt", trace=True)
        a = ctx.solution()
        st1, _, t1 = ctx.run("pc", trace=True)
        ctx.start_from_last(1.0)
        st2, _, t2 = ctx.run("pc", trace=True)
        ctx.clear_start()
        st3, _, t3 = ctx.run("intpt", trace=True)
        b = ctx.solution()
    finally:
        ctx.close()
    assert st0 == st1 == st2 == st3 == 0 and t0 == t3 and t2 != t1
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes()


@pytest.mark.parametrize("name", ALL_CASES)
def test_a_warm_solve_is_still_a_solve(name):
    """Member 1 solved, updated to member 2, started from the clamped
    solution: optimal, with the certificate of a cold solve.  The floor is
    pc_start_ref.WARM_FLOOR units of sqrt(gamma / (n + m)) on every case
    (test_resolve_ref.test_warm_floor).  Line counts are printed only."""
    p1, p2 = members(name)
    ctx = ipo_amd.Context(p1)
    try:
        st1, stats1, _ = ctx.run("pc")
        floor = ps.warm_floor(stats1["final_mu"], p1)      # final_mu: the last line's gamma = z'x + y'w
        ctx.update(**values(p2))
        ctx.start_from_last(floor)                          # member 1's solution, raised to the floor
        st2, warm, _ = ctx.run("pc")
        x, y, w, z = ctx.solution()
        ctx.clear_start()
        cold_st, cold, _ = ctx.run("pc")
    finally:
        ctx.close()
    print(f"{name}: floor {floor:.3e}; cold {cold['iters']} lines, warm {warm['iters']}")
    assert st1 == 0 and cold_st == 0 and st2 == 0 and floor > 0
    check_certificate(p2, x, y, w, z)
