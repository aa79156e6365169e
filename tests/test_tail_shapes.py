"""Small synthetic KKT systems whose dense tail has a chosen size (host code,
no GPU): the shapes tests/test_gpu_tail_shapes.py runs every dense-tail path
over, their tail sizes pinned through ipo_hip_symbolic_tail, and the fp64
oracle (oracle/orc_kkt.c, its three summation orders) measured against the
long-double LDL' of tests/kkt_ref.py.  The oracle's distance from that
reference is the unit of the GPU tests' bounds.

Shapes (tests/kkt_ref.py: dense_lp, rows_lp):
  S1  dense (m, m + 8) at tail density 1: nt = m + 1 = 128, 129, 143, 144, 145,
      191, 192, 193, 256, 257, 321, 577 -- 2, 3, 4, 5, 6 and 10 block columns,
      last blocks of 64, 1, 15, 16, 17 and 63 rows;
  S2  dense at the default density: the whole matrix is the tail (tail_c0 = 0,
      no sparse supernode), nt = 128, 129, 192, 256, 262; (59, 68) has
      T = 127 < kTailMin and no tail at all;
  S3  260 / 300 rows of which 104 ... 200 are dense, 600 columns: an
      elimination tree of 13-16 levels under the tail, gather tasks with
      partial masks; nt 128 ... 236 at density 1, 273 ... 506 at the default.

Scalings: "unit", E, D ~ U(0.1, 10); "wide", log-uniform in [1e-6, 1e6].

Measured (this module, the largest over shapes and the three summation orders):
  pivots    max |d_orc - d_ref| / |d_ref|
            unit  S1 2.2e-14 (nt 577; 1.7e-15 ... 8.6e-15 below it), S2 4.0e-15, S3 5.4e-15
            wide  S1 2.4e-09, S2 1.3e-09, S3 2.9e-05
  solution  ||x_orc - x_ref||_inf / (1 + ||x_ref||_inf)
            unit  S1 1.0e-14, S2 2.3e-15, S3 2.0e-15
            wide  S1 7.8e-13, S2 1.1e-12, S3 1.4e-11
  refinement passes: 1 at unit scaling, 2 at wide scaling; no dependent pivot
  anywhere.
At wide scaling the distances are those of the systems, not of the oracle:
pivots there are small differences of terms twelve decades apart, and every
fp64 summation order is equally far from the reference (the three orders
within a factor of about 4 of one another on every shape).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import ipo_amd
import kkt_ref
import oracle_lib

SEED = 20251121
SCALINGS = ("unit", "wide")

# (id, family, shape, tail density or None for the default, nt)
S1 = [(f"S1-nt{m + 1}", "dense", (m, m + 8), 1.0, m + 1)
      for m in (127, 128, 142, 143, 144, 190, 191, 192, 255, 256, 320, 576)]
S2 = [(f"S2-{m}x{n}", "dense", (m, n), None, nt)
      for (m, n), nt in (((60, 68), 128), ((60, 69), 129), ((92, 100), 192), ((124, 132), 256), ((127, 135), 262),
                         ((59, 68), 0))]
_ROWS = (((260, 600, 104), 128, 273), ((260, 600, 105), 129, 275), ((260, 600, 110), 134, 286),
         ((260, 600, 140), 170, 364), ((260, 600, 160), 196, 418), ((300, 600, 200), 236, 506))
S3 = [(f"S3-r{s[2]}-rho1", "rows", s, 1.0, a) for s, a, _ in _ROWS] + \
     [(f"S3-r{s[2]}-dflt", "rows", s, None, b) for s, _, b in _ROWS]
SHAPES = S1 + S2 + S3
SHAPE_IDS = [s[0] for s in SHAPES]
# the whole solves of the GPU module (Test D)
SOLVE_SHAPES = ((60, 69), (127, 135), (192, 200))


def distinct_lps():
    """(family, shape) of SHAPES, each once (the two densities of S3 share their LPs)."""
    seen = []
    for _, fam, shape, _, _ in SHAPES:
        if (fam, shape) not in seen:
            seen.append((fam, shape))
    return seen


@functools.lru_cache(maxsize=None)
def oracle_case(family, shape, kind):
    """The oracle on case (family, shape, SEED, kind) under its three
    summation orders: per order (ndep, live, pivots, (y, x), passes), and the
    largest pivot and solution distance from the long-double reference."""
    c = kkt_ref.case(family, shape, SEED, kind)
    L = oracle_lib.lib()
    runs = []
    try:
        for order in (0, 1, 2):
            L.orc_set_perturb(order)
            o = oracle_lib.OracleKkt(c.p)
            o.factor(c.E, c.D)
            assert np.array_equal(o.perm(), c.perm)
            y, x, _ = o.solve(c.E, c.D, c.fy, c.fx)
            runs.append((o.info()["ndep"], o.live().copy(), o.diag().copy(), (y, x), o.info()["passes"]))
    finally:
        L.orc_set_perturb(0)
    dpiv = [c.pivot_distance(r[2]) for r in runs]
    dsol = [c.solution_distance(*r[3]) for r in runs]
    return dict(runs=runs, pivot=dpiv, solution=dsol, passes=max(r[4] for r in runs))


@pytest.mark.parametrize("family,shape", [("dense", (60, 69)), ("rows", (60, 140, 24))])
@pytest.mark.parametrize("kind", SCALINGS)
def test_reference_reproduces_k(family, shape, kind):
    """L diag(d) L' of the reference is the permuted K to the backward-error
    bound of an LDL' in long double: 64 eps_ld ||K||_max T (Higham's
    gamma_T |L||D||L'| with the growth these quasi-definite systems show,
    far below 64; derived, not measured)."""
    c = kkt_ref.case(family, shape, SEED, kind)
    K = kkt_ref.kkt_dense(c.p, c.E, c.D)
    L, d = kkt_ref.ldl_ref(K, c.perm)
    assert np.array_equal(d, c.d)
    Kp = K[np.ix_(c.perm, c.perm)].astype(np.longdouble)
    err = np.abs((L * d) @ L.T - Kp).max()
    T = K.shape[0]
    bound = 64 * np.finfo(np.longdouble).eps * np.abs(K).max() * T
    print(f"{family}{shape} {kind}: |L D L' - K|_max {float(err):.2e}, bound {float(bound):.2e}")
    assert err <= bound
    # and the solve: K (y, x) = (fy, fx) to the same accuracy relative to |K| |x|
    sol = np.concatenate([c.y, c.x])
    r = K.astype(np.longdouble) @ sol - np.concatenate([c.fy, c.fx])
    assert np.abs(r).max() <= bound * (1 + np.abs(sol).max())


@pytest.mark.parametrize("kind", SCALINGS)
@pytest.mark.parametrize("family,shape", distinct_lps(), ids=lambda v: str(v).replace(" ", ""))
def test_oracle_against_reference(family, shape, kind):
    """The fp64 oracle under its three summation orders: no dependent pivot,
    every node live; its pivot and solution distances from the long-double
    reference are printed.  The GPU module's bounds are multiples of these
    distances, so a reference or oracle gone wrong must not widen them
    unnoticed: at unit scaling they stay inside the suite's own oracle bars
    for well-scaled systems (1e-9 and 1e-8, tests/test_gpu_kkt.py).

    Refinement passes: one at unit scaling.  At wide scaling two, under every
    order on every shape: scalings twelve decades apart make pivots that are
    small differences of large terms, which any fp64 factor holds to 1e-10 ...
    1e-6 relative only (the printed pivot distances); the first solve's
    residual inherits that and is above the loop's target of
    1e-10 (1 + |f|_inf) (ldlt.c:327-425), the second pass brings it under.  A
    third would mean the residual stopped halving."""
    o = oracle_case(family, shape, kind)
    for ndep, live, _, _, passes in o["runs"]:
        assert ndep == 0
        assert live.all()
        assert passes == 1 if kind == "unit" else 1 <= passes <= 2
    print(f"{family}{shape} {kind}: oracle pivot distance {['%.2e' % v for v in o['pivot']]}, "
          f"solution distance {['%.2e' % v for v in o['solution']]}, passes {[r[4] for r in o['runs']]}")
    assert 0 < max(o["pivot"]) < np.inf and max(o["solution"]) < np.inf
    if kind == "unit":
        assert max(o["pivot"]) <= 1e-9
        assert max(o["solution"]) <= 1e-8


@pytest.mark.parametrize("sid,family,shape,density,nt", SHAPES, ids=SHAPE_IDS)
def test_tail_sizes_pinned(sid, family, shape, density, nt, monkeypatch):
    """The tail each shape is there for, through the device plan's own
    density choice (ipo_hip_symbolic_tail)."""
    monkeypatch.delenv("IPO_HIP_TAIL_DENSITY", raising=False)
    p = kkt_ref.make_lp(family, shape, SEED)
    t = ipo_amd.symbolic_tail(p.m, p.n, p.kA, p.iA, density)
    assert t["nt"] == nt
    assert t["tail_c0"] == (p.m + p.n - nt if nt else p.m + p.n)
    assert t["ntb"] == (nt + 63) // 64
    if family == "dense" and density is None and nt:
        assert t["tail_c0"] == 0 and nt == p.m + p.n        # the whole matrix, no sparse supernode
    if density is not None:
        # what a device factor built under IPO_HIP_TAIL_DENSITY gets is the same plan
        monkeypatch.setenv("IPO_HIP_TAIL_DENSITY", repr(density))
        assert ipo_amd.symbolic_tail(p.m, p.n, p.kA, p.iA) == t
    if family == "dense" and density == 1.0:
        s = ipo_amd.symbolic_forced(p.m, p.n, p.kA, p.iA, 0)
        assert s["tail_c0"] == t["tail_c0"] and s["nlevels"] == 1 and s["nsup"] == p.n - 1


def test_solve_shapes_tails(monkeypatch):
    """The whole-solve shapes: all-tail at the default density; at density 1
    the reference's window (none below kTailMin)."""
    monkeypatch.delenv("IPO_HIP_TAIL_DENSITY", raising=False)
    for (m, n), nt1 in zip(SOLVE_SHAPES, (0, 128, 193)):
        p = kkt_ref.dense_lp(m, n, SEED)
        assert ipo_amd.symbolic_tail(m, n, p.kA, p.iA) == dict(tail_c0=0, nt=m + n, ntb=(m + n + 63) // 64)
        assert ipo_amd.symbolic_tail(m, n, p.kA, p.iA, 1.0)["nt"] == nt1


@functools.lru_cache(maxsize=None)
def oracle_hsd(shape):
    """The oracle's HSD solve of dense_lp(*shape, SEED) under its three summation orders."""
    p = kkt_ref.dense_lp(*shape, SEED)
    L = oracle_lib.lib()
    out = []
    try:
        for order in (0, 1, 2):
            L.orc_set_perturb(order)
            out.append(oracle_lib.solve_arrays(p, "hsd"))
    finally:
        L.orc_set_perturb(0)
    return out


@pytest.mark.parametrize("shape", SOLVE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_solve_shapes_oracle_orders_agree(shape):
    """What makes the whole solves of these LPs a property a device solve
    can be held to: the oracle's three summation orders end with status 0
    after the same number of iterations, at objectives equal to 1e-9
    relative (measured: 1e-11; the device is held to 1e-6)."""
    runs = oracle_hsd(shape)
    print(f"dense{shape}: iterations {[r['iters'] for r in runs]}, pobj {[r['final_pobj'] for r in runs]}")
    assert [r["status"] for r in runs] == [0, 0, 0]
    assert len({r["iters"] for r in runs}) == 1
    for key in ("final_pobj", "final_dobj"):
        v = [r[key] for r in runs]
        assert max(v) - min(v) <= 1e-9 * max(1.0, abs(v[0]))


@pytest.mark.parametrize("kl", [1, 4, 6])
def test_run_schedule_accepts_chunkings(kl):
    """The visit chunkings the GPU module sets (IPO_HIP_VISIT_BLOCKS =
    IPO_HIP_VISIT_LATEST = 1, 4, 6): the persistent run's schedule builds for
    every tail size used, on devices of 256 and of 64 CUs."""
    f = ipo_amd.lib().ipo_hip_tail_run_schedule
    f.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint), C.c_int, C.POINTER(C.c_int)]
    f.restype = C.c_int
    for nt in sorted({s[4] for s in SHAPES if s[4]} | {m + n for m, n in SOLVE_SHAPES}):
        for cap in (256, 64):
            assert f(nt, kl, kl, cap, None, 0, None) > 0, (nt, kl, cap, ipo_amd.last_error())
