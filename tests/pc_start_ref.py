"""pc_ref.solve_pc restated with a start argument, for the start-point
entries of a context (Context.set_start / start_from_last): the same
iteration, line for line (tests/pc_ref.py's docstring states it), from a
given x, y, w, z in place of "every variable 1000".  pc_ref.py itself is the
yardstick of method "pc" and stays as it is; tests/test_resolve_ref.py holds
the two together (the same rows and solution bits from the default start).

Also here, for tests/test_gpu_resolve.py: its cases, the "second member" of a
problem family (the same pattern, other numbers) a context is updated to, the
printed line of one iterate, and the warm start's floor.
"""
import numpy as np

import ipo_amd
import pc_ref
from qp_ref import _Dense, _Oracle, _mats

STEP = pc_ref.STEP

# name -> (make, its arguments, the reference's back end, second_member's seed).
# The seeds: pc_ref and qp_ref (the LP by intpt's iteration when q is None)
# both end optimal on the second member.  0 makes afiro's second member
# infeasible and on 1 intpt's iteration gives up on it; 3 is the one of 2 .. 6
# whose warm runs are shortest.  The synthetic cases pass at 0 and 1; 1 is
# taken.  (test_resolve_ref.py checks what the GPU tests rely on.)
CASES = {
    "lp 63x65": ("lp_shape", (63, 65, 0), "dense", 1),
    "afiro": ("netlib_lp", ("afiro",), "oracle", 3),
    "banded 63x65": ("small_case", (63, 65, "banded", 12), "dense", 1),
    "gaps 20x30": ("small_case", (20, 30, "gaps", 2), "dense", 1),
}
LP_CASES = ("lp 63x65", "afiro")
QP_CASES = ("banded 63x65", "gaps 20x30")
# The warm start's floor, in units of sqrt(final gamma / (n + m)) of the
# previous solve (the geometric mean of a complementary pair there): the
# restated iteration ends optimal on every case's second member from
# max(previous solution, floor) at a decade either side of it too, which
# covers the device's final gamma standing apart from the reference's.
WARM_FLOOR = 1.0e4


def case(name):
    import test_pc
    make, args, backend, seed = CASES[name]
    return getattr(test_pc, make)(*args), backend, seed


def warm_floor(gamma, p, mult=WARM_FLOOR):
    return mult * float(np.sqrt(gamma / (p.n + p.m)))


def f32(v):
    return float(np.float32(v))


def line_of(p, x, y, w, z, it=0):
    """(it, pobj, normr, dobj, norms) as methods intpt, qp and pc print the
    iterate x, y, w, z, and gamma = z'x + y'w."""
    A, Q = _mats(p)
    b, c, f = np.asarray(p.b, np.float64), np.asarray(p.c, np.float64), float(p.f)
    qx = Q @ x if Q is not None else np.zeros(p.n)
    rho = b - A @ x - w
    sig = ((c - A.T @ y) + z) - qx
    hxqx = 0.5 * (x @ qx)
    return ((it, f32(c @ x - hxqx + f), f32(np.sqrt(rho @ rho)), f32(b @ y + hxqx + f), f32(np.sqrt(sig @ sig))),
            z @ x + y @ w)


def solve_pc(p, backend="dense", max_iter=200, start=None):
    """pc_ref.solve_pc(p, backend, max_iter) (stored summation order, the
    relative guard) from start = (x, y, w, z); None: every variable 1000.
    Returns its fields and gamma, the last line's z'x + y'w."""
    m, n = p.m, p.n
    A, Q = _mats(p)
    At = A.T.tocsr()
    qxf = (lambda v: Q @ v) if Q is not None else (lambda v: np.zeros(n))
    b, c, f = np.asarray(p.b, np.float64), np.asarray(p.c, np.float64), float(p.f)
    lin = (_Dense(p) if backend == "dense" else (_Oracle(p) if Q is not None else pc_ref._OracleLp(p))
           if backend == "oracle" else backend)
    if start is None:
        x, z = np.full(n, 1000.0), np.full(n, 1000.0)
        y, w = np.full(m, 1000.0), np.full(m, 1000.0)
    else:
        x, y, w, z = (np.array(v, np.float64, copy=True) for v in start)
        assert x.shape == z.shape == (n,) and y.shape == w.shape == (m,)
        assert all(np.all(np.isfinite(v)) and np.all(v > 0) for v in (x, y, w, z))
    normr0 = norms0 = np.inf
    normr1 = norms1 = None
    rows, status, gamma = [], 5, np.nan

    def ratio(dx, dz, dy, dw):
        return max(0.0, np.max(-dx / x), np.max(-dz / z), np.max(-dy / y), np.max(-dw / w))

    for it in range(max_iter):
        rho = b - A @ x - w
        qx = qxf(x)
        sig = ((c - At @ y) + z) - qx
        normr, norms = f32(np.sqrt(rho @ rho)), f32(np.sqrt(sig @ sig))
        gamma = z @ x + y @ w
        hxqx = 0.5 * (x @ qx)
        rows.append((it, f32(c @ x - hxqx + f), normr, f32(b @ y + hxqx + f), norms))
        if it == 0:
            normr1, norms1 = normr, norms
        if normr < 1.0e-6 and norms < 1.0e-6 and gamma < 1.0e-6:
            status = 0
            break
        if normr > 10 * normr0 and normr >= 1.0e-6 * (1.0 + normr1):
            status = 2
            break
        if norms > 10 * norms0 and norms >= 1.0e-6 * (1.0 + norms1):
            status = 4
            break
        D, E = z / x, w / y
        dya, dxa = lin.solve(E, D, rho + w, sig - z)
        dza = -z - D * dxa
        dwa = -w - E * dya
        t = ratio(dxa, dza, dya, dwa)
        ta = 1.0 if t <= 1.0 else 1.0 / t
        g1 = z @ dxa + x @ dza + w @ dya + y @ dwa
        g2 = dxa @ dza + dya @ dwa
        ga = gamma + ta * (g1 + ta * g2)
        s = min(1.0, max(0.0, ga / gamma))
        mu = s * s * s * gamma / (n + m)
        cx, cy = mu - dxa * dza, mu - dya * dwa
        dy, dx = lin.solve(E, D, rho + w - cy / y, sig - z + cx / x)
        dz = cx / x - z - D * dx
        dw = cy / y - w - E * dy
        t = ratio(dx, dz, dy, dw)
        theta = 1.0 if t == 0.0 or STEP / t > 1.0 else STEP / t
        x, z, y, w = x + theta * dx, z + theta * dz, y + theta * dy, w + theta * dw
        normr0, norms0 = normr, norms
    return dict(status=status, iters=len(rows), rows=rows, x=x, y=y, w=w, z=z, gamma=gamma)


def second_member(p, seed):
    """The same pattern with other numbers: A, b and c multiplied entry by
    entry by seeded factors in [0.8, 1.25], Q by d d' with d in [0.8, 1.25]
    up to a square root (so Q's factors lie in [0.8, 1.25] too, Q stays
    symmetric bit for bit -- d_i d_j is commutative -- and positive
    semidefinite), f shifted."""
    rng = np.random.default_rng([seed, p.m, p.n, 77])
    fac = lambda k: np.exp(rng.uniform(np.log(0.8), np.log(1.25), k))      # noqa: E731
    A, b, c = p.A * fac(p.nz), p.b * fac(p.m), p.c * fac(p.n)
    q = getattr(p, "q", None)
    if q is not None:
        kQ, iQ, Q = q
        d = np.sqrt(fac(p.n))
        cols = np.repeat(np.arange(p.n), np.diff(kQ))
        q = (kQ, iQ, Q * (d[iQ] * d[cols]))
    return ipo_amd.SolverForm(p.m, p.n, p.kA, p.iA, A, b, c, p.f + 0.25, q=q)
