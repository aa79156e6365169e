"""The yardstick of the predictor-corrector solver (method "pc"): Mehrotra's
iteration restated in NumPy on qp_ref's problems and back ends (a plain
module, no fixtures).

The problem, in solver form (Q may be empty: the LP):

    maximise  c'x + f - x'Qx / 2    s.t.  A x <= b,  x >= 0      (Q PSD)

Each iteration opens as qp_ref.solve_qp's (intpt.c's): the start (every
variable 1000), rho, sigma, Q x, gamma = z'x + y'w, the objectives, the
single-precision printed line and the stop rule (normr, norms and gamma all
below 1e-6).  Then, with D = z / x, E = w / y and one factorisation:

  give-up   status 2 if normr > 10 normr0 and normr >= 1e-6 (1 + normr1),
            status 4 likewise with norms; normr0 / norms0 the previous
            line's norms, normr1 / norms1 those of line 0.  (intpt's test is
            the first half alone: once a residual sits at its rounding floor
            it fires on noise.  guard="absolute" puts a plain 1e-6 in the
            second half's place, the variant the relative form was chosen
            over; guard="intpt" is intpt's test.)
  predictor -E dy + A dx = rho + w,  A'dy + (D + Q) dx = sigma - z
            dza = -z - D dxa,  dwa = -w - E dya
            t = max(0, max -dxa / x, -dza / z, -dya / y, -dwa / w)
            theta_a = 1 if t <= 1 else 1 / t
  centring  g1 = z'dxa + x'dza + w'dya + y'dwa,  g2 = dxa'dza + dya'dwa
            gamma_a = gamma + theta_a (g1 + theta_a g2)
            s = min(1, max(0, gamma_a / gamma))^3,  mu = s gamma / (n + m)
  corrector cx = mu - dxa dza,  cy = mu - dya dwa  (entry by entry)
            the same factor, right-hand sides rho + w - cy / y and
            sigma - z + cx / x
            dz = cx / x - z - D dx,  dw = cy / y - w - E dy
            theta = min(1, 0.95 / t), t over the corrected directions
            (theta = 1 if t = 0); one step length for x, z, y, w.
"""
import functools

import numpy as np

import qp_ref
from qp_ref import _Dense, _Oracle, _mats

STEP = 0.95


class _OracleLp:
    """The oracle back end for a problem without Q: oracle_lib.OracleKkt on
    the LP's own K = [-E A; A' D], not qp_ref._Oracle's swapped form -- the
    factor method "pc" itself uses for an LP."""

    def __init__(self, p):
        import oracle_lib
        self.k = oracle_lib.OracleKkt(p)

    def solve(self, E, D, fy, fx):
        self.k.factor(E, D)
        dy, dx, _ = self.k.solve(E, D, fy, fx)
        return dy, dx


class Noisy:
    """A back end whose solutions carry seeded Gaussian noise of standard
    deviation `level` max |solution| per entry: the size of what a refined
    solve's stopping rule may leave."""

    def __init__(self, lin, seed, level=1e-13):
        self.lin, self.rng, self.level = lin, np.random.default_rng(seed), level

    def solve(self, E, D, fy, fx):
        dy, dx = self.lin.solve(E, D, fy, fx)
        a = self.level * max(np.abs(dy).max(), np.abs(dx).max())
        return dy + a * self.rng.standard_normal(dy.size), dx + a * self.rng.standard_normal(dx.size)


def solve_pc(p, backend="dense", max_iter=200, shuffle=None, guard="relative"):
    """The iteration of the module docstring.  Returns qp_ref.solve_qp's
    fields: dict(status, iters, rows, x, y, w, z, growth, floor), rows[k] =
    (k, pobj, normr, dobj, norms) as method "pc" prints line k.
    backend: "dense" (qp_ref._Dense), "oracle" (qp_ref._Oracle's swapped
    factor with Q, _OracleLp without), or an object with their
    solve(E, D, fy, fx).
    shuffle = a seed: A x, A'y and Q x summed in a random order of their terms."""
    m, n = p.m, p.n
    A, Q = _mats(p)
    At = A.T.tocsr()
    if shuffle is not None:
        rs = np.random.default_rng(shuffle)
        pn, pm = rs.permutation(n), rs.permutation(m)
        An, Am = A[:, pn], At[:, pm]
        Qn = Q[:, pn] if Q is not None else None
        ax = lambda v: An @ v[pn]                     # noqa: E731
        aty = lambda v: Am @ v[pm]                    # noqa: E731
        qxf = lambda v: Qn @ v[pn] if Q is not None else np.zeros(n)    # noqa: E731
    else:
        ax = lambda v: A @ v                          # noqa: E731
        aty = lambda v: At @ v                        # noqa: E731
        qxf = lambda v: Q @ v if Q is not None else np.zeros(n)         # noqa: E731
    b, c, f = np.asarray(p.b, np.float64), np.asarray(p.c, np.float64), float(p.f)
    lin = (_Dense(p) if backend == "dense" else (_Oracle(p) if Q is not None else _OracleLp(p)) if backend == "oracle"
           else backend)
    x, z = np.full(n, 1000.0), np.full(n, 1000.0)
    y, w = np.full(m, 1000.0), np.full(m, 1000.0)
    normr0 = norms0 = np.inf
    normr1 = norms1 = None
    rows, status, growth, floor = [], 5, 0.0, 0.0
    f32 = lambda v: float(np.float32(v))     # noqa: E731

    def ratio(dx, dz, dy, dw):
        return max(0.0, np.max(-dx / x), np.max(-dz / z), np.max(-dy / y), np.max(-dw / w))

    def gives_up(v, v0, v1):
        if not v > 10 * v0:
            return False
        return True if guard == "intpt" else v >= 1.0e-6 if guard == "absolute" else v >= 1.0e-6 * (1.0 + v1)

    for it in range(max_iter):
        rho = b - ax(x) - w
        qx = qxf(x)
        sig = ((c - aty(y)) + z) - qx
        normr, norms = f32(np.sqrt(rho @ rho)), f32(np.sqrt(sig @ sig))
        gamma = z @ x + y @ w
        hxqx = 0.5 * (x @ qx)
        pobj, dobj = f32(c @ x - hxqx + f), f32(b @ y + hxqx + f)
        rows.append((it, pobj, normr, dobj, norms))
        if it == 0:
            normr1, norms1 = normr, norms
        if normr < 1.0e-6 and norms < 1.0e-6 and gamma < 1.0e-6:
            status = 0
            break
        growth = max(growth, normr / normr0 if normr0 > 0 else np.inf if normr > 0 else 0.0,
                     norms / norms0 if norms0 > 0 else np.inf if norms > 0 else 0.0)
        if gives_up(normr, normr0, normr1):
            status = 2
            break
        if gives_up(norms, norms0, norms1):
            status = 4
            break
        D, E = z / x, w / y
        # predictor
        fy, fx = rho + w, sig - z
        dya, dxa = lin.solve(E, D, fy, fx)
        dza = -z - D * dxa
        dwa = -w - E * dya
        t = ratio(dxa, dza, dya, dwa)
        ta = 1.0 if t <= 1.0 else 1.0 / t
        # centring
        g1 = z @ dxa + x @ dza + w @ dya + y @ dwa
        g2 = dxa @ dza + dya @ dwa
        ga = gamma + ta * (g1 + ta * g2)
        s = min(1.0, max(0.0, ga / gamma))
        mu = s * s * s * gamma / (n + m)
        # corrector
        cx, cy = mu - dxa * dza, mu - dya * dwa
        fy, fx = rho + w - cy / y, sig - z + cx / x
        floor = 1.0e-10 * (max(np.abs(fy).max(), np.abs(fx).max()) + 1.0)
        dy, dx = lin.solve(E, D, fy, fx)
        dz = cx / x - z - D * dx
        dw = cy / y - w - E * dy
        t = ratio(dx, dz, dy, dw)
        theta = 1.0 if t == 0.0 or STEP / t > 1.0 else STEP / t
        x, z, y, w = x + theta * dx, z + theta * dz, y + theta * dy, w + theta * dw
        normr0, norms0 = normr, norms
    return dict(status=status, iters=len(rows), rows=rows, x=x, y=y, w=w, z=z, growth=growth, floor=floor)


@functools.lru_cache(maxsize=None)
def reference(key, make, backend):
    """(problem, its reference run) of make(*key), computed once per process
    and shared, read-only, by the tests that need it."""
    p = make(*key)
    return p, solve_pc(p, backend)


certificate = qp_ref.certificate
objective = qp_ref.objective
