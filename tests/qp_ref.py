"""The yardstick of the QP path-following solver (method "qp"): the
iteration restated in NumPy, and the problems it is run on (a plain module,
no fixtures).

The reference has no QP loop (ldlt.c carries Q only for an outside caller),
so method "qp" is an extension and this module is what it is held to.  The
problem, in solver form:

    maximise  c'x + f - x'Qx / 2    s.t.  A x <= b,  x >= 0      (Q PSD)

The iteration is intpt.c's (start: every variable 1000; delta = 0.02,
r = 0.9; the same stop and give-up tests on the single-precision printed
quantities) with Q carried through:

    rho = b - A x - w            sigma = c - A'y + z - Q x
    pobj = c'x - x'Qx / 2 + f    dobj = b'y + x'Qx / 2 + f     gamma = z'x + y'w
    -E dy + A dx = rho + w - mu / y,   A'dy + (D + Q) dx = sigma - z + mu / x
    dz = mu / x - z - D dx,  dw = mu / y - w - E dy            (D = z / x, E = w / y)

Everything but the linear solve is fp64 NumPy.  Two back ends solve the
Newton system:

  "dense"   the (m + n)^2 matrix, solved to extended precision: an fp64 LU
            (scipy) refined against the residual formed in np.longdouble
            (numpy.linalg has no long-double solve; three refinement passes
            bring the fp64 LU's solution to the long-double residual's
            accuracy while cond(K) eps64 < 1).  For the small synthetic cases.
  "oracle"  oracle_lib.OracleKkt on the swapped form (A' for A, E' = D,
            D' = E, Q on its first block, qmax = 1; fy' = -fx, fx' = fy,
            dx = dy', dy = -dx'): the reference's ldlt.c restated with Q,
            pinned by tests/test_qp.py and tests/test_gpu_qp.py.  For
            netlib-sized patterns.
"""
import functools

import numpy as np
import scipy.linalg
import scipy.sparse as sp

import ipo_amd
from test_qp import random_q

assert np.finfo(np.longdouble).eps < 2e-19, "np.longdouble is not an extended-precision type on this platform"
LD = np.longdouble

DELTA, R = 0.02, 0.9


# ---------------------------------------------------------------- problems
def csc_of(M):
    """(k, i, v) of a dense matrix's nonzeros, rows ascending in each column."""
    M = np.asarray(M)
    k = np.zeros(M.shape[1] + 1, np.int32)
    ii, vv = [], []
    for j in range(M.shape[1]):
        r = np.nonzero(M[:, j])[0]
        ii.append(r)
        vv.append(M[r, j])
        k[j + 1] = k[j] + r.size
    return k, np.concatenate(ii).astype(np.int32), np.concatenate(vv).astype(np.float64)


def q_dense(n, q):
    M = np.zeros((n, n))
    if q is not None:
        kQ, iQ, Q = q
        for j in range(n):
            M[iQ[kQ[j]:kQ[j + 1]], j] = Q[kQ[j]:kQ[j + 1]]
    return M


Q_KINDS = ("diag", "banded", "lowrank", "gaps")


def make_q(n, kind, seed):
    """diag: a diagonal in U[0.1, 2]; banded: test_qp.random_q (off-diagonal
    entries: the KKT graph is no longer bipartite); lowrank: F F', F n x 2
    (singular PSD, every entry stored); gaps: random_q on every other
    column, the rest of Q's columns empty."""
    rng = np.random.default_rng([seed, n, Q_KINDS.index(kind)])
    if kind == "diag":
        return csc_of(np.diag(rng.uniform(0.1, 2.0, n)))
    if kind == "banded":
        return random_q(n, seed)
    if kind == "lowrank":
        F = rng.uniform(-1.0, 1.0, (n, 2))
        M = np.triu(F @ F.T)
        return csc_of(M + np.triu(M, 1).T)          # mirrored: symmetric bit for bit
    if kind == "gaps":
        sub = np.arange(0, n, 2)
        M = np.zeros((n, n))
        M[np.ix_(sub, sub)] = q_dense(sub.size, random_q(sub.size, seed))
        return csc_of(M)
    raise ValueError(kind)


def make_qp(m, n, kind, seed):
    """A QP that is feasible and bounded by construction from an interior
    point (as ipo_hip_synth_random's LPs): row 0 of A all positive (x >= 0 is
    bounded), every other row with an entry at column i % n, two more random
    entries per column; x*, z*, y*, w* in U[0.5, 1.5], b = A x* + w*,
    c = A'y* - z* + Q x*."""
    rng = np.random.default_rng([seed, m, n])
    M = np.zeros((m, n))
    M[0, :] = rng.uniform(0.5, 1.5, n)
    for i in range(1, m):
        M[i, i % n] = rng.uniform(0.5, 1.5) * rng.choice([-1.0, 1.0])
    if m > 1:
        for j in range(n):
            for i in rng.integers(1, m, 2):
                M[i, j] = rng.uniform(0.5, 1.5) * rng.choice([-1.0, 1.0])
    q = make_q(n, kind, seed)
    xs, zs = rng.uniform(0.5, 1.5, n), rng.uniform(0.5, 1.5, n)
    ys, ws = rng.uniform(0.5, 1.5, m), rng.uniform(0.5, 1.5, m)
    b = M @ xs + ws
    c = M.T @ ys - zs + q_dense(n, q) @ xs
    kA, iA, A = csc_of(M)
    return ipo_amd.SolverForm(m, n, kA, iA, A, b, c, 0.0, q=q)


def budget_projection():
    """max a'x - x'x / 2, sum x <= 1, x >= 0 with a = (1.5, -2, 0, 3, -0.5):
    closed form x = e_4, y = 2 (objective 2.5)."""
    a = np.array([1.5, -2.0, 0.0, 3.0, -0.5])
    kA, iA, A = csc_of(np.ones((1, 5)))
    return ipo_amd.SolverForm(1, 5, kA, iA, A, np.array([1.0]), a, 0.0, q=csc_of(np.eye(5)))


SHAPES = ((3, 5), (20, 30), (63, 65), (40, 200), (200, 40))     # m x n


def with_q(p, q):
    return ipo_amd.SolverForm(p.m, p.n, p.kA, p.iA, p.A, p.b, p.c, p.f, q=q)


# ---------------------------------------------------------------- the iteration
def _mats(p):
    A = sp.csc_matrix((p.A, p.iA, p.kA), shape=(p.m, p.n))
    q = getattr(p, "q", None)
    Q = sp.csc_matrix((q[2], q[1], q[0]), shape=(p.n, p.n)) if q is not None and len(q[2]) else None
    return A, Q


class _Dense:
    def __init__(self, p):
        self.m, self.n = p.m, p.n
        A, Q = _mats(p)
        T = p.m + p.n
        self.K = np.zeros((T, T))
        self.K[:p.m, p.m:] = A.toarray()
        self.K[p.m:, :p.m] = A.toarray().T
        self.Qd = Q.toarray() if Q is not None else np.zeros((p.n, p.n))

    def solve(self, E, D, fy, fx):
        m = self.m
        K = self.K.copy()
        K[m:, m:] = self.Qd
        K[np.arange(m), np.arange(m)] = -E
        K[m:, m:][np.diag_indices(self.n)] += D
        rhs = np.concatenate([fy, fx]).astype(LD)
        Kl = K.astype(LD)
        lu = scipy.linalg.lu_factor(K)
        s = scipy.linalg.lu_solve(lu, rhs.astype(np.float64)).astype(LD)
        for _ in range(3):
            s += scipy.linalg.lu_solve(lu, (rhs - Kl @ s).astype(np.float64)).astype(LD)
        s = s.astype(np.float64)
        return s[:m], s[m:]


class _Oracle:
    def __init__(self, p):
        import oracle_lib
        kAt, iAt, At = p.transpose()
        sw = ipo_amd.SolverForm(p.n, p.m, kAt, iAt, At, p.c, p.b, 0.0)
        q = getattr(p, "q", None)
        self.k = oracle_lib.OracleKkt(sw, q=q if q is not None and len(q[2]) else None, qmax=1)

    def solve(self, E, D, fy, fx):
        self.k.factor(D, E)
        dyp, dxp, _ = self.k.solve(D, E, -fx, fy)
        return -dxp, dyp


def solve_qp(p, backend="dense", max_iter=200, shuffle=None, giveup=True):
    """The iteration of the module docstring.  Returns dict(status, iters,
    rows, x, y, w, z, growth): rows[k] = (k, pobj, normr, dobj, norms), the
    line method "qp" prints at iteration k (single precision, as
    intpt.c:47); growth = the largest normr / normr0 or norms / norms0 any
    iteration saw (the give-up tests fire above 10); floor = the residual the
    refined solve of ldlt.c:367-416 may leave in the last Newton system,
    1e-10 (max |right-hand side| + 1), entry by entry: what the next
    iteration's rho and sigma inherit from it.
    giveup=False: without intpt's two give-up tests (the iteration runs to
    its stop rule), for a problem on which they fire on rounding noise.
    shuffle = a seed: A x, A'y and Q x summed in a random order of their
    terms -- the same iteration under another rounding (STABLE_GROWTH)."""
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
    lin = _Dense(p) if backend == "dense" else _Oracle(p)
    x, z = np.full(n, 1000.0), np.full(n, 1000.0)
    y, w = np.full(m, 1000.0), np.full(m, 1000.0)
    normr0 = norms0 = np.inf
    rows, status, growth, floor = [], 5, 0.0, 0.0
    f32 = lambda v: float(np.float32(v))     # noqa: E731
    for it in range(max_iter):
        rho = b - ax(x) - w
        qx = qxf(x)
        sig = ((c - aty(y)) + z) - qx
        normr, norms = f32(np.sqrt(rho @ rho)), f32(np.sqrt(sig @ sig))
        gamma = z @ x + y @ w
        hxqx = 0.5 * (x @ qx)
        pobj, dobj = f32(c @ x - hxqx + f), f32(b @ y + hxqx + f)
        rows.append((it, pobj, normr, dobj, norms))
        if normr < 1.0e-6 and norms < 1.0e-6 and gamma < 1.0e-6:
            status = 0
            break
        growth = max(growth, normr / normr0 if normr0 > 0 else np.inf if normr > 0 else 0.0,
                     norms / norms0 if norms0 > 0 else np.inf if norms > 0 else 0.0)
        if giveup and normr > 10 * normr0:
            status = 2
            break
        if giveup and norms > 10 * norms0:
            status = 4
            break
        mu = DELTA * gamma / (n + m)
        D, E = z / x, w / y
        fy, fx = rho + w - mu / y, sig - z + mu / x
        floor = 1.0e-10 * (max(np.abs(fy).max(), np.abs(fx).max()) + 1.0)
        dy, dx = lin.solve(E, D, fy, fx)
        dz = mu / x - z - D * dx
        dw = mu / y - w - E * dy
        theta = max(0.0, np.max(-dx / x), np.max(-dz / z), np.max(-dy / y), np.max(-dw / w))
        theta = 1.0 if theta == 0.0 or R / theta > 1.0 else R / theta
        x, z, y, w = x + theta * dx, z + theta * dz, y + theta * dy, w + theta * dw
        normr0, norms0 = normr, norms
    return dict(status=status, iters=len(rows), rows=rows, x=x, y=y, w=w, z=z, growth=growth, floor=floor)


@functools.lru_cache(maxsize=None)
def reference(key, make, backend):
    """(problem, its reference run) of make(*key), computed once per process
    and shared, read-only, by the tests that need it."""
    p = make(*key)
    return p, solve_qp(p, backend)


# ---------------------------------------------------------------- checks
def certificate(p, x, y, w, z):
    """The optimality conditions recomputed in fp64, independent of the
    method: (||b - Ax - w||_2, ||c - A'y + z - Qx||_2, z'x + y'w, min entry)."""
    A, Q = _mats(p)
    qx = Q @ x if Q is not None else 0.0
    rp = np.asarray(p.b) - A @ x - w
    rd = np.asarray(p.c) - A.T @ y + z - qx
    return (float(np.sqrt(rp @ rp)), float(np.sqrt(rd @ rd)), float(z @ x + y @ w),
            float(min(x.min(), y.min(), w.min(), z.min())))


def objective(p, x):
    """c'x + f - x'Qx / 2"""
    A, Q = _mats(p)
    return float(np.asarray(p.c) @ x + p.f - (0.5 * (x @ (Q @ x)) if Q is not None else 0.0))
