"""Small synthetic LPs whose dense tail, or whose sparse supernodes, have a
chosen size, and an extended-precision LDL' of their KKT matrix (numpy only;
a plain module, no fixtures).

K = [[-diag(E), A], [A', diag(D)]], y-nodes first -- the numbering perm()
speaks of (perm[new] = old).  The reference factors K[perm][:, perm]
right-looking in np.longdouble (x86-64: 64-bit mantissa, eps 1.08e-19), with
no pivoting and no zero test, and solves with it; it is what both the fp64
oracle (oracle/orc_kkt.c) and the device factor are measured against in
tests/test_tail_shapes.py and tests/test_gpu_tail_shapes.py, and in
tests/test_sparse_shapes.py and tests/test_gpu_sparse_shapes.py.
"""
import functools

import numpy as np

import ipo_amd

# the reference has to be worth more than the fp64 factors it judges: fail
# (not skip) where long double is double
assert np.finfo(np.longdouble).eps < 2e-19, "np.longdouble is not an extended-precision type on this platform"

LD = np.longdouble


def _finish(m, n, kA, iA, A, rng):
    """b = A xs + ws, c = A' ys - zs for an interior point (synth.cpp's
    interior_point), so that the pattern is also a feasible, bounded LP."""
    xs, ws = rng.uniform(0.5, 2.0, n), rng.uniform(0.5, 2.0, m)
    ys, zs = rng.uniform(0.5, 2.0, m), rng.uniform(0.5, 2.0, n)
    b, c = ws.copy(), -zs
    for j in range(n):
        k0, k1 = kA[j], kA[j + 1]
        b[iA[k0:k1]] += A[k0:k1] * xs[j]
        c[j] += A[k0:k1] @ ys[iA[k0:k1]]
    return ipo_amd.SolverForm(m, n, kA, iA, A, b, c, 0.0)


def dense_lp(m, n, seed):
    """Every one of A's m n entries stored: uniform(0.5, 1.5) times a random sign."""
    rng = np.random.default_rng(seed)
    V = rng.uniform(0.5, 1.5, (m, n)) * rng.choice([-1.0, 1.0], (m, n))
    kA = (np.arange(n + 1) * m).astype(np.int32)
    iA = np.tile(np.arange(m, dtype=np.int32), n)
    A = np.ascontiguousarray(V.T).reshape(-1)
    return _finish(m, n, kA, iA, A, rng)


def rows_lp(m, n, r, seed):
    """A sparse part of ms = m - r rows and r dense rows: column j has entries
    in rows ((j ms) // n + k) % ms, k = 0, 1, 2 (uniform(0.5, 1.5)) and one in
    each of rows ms .. m-1 (uniform(-1.5, 1.5))."""
    ms = m - r
    assert ms >= 3 and r >= 0
    rng = np.random.default_rng(seed)
    per = 3 + r
    kA = (np.arange(n + 1) * per).astype(np.int32)
    iA = np.zeros(n * per, np.int32)
    A = np.zeros(n * per)
    dense_rows = np.arange(ms, m, dtype=np.int32)
    for j in range(n):
        rows = np.array([((j * ms) // n + k) % ms for k in range(3)], np.int32)
        vals = rng.uniform(0.5, 1.5, 3)
        o = np.argsort(rows)
        iA[j * per:j * per + 3] = rows[o]
        A[j * per:j * per + 3] = vals[o]
        iA[j * per + 3:(j + 1) * per] = dense_rows
        A[j * per + 3:(j + 1) * per] = rng.uniform(-1.5, 1.5, r)
    return _finish(m, n, kA, iA, A, rng)


def blocks_lp(blocks, r, seed):
    """A block diagonal of dense m_i x n_i blocks, blocks = ((m_i, n_i), ...),
    over r dense linking rows, which come last: column j of block i stores
    rows [row0_i, row0_i + m_i) and rows [m - r, m); values as in dense_lp.
    Minimum degree turns the side of a block with the lower degree into
    single-column leaves and the other side into one supernode per block;
    the linking rows end on top (tests/test_sparse_shapes.py pins what each
    (blocks, r) realises)."""
    rng = np.random.default_rng(seed)
    ms = sum(mi for mi, _ in blocks)
    m, n = ms + r, sum(ni for _, ni in blocks)
    link = np.arange(ms, m, dtype=np.int32)
    kA, iA, A = [0], [], []
    row0 = 0
    for mi, ni in blocks:
        V = rng.uniform(0.5, 1.5, (ni, mi + r)) * rng.choice([-1.0, 1.0], (ni, mi + r))
        rows = np.concatenate([np.arange(row0, row0 + mi, dtype=np.int32), link])
        for j in range(ni):
            iA.append(rows)
            A.append(V[j])
            kA.append(kA[-1] + mi + r)
        row0 += mi
    return _finish(m, n, np.array(kA, np.int32), np.concatenate(iA).astype(np.int32), np.concatenate(A), rng)


def make_lp(family, shape, seed):
    if family == "blocks":
        return blocks_lp(*shape, seed)
    return dense_lp(*shape, seed) if family == "dense" else rows_lp(*shape, seed)


def scaling(p, kind, seed):
    """(E, D, fy, fx): kind "unit": E, D ~ U(0.1, 10), the suite's usual
    inputs; "wide": log-uniform in [1e-6, 1e6], the spread of an interior-point
    iteration.  fy, fx ~ U(-1, 1)."""
    rng = np.random.default_rng(seed)
    if kind == "unit":
        E, D = rng.uniform(0.1, 10.0, p.m), rng.uniform(0.1, 10.0, p.n)
    elif kind == "wide":
        E, D = 10.0 ** rng.uniform(-6.0, 6.0, p.m), 10.0 ** rng.uniform(-6.0, 6.0, p.n)
    else:
        raise ValueError(kind)
    return E, D, rng.uniform(-1, 1, p.m), rng.uniform(-1, 1, p.n)


def kkt_dense(p, E, D):
    """The (m + n)^2 matrix [[-diag(E), A], [A', diag(D)]] in fp64 (its entries are the inputs, exact)."""
    T = p.m + p.n
    K = np.zeros((T, T))
    cols = np.repeat(np.arange(p.n), np.diff(p.kA))
    K[p.iA, p.m + cols] = p.A
    K[p.m + cols, p.iA] = p.A
    K[np.arange(p.m), np.arange(p.m)] = -np.asarray(E)
    K[p.m + np.arange(p.n), p.m + np.arange(p.n)] = np.asarray(D)
    return K


def ldl_ref(K, perm):
    """Right-looking LDL' of K[perm][:, perm] in long double, no pivoting, no
    zero test: (L unit lower, d)."""
    perm = np.asarray(perm)
    S = K[np.ix_(perm, perm)].astype(LD)
    T = S.shape[0]
    L = np.eye(T, dtype=LD)
    d = np.zeros(T, LD)
    B = 64      # the trailing update by column strips from their diagonal down: the lower triangle only
    for j in range(T):
        d[j] = S[j, j]
        a = S[j + 1:, j].copy()
        l = a / d[j]
        L[j + 1:, j] = l
        for c in range(j + 1, T, B):
            k = c - (j + 1)
            S[c:, c:c + B] -= np.outer(l[k:], a[k:k + B])
    return L, d


def solve_ref(L, d, perm, fy, fx):
    """K (y, x) = (fy, fx) through the reference factor, in long double."""
    perm = np.asarray(perm)
    m = len(fy)
    z = np.concatenate([np.asarray(fy), np.asarray(fx)]).astype(LD)[perm]
    T = z.size
    for j in range(T - 1):
        z[j + 1:] -= L[j + 1:, j] * z[j]
    z /= d
    for j in range(T - 2, -1, -1):
        z[j] -= L[j + 1:, j] @ z[j + 1:]
    out = np.zeros(T, LD)
    out[perm] = z
    return out[:m], out[m:]


class Case:
    """One (family, shape, seed, scaling): the LP, its K(E, D), a right-hand
    side, the reference order and the long-double pivots and solution."""

    def __init__(self, family, shape, seed, kind):
        self.family, self.shape, self.seed, self.kind = family, shape, seed, kind
        self.p = p = make_lp(family, shape, seed)
        self.E, self.D, self.fy, self.fx = scaling(p, kind, seed + 1)
        # the reference's ordering (host only; what perm() of a device factor returns)
        self.perm = ipo_amd.symbolic(p.m, p.n, p.kA, p.iA)["perm"]
        L, d = ldl_ref(kkt_dense(p, self.E, self.D), self.perm)
        self.d = d
        self.y, self.x = solve_ref(L, d, self.perm, self.fy, self.fx)

    def pivot_distance(self, d):
        """max |d - d_ref| / |d_ref|"""
        return float(np.max(np.abs(np.asarray(d).astype(LD) - self.d) / np.abs(self.d)))

    def solution_distance(self, y, x):
        """||(y, x) - ref||_inf / (1 + ||ref||_inf)"""
        ref = np.concatenate([self.y, self.x])
        got = np.concatenate([np.asarray(y), np.asarray(x)]).astype(LD)
        return float(np.max(np.abs(got - ref)) / (1 + np.max(np.abs(ref))))


@functools.lru_cache(maxsize=None)
def case(family, shape, seed, kind):
    """The Case of (family, shape, seed, scaling), computed once per process
    (0.1 s at T = 262, 1 s at 648, 2.4 s at 860) and shared, read-only, by
    every path variant."""
    return Case(family, tuple(shape), seed, kind)
