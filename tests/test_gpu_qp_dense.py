"""Long columns of Q on the GPU: a column of at least IPO_HIP_Q_LONG entries
(default kLongQCol = 256) is summed by one wave (csrc/dev_common.hip
k_q_long) instead of one thread's sparse_dot, in the QP residual
(k_qp_residuals) and in the KKT refinement's residual (kkt_residual_body).

1. ipo_amd.q_times against a NumPy restatement of the wave's order, bit for
   bit: lane l sums the products p[l::64] serially from 0.0, then
   s[:o] = s[:o] + s[o:2o] for o = 32, 16, 8, 4, 2, 1, and the result is s[0].
   Columns below the threshold equal the serial in-order sum, bit for bit.
   The kernel's load batch spans 256 entries (kQLongSteps = 4 steps of 64).
2. The KKT factor with a dense and an arrow Q on the y-nodes against the
   oracle, at the bars of test_gpu_qp.py::test_kkt_with_q_matches_oracle,
   with the wave path and (IPO_HIP_Q_LONG=0) without it.
3. Method "qp" on qp_dense's cases (conditions: tests/test_qp_dense.py) at
   the bars of test_gpu_qp_solver.py, and on three of its own small cases
   with every nonempty column forced onto the wave path (IPO_HIP_Q_LONG=1).
"""
import numpy as np
import pytest

import ipo_amd
import oracle_lib
import qp_dense
import qp_ref
from test_gpu_qp import _inputs, qp_residual
from test_gpu_qp_solver import check_against, check_certificate
from test_qp_solver import small_problem

pytestmark = pytest.mark.gpu

LONG_Q_COL = 256      # csrc/kkt_knobs.h kLongQCol

# a partly filled wave, the threshold on both sides, multiples of 64 and of
# the 256-entry load batch on both sides, many batches
EDGE_LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 4097)


# ---------------------------------------------------------------- 1. q_times
def serial_order(p):
    s = 0.0
    for t in p.tolist():
        s += t
    return s


def wave_order(p):
    s = np.zeros(64)
    for lane in range(64):
        acc = 0.0
        for t in p[lane::64].tolist():
            acc += t
        s[lane] = acc
    for o in (32, 16, 8, 4, 2, 1):
        s[:o] = s[:o] + s[o:2 * o]
    return s[0]


def columns_matrix(n, lengths, seed):
    """n x n CSC (not symmetric) with lengths[j] entries in column j, rows
    ascending; values over 40 binades with zeros and -0.0, as test_gpu_dot.py,
    so that another order of the adds gives other bits."""
    rng = np.random.default_rng(seed)
    kQ = np.zeros(n + 1, np.int32)
    kQ[1:] = np.cumsum(lengths)
    iQ = np.concatenate([np.sort(rng.choice(n, ln, replace=False)) for ln in lengths] + [np.zeros(0, np.int64)])
    nz = int(kQ[-1])
    Q = rng.standard_normal(nz) * 2.0 ** rng.uniform(-20, 20, nz)
    Q[rng.uniform(size=nz) < 0.05] = 0.0
    Q[rng.uniform(size=nz) < 0.02] = -0.0
    v = rng.standard_normal(n)
    v[rng.uniform(size=n) < 0.03] = 0.0
    v[rng.uniform(size=n) < 0.03] = -0.0
    return (kQ, iQ.astype(np.int32), Q), v


def expected(q, v, long_min):
    kQ, iQ, Q = q
    out = np.zeros(kQ.size - 1)
    for j in range(kQ.size - 1):
        p = Q[kQ[j]:kQ[j + 1]] * v[iQ[kQ[j]:kQ[j + 1]]]
        out[j] = wave_order(p) if long_min > 0 and p.size >= long_min else serial_order(p)
    return out


def assert_same_bits(got, want, lengths):
    bad = np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0]
    assert bad.size == 0, [(int(j), int(lengths[j]), got[j], want[j]) for j in bad[:8]]


def edge_layout():
    """Every EDGE_LENGTHS column twice, long ones at j = 0, in the middle and at
    j = n - 1, columns of 0-20 entries between them."""
    n = 4200
    rng = np.random.default_rng(5)
    lengths = rng.integers(0, 21, n)
    lengths[0] = 4097
    lengths[n - 1] = 513
    lengths[7:7 + 20 * len(EDGE_LENGTHS):20] = EDGE_LENGTHS
    lengths[n // 2:n // 2 + len(EDGE_LENGTHS)] = EDGE_LENGTHS[::-1]      # adjacent long columns: whole blocks of four waves
    return n, lengths


@pytest.fixture(scope="module")
def edge_case():
    n, lengths = edge_layout()
    q, v = columns_matrix(n, lengths, 11)
    return q, v, lengths


def test_q_times_threshold_256(edge_case, monkeypatch):
    q, v, lengths = edge_case
    monkeypatch.delenv("IPO_HIP_Q_LONG", raising=False)
    want = expected(q, v, LONG_Q_COL)
    assert_same_bits(ipo_amd.q_times(q, v, LONG_Q_COL), want, lengths)
    assert_same_bits(ipo_amd.q_times(q, v), want, lengths)               # the knob's default
    # the two orders differ on these inputs: the comparison can tell them apart
    assert np.any(want.view(np.uint64) != expected(q, v, 0).view(np.uint64))


def test_q_times_every_column_by_waves(edge_case):
    q, v, lengths = edge_case
    assert_same_bits(ipo_amd.q_times(q, v, 1), expected(q, v, 1), lengths)


def test_q_times_knob_zero_is_serial(edge_case, monkeypatch):
    q, v, lengths = edge_case
    monkeypatch.setenv("IPO_HIP_Q_LONG", "0")
    assert_same_bits(ipo_amd.q_times(q, v, 0), expected(q, v, 0), lengths)


@pytest.mark.parametrize("nlong", [1, 3, 4, 5])
def test_q_times_long_column_counts(nlong):
    """Blocks of four waves, partly filled; the long columns at j = 0, in the
    middle and at j = n - 1, short ones between."""
    n = 700
    rng = np.random.default_rng(nlong)
    lengths = rng.integers(0, 40, n)
    at = [0, n - 1, n // 2, n // 3, 5][:nlong] if nlong > 1 else [n // 2]
    for t, j in enumerate(at):
        lengths[j] = (256, 700, 449, 257, 512)[t]
    q, v = columns_matrix(n, lengths, 100 + nlong)
    assert int((lengths >= LONG_Q_COL).sum()) == nlong
    assert_same_bits(ipo_amd.q_times(q, v, LONG_Q_COL), expected(q, v, LONG_Q_COL), lengths)


def test_q_times_refuses_bad_input():
    q, v = columns_matrix(8, np.full(8, 3), 0)
    bad = q[1].copy()
    bad[4] = 8
    with pytest.raises(ipo_amd.IpoHipError, match="out of range"):
        ipo_amd.q_times((q[0], bad, q[2]), v)
    badk = q[0].copy()
    badk[3] = 1
    with pytest.raises(ipo_amd.IpoHipError, match="decreasing"):
        ipo_amd.q_times((badk, q[1], q[2]), v)


# ---------------------------------------------------------------- 2. the KKT factor
@pytest.fixture(scope="module")
def kkt_problem():
    return ipo_amd.synth_random(320, 1500, 4, 64)


@pytest.mark.parametrize("knob,kind,qmax", [(k, kind, qm) for k in (None, "0") for kind in qp_dense.DENSE_KINDS
                                            for qm in (1, -1)])
def test_kkt_with_long_q_matches_oracle(kkt_problem, monkeypatch, knob, kind, qmax):
    p = kkt_problem
    if knob is None:
        monkeypatch.delenv("IPO_HIP_Q_LONG", raising=False)
    else:
        monkeypatch.setenv("IPO_HIP_Q_LONG", knob)
    q = qp_dense.make_q_dense(p.m, kind, 0)
    E, D, fy, fx = _inputs(p, 20251121)
    if qmax < 0:
        E = E + np.abs(qp_ref.q_dense(p.m, q)).sum(0).max()     # keep -E + Q negative definite (quasi-definite K)
    gpu = ipo_amd.KktFactor(p.m, p.n, p.kA, p.iA, p.A, q=q, qmax=qmax)
    orc = oracle_lib.OracleKkt(p, q=q, qmax=qmax)
    try:
        assert gpu.q_long() == (0 if knob == "0" else p.m if kind == "factor" else 3)
        assert np.array_equal(gpu.perm(), orc.perm())
        gpu.factor(E, D)
        orc.factor(E, D)
        gd, glive = gpu.pivots()
        od = orc.diag()
        assert np.array_equal(glive, orc.live()) and gpu.info()["ndep"] == orc.info()["ndep"] == 0
        print(f"pivots: worst relative distance {np.abs((gd - od) / od).max():.3e}")
        assert (np.abs(gd - od) <= 1e-9 * np.abs(od)).all()
        gy, gx, ok = gpu.solve(E, D, fy, fx)
        oy, ox, _ = orc.solve(E, D, fy, fx)
        assert ok == 1
        scale = 1.0 + max(np.abs(oy).max(), np.abs(ox).max())
        bc = max(np.abs(fy).max(), np.abs(fx).max()) + 1
        res = qp_residual(p, q, qmax, E, D, fy, fx, gy, gx)
        print(f"solution: {np.abs(gy - oy).max() / scale:.3e} {np.abs(gx - ox).max() / scale:.3e} of its scale; "
              f"residual {res / bc:.3e} of bc; passes {gpu.info()['passes']}")
        assert np.abs(gy - oy).max() <= 1e-8 * scale and np.abs(gx - ox).max() <= 1e-8 * scale
        assert res <= 1e-9 * bc
    finally:
        gpu.close()


def test_kkt_without_q_has_no_long_column(kkt_problem):
    p = kkt_problem
    gpu = ipo_amd.KktFactor(p.m, p.n, p.kA, p.iA, p.A)
    try:
        assert gpu.q_long() == 0
    finally:
        gpu.close()


# ---------------------------------------------------------------- 3. solves
def ctx_q_long(p):
    ctx = ipo_amd.Context(p)
    try:
        return ctx.q_long()
    finally:
        ctx.close()


@pytest.mark.parametrize("m,n,kind", sorted(qp_dense.DENSE_SEEDS))
def test_dense_cases_match_reference(monkeypatch, m, n, kind):
    monkeypatch.delenv("IPO_HIP_Q_LONG", raising=False)
    p, ref = qp_ref.reference((m, n, kind), qp_dense.dense_problem, "dense")
    assert ctx_q_long(p) == (n if kind == "factor" else 3)
    out = ipo_amd.solver(p, method="qp", trace=True)
    check_against(ref, out)
    check_certificate(p, out["x"], out["y"], out["w"], out["z"])


@pytest.mark.parametrize("m,n,kind", [(63, 65, "lowrank"), (63, 65, "gaps"), (20, 30, "banded")])
def test_wave_path_on_short_columns(monkeypatch, m, n, kind):
    """IPO_HIP_Q_LONG=1: columns shorter than a wave, and empty ones (never long)."""
    monkeypatch.setenv("IPO_HIP_Q_LONG", "1")
    p, ref = qp_ref.reference((m, n, kind), small_problem, "dense")
    lens = qp_dense.column_lengths(p.q)
    assert ctx_q_long(p) == int((lens > 0).sum())
    if kind == "gaps":
        assert int((lens == 0).sum()) > 0
    out = ipo_amd.solver(p, method="qp", trace=True)
    check_against(ref, out)
    check_certificate(p, out["x"], out["y"], out["w"], out["z"])


def test_two_runs_on_one_dense_context_identical(monkeypatch):
    monkeypatch.delenv("IPO_HIP_Q_LONG", raising=False)
    p, _ = qp_ref.reference((300, 257, "factor"), qp_dense.dense_problem, "dense")
    ctx = ipo_amd.Context(p)
    try:
        assert ctx.q_long() == 257
        st1, s1, _ = ctx.run("qp")
        a = ctx.solution()
        st2, s2, _ = ctx.run("qp")
        b = ctx.solution()
    finally:
        ctx.close()
    assert st1 == st2 == 0 and s1["iters"] == s2["iters"]
    for u, v in zip(a, b):
        assert np.array_equal(u, v)


def test_existing_longest_column_stays_serial(monkeypatch):
    """(40, 240, lowrank): the longest column of Q any earlier test builds,
    below the default threshold."""
    monkeypatch.delenv("IPO_HIP_Q_LONG", raising=False)
    p = small_problem(40, 240, "lowrank")
    assert int(qp_dense.column_lengths(p.q).max()) == 240
    assert ctx_q_long(p) == 0
