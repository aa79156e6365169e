"""The index maps Context.update() refreshes a context's value arrays through
(ipo_hip_value_maps; csrc/value_maps.cpp), on the host: every derived copy of
a value array is the caller's array gathered through one of them, so a map
that is right makes the refresh right.  Without a GPU.

  "csr"    A[map] is the CSR's value array (SolverForm.transpose) and the map
           is a permutation
  "jds"    the RowAxPlan slices gathered through the map give A x, exactly,
           on small-integer data, and every entry of A is used once
  "qt"     an involution that fixes the diagonal entries and sends (i, j) to (j, i)
  "qdiag"  exactly the diagonal entries
"""
import numpy as np
import pytest

import ipo_amd
import qp_ref
from conftest import mps_path
from test_abi import declared_functions

NEW_ENTRIES = ("ipo_hip_ctx_update", "ipo_hip_ctx_update_seconds", "ipo_hip_ctx_set_start",
               "ipo_hip_ctx_start_from_last", "ipo_hip_value_maps")


def pattern(m, n, seed, density=0.3, empty=False):
    """A random m x n pattern with integer values; empty: row 1 and column 2 without entries."""
    rng = np.random.default_rng([seed, m, n])
    M = (rng.uniform(size=(m, n)) < density) * rng.integers(1, 8, (m, n)) * rng.choice([-1, 1], (m, n))
    M[0, 0] = 3                       # never an empty matrix
    if empty:
        M[1, :] = 0
        M[:, 2] = 0
    kA, iA, A = qp_ref.csc_of(M.astype(np.float64))
    return ipo_amd.SolverForm(m, n, kA, iA, A, np.zeros(m), np.zeros(n), 0.0), M


def shapes():
    out = {"1x1": pattern(1, 1, 0)[0], "1x64": pattern(1, 64, 1, 0.9)[0], "63x65": pattern(63, 65, 2)[0],
           "empty row and column": pattern(7, 9, 3, 0.5, empty=True)[0]}
    return out


SHAPES = ("1x1", "1x64", "63x65", "empty row and column", "afiro")


def problem(name):
    return ipo_amd.load_mps(mps_path("afiro")) if name == "afiro" else shapes()[name]


@pytest.mark.parametrize("name", SHAPES)
def test_csr_map(name):
    p = problem(name)
    mp = ipo_amd.value_maps(p.m, p.n, p.kA, p.iA, "csr")
    kAt, iAt, At = p.transpose()
    assert mp.size == p.nz and np.array_equal(np.sort(mp), np.arange(p.nz))
    vals = np.arange(p.nz, dtype=np.float64) + 0.5          # every entry told apart
    q = ipo_amd.SolverForm(p.m, p.n, p.kA, p.iA, vals, p.b, p.c, 0.0)
    assert np.array_equal(vals[mp], q.transpose()[2]) and np.array_equal(p.A[mp], At)
    # and the columns the CSR lists are those entries' columns
    cols = np.repeat(np.arange(p.n), np.diff(p.kA))
    assert np.array_equal(cols[mp], iAt)


def jds_product(p, vals, x, maps):
    """k_rows_ax_jds's sums (dev_common.hip) on the layout's arrays, pass by pass."""
    dims = maps["jds.dims"]
    npass, ax = int(dims[0]), np.full(p.m, np.nan)
    for ps in range(npass):
        rows, nd, dbase = (int(v) for v in dims[1 + 3 * ps:4 + 3 * ps])
        for r in range(rows):
            i = maps["jds.perm"][ps * p.m + r]
            s = 0.0 if ps == 0 else ax[i]
            for k in range(nd):
                if r >= maps["jds.dlen"][dbase + k]:
                    break
                q = maps["jds.dptr"][dbase + k] + r
                s += vals[q] * x[maps["jds.cols"][q]]
            ax[i] = s
    return ax


@pytest.mark.parametrize("blocks", ["1", "3"])
@pytest.mark.parametrize("name", SHAPES)
def test_jds_map(monkeypatch, name, blocks):
    monkeypatch.setenv("IPO_HIP_AX_JDS", "1")
    monkeypatch.setenv("IPO_HIP_AX_BLOCKS", blocks)
    p = problem(name)
    maps = {k: ipo_amd.value_maps(p.m, p.n, p.kA, p.iA, k)
            for k in ("jds", "jds.cols", "jds.perm", "jds.dptr", "jds.dlen", "jds.dims")}
    mp = maps["jds"]
    assert int(maps["jds.dims"][0]) == int(blocks)
    assert mp.size == p.nz and np.array_equal(np.sort(mp), np.arange(p.nz))       # every entry once
    cols = np.repeat(np.arange(p.n), np.diff(p.kA))
    assert np.array_equal(cols[mp], maps["jds.cols"])
    # small integers: every product and partial sum is exact, so the order of the sums does not show
    rng = np.random.default_rng(5)
    A = rng.integers(-7, 8, p.nz).astype(np.float64)
    x = rng.integers(-5, 6, p.n).astype(np.float64)
    kAt, iAt, At = ipo_amd.SolverForm(p.m, p.n, p.kA, p.iA, A, p.b, p.c, 0.0).transpose()
    want = np.array([At[kAt[i]:kAt[i + 1]] @ x[iAt[kAt[i]:kAt[i + 1]]] for i in range(p.m)])
    assert np.array_equal(jds_product(p, A[mp], x, maps), want)


def q_patterns():
    gaps = qp_ref.make_q(9, "gaps", 4)
    dense = qp_ref.csc_of(np.arange(1.0, 26.0).reshape(5, 5) + np.arange(1.0, 26.0).reshape(5, 5).T)
    banded = qp_ref.make_q(30, "banded", 1)
    nodiag = qp_ref.csc_of(np.array([[0.0, 1.0, 0.0], [1.0, 2.0, 0.0], [0.0, 0.0, 0.0]]))
    # rows descending in every column: the maps' general path (a context refuses such a Q; the maps do not)
    kQ, iQ, Q = banded
    rev = np.concatenate([np.arange(kQ[j], kQ[j + 1])[::-1] for j in range(kQ.size - 1)])
    return {"gaps": gaps, "dense 5x5": dense, "banded": banded, "no diagonal in column 0": nodiag,
            "banded, rows descending": (kQ, iQ[rev], Q[rev])}


@pytest.mark.parametrize("name", sorted(q_patterns()))
def test_q_maps(name):
    kQ, iQ, Q = q_patterns()[name]
    n = kQ.size - 1
    cols = np.repeat(np.arange(n), np.diff(kQ))
    qt = ipo_amd.value_maps(n, n, kQ, iQ, "qt")
    qd = ipo_amd.value_maps(n, n, kQ, iQ, "qdiag")
    assert qt.size == iQ.size and qd.size == n
    # the transposed entry, an involution, the diagonal fixed
    assert np.array_equal(iQ[qt], cols) and np.array_equal(cols[qt], iQ)
    assert np.array_equal(qt[qt], np.arange(iQ.size))
    diag = np.nonzero(iQ == cols)[0]
    assert np.array_equal(qt[diag], diag)
    # exactly the diagonal entries, by column; -1 where a column has none
    want = np.full(n, -1)
    want[cols[diag]] = diag
    assert np.array_equal(qd, want)
    if name == "gaps":
        assert (np.diff(kQ) == 0).any() and (qd == -1).any()
    # symmetric values pass the update's test Q[k] == Q[qt[k]]; one side changed does not
    assert np.array_equal(Q, Q[qt])
    off = np.nonzero(iQ != cols)[0]
    if off.size:
        Q2 = Q.copy()
        Q2[off[0]] += 1.0
        bad = np.nonzero(Q2 != Q2[qt])[0]
        assert sorted(bad) == sorted([off[0], qt[off[0]]])


def test_refusals():
    kQ, iQ, _ = qp_ref.csc_of(np.array([[1.0, 1.0], [0.0, 1.0]]))        # (0, 1) without (1, 0)
    with pytest.raises(ipo_amd.IpoHipError, match="symmetric"):
        ipo_amd.value_maps(2, 2, kQ, iQ, "qt")
    p = shapes()["63x65"]
    with pytest.raises(ipo_amd.IpoHipError, match="square"):
        ipo_amd.value_maps(p.m, p.n, p.kA, p.iA, "qdiag")
    with pytest.raises(ipo_amd.IpoHipError, match="unknown"):
        ipo_amd.value_maps(p.m, p.n, p.kA, p.iA, "nonesuch")
    bad = p.iA.copy()
    bad[3] = p.m
    with pytest.raises(ipo_amd.IpoHipError, match="out of range"):
        ipo_amd.value_maps(p.m, p.n, p.kA, bad, "csr")


def test_header_and_binding():
    """The header declares every new entry and the ctypes binding resolves it."""
    names = declared_functions()
    L = ipo_amd.lib()
    for n in NEW_ENTRIES:
        assert n in names and n in ipo_amd.EXPORTED and hasattr(L, n), n
    for meth in ("update", "set_start", "clear_start", "start_from_last"):
        assert callable(getattr(ipo_amd.Context, meth)) and callable(getattr(ipo_amd.ShardContext, meth))
