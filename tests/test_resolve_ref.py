"""What tests/test_gpu_resolve.py relies on, checked on the host: the
restated iteration with a start argument (tests/pc_start_ref.py) is
pc_ref's, the references end optimal on every case's second member, and the
warm start's floor ends optimal from the clamped previous solution on all of
them.  Without a GPU.
"""
import functools

import numpy as np
import pytest

import pc_ref
import pc_start_ref as ps
import qp_ref


@functools.lru_cache(maxsize=None)
def members(name):
    p, backend, seed = ps.case(name)
    return p, ps.second_member(p, seed), backend


@pytest.mark.parametrize("name", sorted(ps.CASES))
def test_restatement_is_pc_ref(name):
    p, _, backend = members(name)
    a, b = pc_ref.solve_pc(p, backend), ps.solve_pc(p, backend)
    assert a["status"] == b["status"] == 0 and a["rows"] == b["rows"]
    for k in "xywz":
        assert np.array_equal(a[k], b[k])
    # an explicit start at the default is the default, and a stopped run goes on where it stood
    c = ps.solve_pc(p, backend, start=(np.full(p.n, 1000.0), np.full(p.m, 1000.0), np.full(p.m, 1000.0),
                                       np.full(p.n, 1000.0)))
    assert c["rows"] == a["rows"]
    head = ps.solve_pc(p, backend, max_iter=5)
    rest = ps.solve_pc(p, backend, start=tuple(head[k] for k in "xywz"))
    assert head["status"] == 5 and [r[1:] for r in rest["rows"]] == [r[1:] for r in a["rows"][5:]]


@pytest.mark.parametrize("name", sorted(ps.CASES))
def test_second_member(name):
    """The same pattern, factors in [0.8, 1.25], Q symmetric bit for bit, and
    the references end optimal on it (pc's, and intpt's / qp's iteration)."""
    p, p2, backend = members(name)
    assert np.array_equal(p.kA, p2.kA) and np.array_equal(p.iA, p2.iA)
    for a, b in ((p.A, p2.A), (p.b, p2.b), (p.c, p2.c)):
        r = b[a != 0] / a[a != 0]
        assert r.min() >= 0.8 - 1e-12 and r.max() <= 1.25 + 1e-12 and not np.array_equal(a, b)
    if p.q is not None:
        n = p.n
        r = p2.q[2] / p.q[2]
        assert r.min() >= 0.8 - 1e-12 and r.max() <= 1.25 + 1e-12
        M = qp_ref.q_dense(n, p2.q)
        assert np.array_equal(M, M.T) and np.linalg.eigvalsh(M).min() >= -1e-12 * np.abs(M).max()
    pc, qp = pc_ref.solve_pc(p2, backend), qp_ref.solve_qp(p2, backend)
    print(name, "pc", pc["status"], pc["iters"], "qp / intpt", qp["status"], qp["iters"])
    assert pc["status"] == 0 and qp["status"] == 0


@pytest.mark.parametrize("name", sorted(ps.CASES))
def test_warm_floor(name):
    """From max(member 1's solution, floor) the restated pc ends optimal on
    member 2, at WARM_FLOOR and a decade either side."""
    p, p2, backend = members(name)
    r1 = ps.solve_pc(p, backend)
    cold = ps.solve_pc(p2, backend)
    for mult in (0.1 * ps.WARM_FLOOR, ps.WARM_FLOOR, 10.0 * ps.WARM_FLOOR):
        fl = ps.warm_floor(r1["gamma"], p, mult)
        warm = ps.solve_pc(p2, backend, start=tuple(np.maximum(r1[k], fl) for k in "xywz"))
        print(f"{name}: floor {fl:.3e} ({mult:g} units): warm {warm['status']} after {warm['iters']} lines, "
              f"cold {cold['iters']}")
        assert warm["status"] == 0
        pr, du, gap, lo = qp_ref.certificate(p2, warm["x"], warm["y"], warm["w"], warm["z"])
        assert pr <= 1e-6 and du <= 1e-6 and gap <= 1e-6 and lo > 0
