"""The yardstick of the start rule "mehrotra" (Context.set_start_rule,
DESIGN.md section 10.4): the rule in NumPy on pc_ref's back ends (a plain
module, no fixtures).

"Solve" is a back end's solve(E, D, fy, fx): [-E A; A' D (+ Q)] (dy, dx) =
(fy, fx).

  1. E = 1 (m entries), D = 1 (n entries)
  2. solve with (fy, fx) = (b, 0): x~ = dx, w~ = -dy, so A x~ + w~ = b, at
     least norm (with Q the norm weighted by I + Q)
  3. solve with (fy, fx) = (0, c): y~ = dy, z~ = -dx, for an LP
     A'y~ - z~ = c at least norm
  4. delta_p = max(0, -1.5 min(x~, w~)) onto x~ and w~,
     delta_d = max(0, -1.5 min(y~, z~)) onto y~ and z~
  5. g = x'z + w'y, Sp = sum x + sum w, Sd = sum z + sum y.  If g, Sp and Sd
     are all > 0: eps_p = g / (2 Sd), eps_d = g / (2 Sp); otherwise both 1
     (b = 0 and c = 0).  eps_p onto x and w, eps_d onto y and z.

Also here, for tests/test_start_rule.py and tests/test_gpu_start_rule.py:
their cases.
"""
import functools

import numpy as np

import pc_ref
import pc_start_ref
from qp_ref import _Dense, _Oracle, _mats


def backend_of(p, backend):
    _, Q = _mats(p)
    return (_Dense(p) if backend == "dense" else (_Oracle(p) if Q is not None else pc_ref._OracleLp(p))
            if backend == "oracle" else backend)


def least_squares(p, backend="dense"):
    """Steps 1 to 3: (x~, y~, w~, z~), before any shift."""
    lin = backend_of(p, backend)
    b, c = np.asarray(p.b, np.float64), np.asarray(p.c, np.float64)
    E, D = np.ones(p.m), np.ones(p.n)
    dy, dx = lin.solve(E, D, b, np.zeros(p.n))
    x, w = dx, -dy
    dy, dx = lin.solve(E, D, np.zeros(p.m), c)
    y, z = dy, -dx
    return x, y, w, z


def shifts(x, y, w, z):
    """Steps 4 and 5 on the least-squares point: (delta_p, delta_d, eps_p, eps_d)."""
    dp = max(0.0, -1.5 * min(x.min(), w.min()))
    dd = max(0.0, -1.5 * min(y.min(), z.min()))
    x, w, y, z = x + dp, w + dp, y + dd, z + dd
    g = x @ z + w @ y
    Sp = x.sum() + w.sum()
    Sd = z.sum() + y.sum()
    if g > 0 and Sp > 0 and Sd > 0:
        return dp, dd, g / (2 * Sd), g / (2 * Sp)
    return dp, dd, 1.0, 1.0


def start(p, backend="dense"):
    """The rule's point (x, y, w, z)."""
    x, y, w, z = least_squares(p, backend)
    dp, dd, ep, ed = shifts(x, y, w, z)
    return (x + dp) + ep, (y + dd) + ed, (w + dp) + ep, (z + dd) + ed


# ---------------------------------------------------------------- the cases
def zero_lp():
    """The b = c = 0 member of lp_shape(3, 5, 0): the rule gives all ones."""
    import ipo_amd
    import test_pc
    p = test_pc.lp_shape(3, 5, 0)
    return ipo_amd.SolverForm(p.m, p.n, p.kA, p.iA, p.A, np.zeros(p.m), np.zeros(p.n), p.f)


# name -> (make in test_pc or test_qp_solver, its arguments, the back end)
CASES = {
    "lp 3x5": ("lp_shape", (3, 5, 0), "dense"),
    "lp 1x64": ("lp_shape", (1, 64, 0), "dense"),
    "lp 63x65": ("lp_shape", (63, 65, 0), "dense"),
    "lp 200x40": ("lp_shape", (200, 40, 0), "dense"),
    "banded 63x65": ("small_case", (63, 65, "banded", 12), "dense"),
    "gaps 20x30": ("small_case", (20, 30, "gaps", 2), "dense"),
    "lowrank 40x200": ("small_case", (40, 200, "lowrank", 0), "dense"),
    "diag 1x64": ("small_case", (1, 64, "diag", 0), "dense"),
    "afiro": ("netlib_lp", ("afiro",), "oracle"),
    "stocfor1": ("netlib_lp", ("stocfor1",), "oracle"),
    "afiro with Q": ("netlib_problem", ("afiro",), "oracle"),
}
ZERO = "zero lp 3x5"


def problem(name):
    import test_pc
    import test_qp_solver
    if name == ZERO:
        return zero_lp(), "dense"
    make, args, backend = CASES[name]
    mod = test_qp_solver if make == "netlib_problem" else test_pc
    return getattr(mod, make)(*args), backend


@functools.lru_cache(maxsize=None)
def reference(name):
    """(problem, its start, the restated pc run from it), computed once per
    process and shared, read-only, by the tests that need it."""
    p, backend = problem(name)
    s = start(p, backend)
    return p, s, pc_start_ref.solve_pc(p, backend, start=s)
