"""Every dense-tail path of the factorisation (kkt_dense.hip: k_tail_run, the
look-ahead panels, the visits, the tail sweeps) on small synthetic systems
whose tail size is chosen -- tests/test_tail_shapes.py lists and pins them:
tails of exactly 128, 129, 192, 193 ... rows, last blocks of 1, 15, 16, 17, 63
and 64 rows, the whole matrix as the tail (tail_c0 = 0, no sparse supernode),
gather tasks with partial masks -- against the long-double LDL' of
tests/kkt_ref.py.

Bounds.  The fp64 oracle's own distance from that reference on the same case
(the largest of its three summation orders, computed here) is the unit: the
device pivots, max |d - d_ref| / |d_ref|, and the refined solution,
||x - x_ref||_inf / (1 + ||x_ref||_inf), may be MARGIN = 16 times as far.  The
device sums in another order again (MFMA k-steps, up to four blocks'
products in one accumulator, no FMA contraction on either side), and the
largest of T differently rounded sums can pass one order's largest by a
small factor; 16 is about 1e-13 on the unit scaling, four orders below the
suite's 1e-9, and does not depend on the code under test.  Refinement passes:
at most the oracle's largest count plus one.

Measured on an MI355X (largest device / oracle ratio per family, over every
shape, scaling and path; every case prints its own):
  pivots    S1 1.38 (nt 145, wide), S2 1.40 (60 x 69, wide), S3 1.74 (r = 105, density 1, wide);
            at unit scaling 0.93, 0.91 and 1.29;
  solution  S1 1.00, S2 1.29 (60 x 69, unit), S3 1.00;
  passes    1 at unit scaling, 2 at wide scaling, as the oracle.
A visit that leaves out one block's products on the tiles of a partial last
block row (tried once on the device, not kept) fails test A on every shape
with such a row and at least four block columns, on every path whose chunks
hold two blocks or more, with pivots wrong in the first digit -- while the
bitwise group agrees with itself and refinement still brings the solution
to 1e-11 of the reference, inside the suite's older 1e-8 bar.
"""
import functools
import os

import numpy as np
import pytest

import ipo_amd
import kkt_ref
from test_tail_shapes import SCALINGS, SEED, SHAPE_IDS, SHAPES, SOLVE_SHAPES, oracle_case, oracle_hsd

pytestmark = pytest.mark.gpu

MARGIN = 16

PIN = {"IPO_HIP_VISIT_BLOCKS": "4", "IPO_HIP_VISIT_LATEST": "4"}
# the same operations in the same order (tests/test_gpu_panel.py), all at K = L = 4
BITWISE = {
    "default": {},
    "run0": {"IPO_HIP_TAIL_RUN": "0"},                  # one launch per look-ahead step
    "winpub0": {"IPO_HIP_TAIL_WINPUB": "0"},            # no window hand-off
    "sched0": {"IPO_HIP_VISIT_SCHED": "0"},             # visit placement only
    "xcd0": {"IPO_HIP_VISIT_XCD": "0"},                 # schedule order
    "lead0": {"IPO_HIP_CHAIN_LEAD": "0"},               # per-block forward chain
    "pairs": {"IPO_HIP_CHAIN_LEAD": "0", "IPO_HIP_CHAIN_PAIRS": "1"},
}
PATHS = {k: dict(PIN, **v) for k, v in BITWISE.items()}
PATHS["panel0"] = dict(PIN, IPO_HIP_PANEL="0")          # per-phase kernels
PATHS["kl1"] = {"IPO_HIP_VISIT_BLOCKS": "1", "IPO_HIP_VISIT_LATEST": "1"}     # other chunkings: to rounding
PATHS["kl6"] = {"IPO_HIP_VISIT_BLOCKS": "6", "IPO_HIP_VISIT_LATEST": "6"}
CONTROLLED = sorted({v for e in PATHS.values() for v in e} | {"IPO_HIP_TAIL_DENSITY"})
BY_ID = {s[0]: s for s in SHAPES}


class _Env:
    """The controlled variables set to exactly `env` (the others unset) for a
    block; the library reads them when a factor is built."""

    def __init__(self, env, density):
        self.env = dict(env)
        if density is not None:
            self.env["IPO_HIP_TAIL_DENSITY"] = repr(density)

    def __enter__(self):
        self.old = {v: os.environ.get(v) for v in CONTROLLED}
        for v in CONTROLLED:
            os.environ.pop(v, None)
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for v, x in self.old.items():
            if x is None:
                os.environ.pop(v, None)
            else:
                os.environ[v] = x


def _factor_solve(k, c):
    k.factor(c.E, c.D)
    d, live = k.pivots()
    y, x, ok = k.solve(c.E, c.D, c.fy, c.fx)
    i = k.info()
    return dict(d=d, live=live, y=y, x=x, ok=ok, ndep=i["ndep"], passes=i["passes"])


def _factor(sid, path):
    _, family, shape, density, nt = BY_ID[sid]
    p = kkt_ref.case(family, shape, SEED, "unit").p
    with _Env(PATHS[path], density):
        assert ipo_amd.symbolic_tail(p.m, p.n, p.kA, p.iA)["nt"] == nt     # the tail this case is there for
        return ipo_amd.KktFactor(p.m, p.n, p.kA, p.iA, p.A)


@functools.lru_cache(maxsize=None)
def gpu_run(sid, kind, path):
    """A fresh device factor of shape `sid` on path `path`: pivots, live
    marks, refined solution (once per process; shared by the tests below)."""
    _, family, shape, _, _ = BY_ID[sid]
    k = _factor(sid, path)
    try:
        out = _factor_solve(k, kkt_ref.case(family, shape, SEED, kind))
        out["perm"] = k.perm()
        return out
    finally:
        k.close()


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("kind", SCALINGS)
@pytest.mark.parametrize("sid", SHAPE_IDS)
def test_paths_against_reference(sid, kind, path):
    """Test A: every shape, scaling and path against the long-double
    reference, in units of the oracle's own distance from it."""
    _, family, shape, _, _ = BY_ID[sid]
    c = kkt_ref.case(family, shape, SEED, kind)
    o = oracle_case(family, shape, kind)
    g = gpu_run(sid, kind, path)
    assert np.array_equal(g["perm"], c.perm)        # the oracle's (oracle_case checks its own against c.perm)
    assert g["ndep"] == 0 and g["live"].all() and g["ok"] == 1
    rp = c.pivot_distance(g["d"]) / max(o["pivot"])
    rs = c.solution_distance(g["y"], g["x"]) / max(o["solution"])
    print(f"{sid} {kind} {path}: pivot distance {c.pivot_distance(g['d']):.2e} = {rp:.2f} x oracle, solution "
          f"{c.solution_distance(g['y'], g['x']):.2e} = {rs:.2f} x oracle, passes {g['passes']} (oracle {o['passes']})")
    assert rp <= MARGIN
    assert rs <= MARGIN
    assert g["passes"] <= o["passes"] + 1


@pytest.mark.parametrize("kind", SCALINGS)
@pytest.mark.parametrize("sid", SHAPE_IDS)
def test_bitwise_group(sid, kind):
    """Test B: the paths documented as the same operations in the same order
    give the same bits: pivots, live marks, refined solution."""
    ref = gpu_run(sid, kind, "default")
    for path in BITWISE:
        g = gpu_run(sid, kind, path)
        for key in ("d", "live", "y", "x"):
            assert np.array_equal(g[key], ref[key]), (path, key)


@pytest.mark.parametrize("path", ["default", "run0"])
@pytest.mark.parametrize("sid", ["S1-nt129", "S1-nt193", "S1-nt577", "S2-60x69", "S3-r105-dflt"])
def test_state_across_factorisations(sid, path):
    """Test C: one factor object, three factorisations -- unit scaling, wide
    scaling (what is left in the tail differs by up to 1e12), unit scaling
    again; each bitwise what a fresh object gives for the same input (the
    run's epochs, window flags, double-buffered windows and counters, and
    the tail's partial clear, carry nothing over)."""
    _, family, shape, _, _ = BY_ID[sid]
    cu, cw = (kkt_ref.case(family, shape, SEED, kind) for kind in ("unit", "wide"))
    k = _factor(sid, path)
    try:
        outs = [_factor_solve(k, c) for c in (cu, cw, cu)]
    finally:
        k.close()
    fresh = [gpu_run(sid, kind, path) for kind in ("unit", "wide", "unit")]
    for i, (a, b) in enumerate(zip(outs, fresh)):
        assert a["ok"] == b["ok"] == 1 and a["ndep"] == b["ndep"] == 0 and a["passes"] == b["passes"]
        for key in ("d", "live", "y", "x"):
            assert np.array_equal(a[key], b[key]), (i, key)


@pytest.mark.parametrize("density", [None, 1.0], ids=["dflt", "rho1"])
@pytest.mark.parametrize("shape", SOLVE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_whole_solves(shape, density):
    """Test D: HSD solves of the dense family (the two-right-hand-side tail
    sweeps on partial blocks) against the oracle, whose three summation
    orders agree on these (tests/test_tail_shapes.py): status 0, iterations
    within one, final objectives to 1e-6 relative -- the synthetic LPs' bars
    of tests/test_gpu_deep.py."""
    p = kkt_ref.dense_lp(*shape, SEED)
    o = oracle_hsd(shape)[0]
    with _Env(PIN, density):
        r = ipo_amd.solver(p, "hsd")
    st = r["stats"]
    print(f"dense{shape} density {density}: {st['iters']} iterations (oracle {o['iters']}), "
          f"pobj {st['final_pobj']:.12e} (oracle {o['final_pobj']:.12e})")
    assert r["status"] == 0 and o["status"] == 0
    assert abs(st["iters"] - o["iters"]) <= 1
    for key in ("final_pobj", "final_dobj"):
        assert abs(st[key] - o[key]) <= 1e-6 * max(1.0, abs(o[key]))
