"""Every sparse path of the factorisation and of the substitution sweeps
(kkt_device.hip: k_update, k_update_flat, k_update_quad, split-K partial
tiles and their wide sum; kkt_dense.hip: k_panel_w, k_panel_s, k_panel_s1,
k_panel_ws, k_diag + k_trsm; kkt_sweep.hip: the leaf, leaf8, level, plain,
chunked, pre-pass and sync-free kernels) on small synthetic systems whose
supernodes are chosen -- tests/test_sparse_shapes.py lists and pins them:
supernodes of 15, 16, 17, 63, 64 and 65 columns, panels of 63 ... 66, 128, 129
and 257 rows, 128 and 129 rows below, leaves with 8, 9, 64 and 65 rows below,
units of 15 ... 17 and 31 ... 33 k-slots, tiles on the quadrant edges -- against
the long-double LDL' of tests/kkt_ref.py.

Bounds (those of tests/test_gpu_tail_shapes.py, where MARGIN is justified).
The fp64 oracle's own distance from the reference on the same case (the
largest of its three summation orders) is the unit: the device pivots,
max |d - d_ref| / |d_ref|, and the refined solution, ||x - x_ref||_inf /
(1 + ||x_ref||_inf), may be MARGIN = 16 times as far.  The unit has a floor
of 2^-50 = 8.9e-16: the unit, the largest of the oracle's three orders, is as
low as 1.3e-16 (leaf8, wide scaling; single orders reach 4e-17), and no fp64
result can be held closer to the reference than a few roundings of the value
itself (derived, not measured).  On b5x6 at wide scaling the solution's unit
is 7.8e-10, from one order that stops after one pass: the solution bound is
about 1e-8 there, and only the pivot bound is sharp.  Refinement passes:
at most the oracle's largest count plus one.

Paths (tests/test_sparse_shapes.py: PATHS).  The same operations in the same
order, bitwise: default, sf0, sfw1, merge0, leaf8, split1, flat2, occ1, xcd1,
and panel0 on the shapes without a dense tail (the per-phase kernels factor a
tail in another order: tests/test_gpu_panel.py).  To rounding: chunk16
(other split-K partial sums), visits and vslots16 (slots in source-level
order, early ones as visits), panel0 under a tail.
visits_noquad against visits: k_update_quad runs gather_acc_flat's MFMA steps
in its k order on every entry (kkt_device.hip: the kk loop of k_update_quad
against that of gather_acc_flat, both over rounds of FK slots from kb) and
sums the diagonal's |terms| in gather_acc's four wave partials, added as
gather_put adds them (dp[w] and ((dp[0] + dp[1]) + dp[2]) + dp[3] against
dred) -- but over a unit's whole slot range: ck_part holds the quadrant, there
is no split K.  The flat gather splits a unit of more than 64 slots here into
chunks whose partial tiles are summed afterwards, another order.  So the pair
is bitwise exactly on the shapes where the flat schedule splits no unit the
quadrant schedule gathers whole (equal pinned sp_n: NOQUAD_BITWISE, nine
shapes), and to rounding on the others.  The shapes quad and b40x300 are
among the others (their top units have 393 and 704 slots): their quadrant
gathers are compared to rounding only, in test A.  quad0 and quad31 are the
bitwise partners of quad's edge tiles: the same block sizes in trees whose
units the flat schedule leaves whole.

Measured on an MI355X (largest device / oracle ratio over every shape and
path; every case prints its own; the 19 x 2 x 14 factors, the 15 state cases
and the 8 whole solves take 11 s together):
  pivots    unit 1.46 (mixed3, visits), wide 1.44 (mixed3, chunk16); the
            bitwise group 1.40 (b65x90, unit); per shape 0.29 ... 1.46
  solution  unit 1.51 (mixed3, chunk16), wide 1.11 (b70x150, default); the
            floor of 2^-50 = 8.9e-16 is the unit on most unit-scaling cases
            (the oracle's distance there is 1e-16 ... 5e-15)
  passes    1 at unit scaling; at wide scaling the oracle's count, but 1 on
            b4x12 outside the visit paths, where two of the oracle's three
            orders take 1 and one takes 2
  whole solves: the oracle's iteration count on all eight, objectives to 1e-11
Two arithmetic faults tried once on the device (before quad0 and quad31
were added), not kept.  split_sum leaving out the last partial tile of a unit split five ways or more fails test A on
every path on the eight shapes with such a unit (b70x150, b40x300, b10x200,
b8x300, leafh, rows128, rows129, quad) and on 28 of chunk16's 34 cases, while
the bitwise group and test C still agree with themselves.  k_bwd_leaf8
without its first reduction step (leaves of more than four rows) fails test
B on the six shapes with such small leaves, and test A on five of their
wide-scaling cases.
"""
import functools

import numpy as np
import pytest

import ipo_amd
import kkt_ref
from test_sparse_shapes import (PATHS, SCALINGS, SEED, SHAPE_IDS, SHAPES, SOLVE_KINDS, Env, check_pinned, lp,
                                oracle_case, oracle_hsd, pinned)

pytestmark = pytest.mark.gpu

MARGIN = 16
FLOOR = 2.0 ** -50

# the same operations in the same order
BITWISE = ("default", "sf0", "sfw1", "merge0", "leaf8", "split1", "flat2", "occ1", "xcd1")
# shapes on which visits_noquad splits no unit that visits gathers whole (module docstring)
NOQUAD_BITWISE = [s for s in SHAPE_IDS if 2 in pinned(s, "visits")["ck_kind"] and
                  pinned(s, "visits_noquad")["sp_n"] == pinned(s, "visits")["sp_n"]]


def has_tail(sid):
    return pinned(sid, "default")["nt"] > 0


def _factor_solve(k, c):
    k.factor(c.E, c.D)
    d, live = k.pivots()
    y, x, ok = k.solve(c.E, c.D, c.fy, c.fx)
    i = k.info()
    return dict(d=d, live=live, y=y, x=x, ok=ok, ndep=i["ndep"], passes=i["passes"])


def _factor(sid, path):
    p = lp(sid)
    check_pinned(sid, path)         # the structure this case is there for
    with Env(PATHS[path]):
        return ipo_amd.KktFactor(p.m, p.n, p.kA, p.iA, p.A)


@functools.lru_cache(maxsize=None)
def gpu_run(sid, kind, path):
    """A fresh device factor of shape `sid` on path `path`: pivots, live
    marks, refined solution (once per process; shared by the tests below)."""
    k = _factor(sid, path)
    try:
        out = _factor_solve(k, kkt_ref.case("blocks", SHAPES[sid], SEED, kind))
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
    c = kkt_ref.case("blocks", SHAPES[sid], SEED, kind)
    o = oracle_case(sid, kind)
    g = gpu_run(sid, kind, path)
    assert np.array_equal(g["perm"], c.perm)        # the oracle's (oracle_case checks its own against c.perm)
    assert g["ndep"] == 0 and g["live"].all() and g["ok"] == 1
    rp = c.pivot_distance(g["d"]) / max(FLOOR, max(o["pivot"]))
    rs = c.solution_distance(g["y"], g["x"]) / max(FLOOR, max(o["solution"]))
    print(f"{sid} {kind} {path}: pivot distance {c.pivot_distance(g['d']):.2e} = {rp:.2f} x oracle, solution "
          f"{c.solution_distance(g['y'], g['x']):.2e} = {rs:.2f} x oracle, passes {g['passes']} (oracle {o['passes']})")
    assert rp <= MARGIN
    assert rs <= MARGIN
    assert g["passes"] <= o["passes"] + 1


def _same_bits(sid, kind, a, b):
    ga, gb = gpu_run(sid, kind, a), gpu_run(sid, kind, b)
    for key in ("d", "live", "y", "x"):
        assert np.array_equal(ga[key], gb[key]), (a, b, key)


@pytest.mark.parametrize("kind", SCALINGS)
@pytest.mark.parametrize("sid", SHAPE_IDS)
def test_bitwise_group(sid, kind):
    """Test B: the paths documented as the same operations in the same order
    give the same bits: pivots, live marks, refined solution."""
    for path in BITWISE + (() if has_tail(sid) else ("panel0",)):
        _same_bits(sid, kind, "default", path)


@pytest.mark.parametrize("kind", SCALINGS)
@pytest.mark.parametrize("sid", NOQUAD_BITWISE)
def test_quadrant_gathers_bitwise(sid, kind):
    """Test B, the pair visits / visits_noquad where no unit is split."""
    assert 2 not in pinned(sid, "visits_noquad")["ck_kind"]
    _same_bits(sid, kind, "visits", "visits_noquad")


@pytest.mark.parametrize("path", ["default", "sf0", "visits"])
@pytest.mark.parametrize("sid", ["b70x150", "b40x300", "b10x200", "rows129", "split"])
def test_state_across_factorisations(sid, path):
    """Test C: one factor object, three factorisations -- unit scaling, wide
    scaling, unit scaling again; each bitwise what a fresh object gives for
    the same input (the split units' arrival counters and partial tiles, the
    sync-free epochs, counters and flags, ybuf and zpad carry nothing over).
    b70x150: units split up to six ways, the wide partial sum; b40x300: the
    pre-pass and quadrant gathers; b10x200, rows129: chunked levels under a
    tail; split: chunked multi-column supernodes inside the sync-free range."""
    cu, cw = (kkt_ref.case("blocks", SHAPES[sid], SEED, kind) for kind in ("unit", "wide"))
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


@pytest.mark.parametrize("sid,path", list(SOLVE_KINDS), ids=lambda v: v)
def test_whole_solves(sid, path):
    """Test D: HSD solves (the two-right-hand-side sweeps, k_perm_in2 through
    every level kind) against the oracle, whose three summation orders agree
    on these (tests/test_sparse_shapes.py): status 0, iterations within one,
    final objectives to 1e-6 relative -- the bars of
    tests/test_gpu_tail_shapes.py.  Which kinds each case runs is SOLVE_KINDS,
    asserted here from the pins: leaf8 at sf0 Leaf, Merged and Plain, on path
    leaf8 also Leaf8; b10x200 Chunked under a tail; quad the sync-free range,
    at sf0 Leaf and Plain, and the quadrant gathers at visits."""
    assert set(pinned(sid, path)["fwd"]) == set(SOLVE_KINDS[sid, path])
    assert path != "visits" or 2 in pinned(sid, path)["ck_kind"]
    o = oracle_hsd(sid)[0]
    check_pinned(sid, path)
    with Env(PATHS[path]):
        r = ipo_amd.solver(lp(sid), "hsd")
    st = r["stats"]
    print(f"{sid} {path}: {st['iters']} iterations (oracle {o['iters']}), "
          f"pobj {st['final_pobj']:.12e} (oracle {o['final_pobj']:.12e})")
    assert r["status"] == 0 and o["status"] == 0
    assert abs(st["iters"] - o["iters"]) <= 1
    for key in ("final_pobj", "final_dobj"):
        assert abs(st[key] - o[key]) <= 1e-6 * max(1.0, abs(o[key]))
