"""Small synthetic KKT systems whose sparse supernodes have chosen sizes (host
code, no GPU): the shapes tests/test_gpu_sparse_shapes.py runs every sparse
path of the factorisation and of the sweeps over (kkt_device.hip: k_update,
k_update_flat, k_update_quad, split K; kkt_dense.hip: k_panel_w / _s / _s1 /
_ws, k_diag + k_trsm; kkt_sweep.hip: the leaf, level, plain, chunked,
pre-pass and sync-free kernels), what each realises pinned through
ipo_hip_kkt_schedule, and the fp64 oracle (oracle/orc_kkt.c, its three
summation orders) measured against the long-double LDL' of tests/kkt_ref.py.
The oracle's distance from that reference is the unit of the GPU tests'
bounds.

Shapes (tests/kkt_ref.py: blocks_lp(blocks, r); all at tail density 1).  A
block (m_i, n_i) whose rows have the lower degree (n_i < m_i + r) becomes
single-column leaves with n_i rows below and one supernode of n_i columns;
otherwise leaves with m_i + r rows below and a supernode of m_i + 1 columns;
r rows below either supernode, panels of at most 64 columns; the linking rows
and one block's supernode end on top, as a dense tail from 128 rows up.
  b5x6 ... b65x90   the first nine of SHAPES, in order: small panels only; a
           unit split four ways at IPO_HIP_MIN_CHUNK=16; eight-to-a-wave
           panels and leaves (two shapes); merged levels and units split up
           to six ways (the wide partial sum); four levels, the pre-pass and
           quadrant gathers under IPO_HIP_VISITS=1; chunked levels under a
           tail (135 and 130 rows below, two shapes); a tail of 152
  small    supernodes of 15, 16 and 17 columns, 3 rows below: the first two
           are small panels (nc <= 16 and h <= 64), the third is fused
  leafh    leaves with 62, 63, 64 and 65 rows below (panel heights 63 ... 66:
           63 and 64 small, 65 and 66 fused of one unit; 65 is no leaf:
           k_forward / k_backward), supernodes of 62, 63 and 64 columns and
           one of 65 that splits into (64, 4) and a column on top
  rows128  leaves with 127 and 128 rows below (h = 128: one fused unit,
           h = 129: two); no level is chunked; tail 129
  rows129  leaves with 128 and 129 rows below on one level, which is chunked
           (kChunkRows = 128 < 129); tail 130
  leaf8    leaves with 8 and 9 rows below (kSmallLeaf = 8), single-column
           panels of 2, 3 and 9, 10 rows (k_panel_s1 takes <= 8), and on
           level 1 two single-column supernodes with 3 rows below and update
           lists of 5 and of 12 entries: the second is no small leaf
  kslots   units of 15, 16, 17, 31, 32 and 33 k-slots (kSlab = 16), and one of
           179 (three chunks)
  quad     supernodes of 29 ... 33 columns with 2 rows below: tiles of 31 ...
           35 rows and 29 ... 33 columns, on either side of k_update_quad's
           32 x 32 quadrants; quadrant gathers under IPO_HIP_VISITS=1.  The
           flat schedule splits its top unit, so the quadrant gathers are
           held to rounding here; the next two are their bitwise partners
  quad0    the same five blocks without linking rows: five trees, square
           tiles of 29 ... 33 rows and columns, 39 k-slots each
  quad31   a supernode of 31 columns with 2 rows below (a tile of 33 rows: the
           rows straddle the quadrants, the columns do not) under a top tile
           of 37 x 37 with a visit; no unit of either is split by the flat
           schedule, so k_update_quad must give k_update_flat's bits
  split    two supernodes of 130 columns under 127 linking rows: panels
           (64, 193) and (64, 129), h = 257 and 193: four and three fused
           units, chunked sweeps of multi-column supernodes; the first is
           alone on its level, which runs k_diag + k_trsm under
           IPO_HIP_PANEL_SPLIT=1; tail 257

Scalings: "unit", E, D ~ U(0.1, 10); "wide", log-uniform in [1e-6, 1e6].

Measured (this module, over shapes and the three summation orders):
  pivots    max |d_orc - d_ref| / |d_ref|
            unit  6.5e-16 (kslots) ... 4.6e-15 (b10x200)
            wide  1.2e-14 (kslots) ... 1.4e-07 (b65x90), 1.4e-05 (split)
  solution  ||x_orc - x_ref||_inf / (1 + ||x_ref||_inf)
            unit  2.8e-16 (leaf8) ... 5.3e-15 (b65x90)
            wide  1.3e-16 (leaf8) ... 4.7e-12 (split), 7.8e-10 (b5x6, one order in one pass)
  refinement passes: 1 at unit scaling; 2 at wide scaling, except b5x6 and
  b4x12, where one order takes 2 and two take 1; no dependent pivot anywhere.
At wide scaling the distances are those of the systems, not of the oracle
(tests/test_tail_shapes.py).
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "linear-programming-vanderbei_amd"))     # as tests/test_kkt_schedule.py: also a script
import ipo_amd  # noqa: E402
import kkt_ref  # noqa: E402
import oracle_lib  # noqa: E402

SEED = 20251121
SCALINGS = ("unit", "wide")

# id -> (blocks, r)
SHAPES = {
    "b5x6": (((5, 6),) * 4, 2),
    "b4x12": (((4, 12),) * 4, 4),
    "mixed3": (((1, 2),) * 6 + ((30, 50), (17, 30)), 3),
    "mixed6": (((1, 3), (2, 5), (20, 40), (40, 100), (3, 3)), 6),
    "b70x150": (((70, 150), (33, 80)), 20),
    "b40x300": (((40, 300),) * 2, 30),
    "b10x200": (((10, 200),) * 2, 125),
    "b8x300": (((8, 300),), 122),
    "b65x90": (((65, 90),) * 2, 62),
    "small": (((14, 20), (15, 21), (16, 22), (17, 24)), 3),
    "leafh": (((66, 62), (66, 63), (66, 64), (66, 65), (3, 8)), 3),
    "rows128": (((8, 140), (7, 140)), 120),
    "rows129": (((9, 140), (8, 140)), 120),
    "leaf8": (((1, 2),) * 3 + ((12, 1), (5, 1), (5, 12), (6, 12), (2, 9)), 3),
    "kslots": (((3, 12), (3, 16), (3, 17), (3, 18), (3, 32), (3, 33), (3, 34)), 2),
    "quad": (((28, 40), (29, 40), (30, 40), (31, 40), (32, 40), (34, 44)), 2),
    "quad0": (((28, 40), (29, 40), (30, 40), (31, 40), (32, 40)), 0),
    "quad31": (((30, 40), (34, 44)), 2),
    "split": (((4, 130),) * 2, 127),
}
SHAPE_IDS = list(SHAPES)
# the whole solves of the GPU module (Test D): leaf8, leaf, merged and plain levels (SOLVE_KINDS); chunked levels
# under a tail; quadrant gathers
SOLVE_SHAPES = ("leaf8", "b10x200", "quad")
# (shape, path) of Test D -> level kinds its forward list must hold; between them every level kind
SOLVE_KINDS = {
    ("leaf8", "default"): ("SyncFree",),
    ("leaf8", "sf0"): ("Leaf", "Merged", "Plain"),
    ("leaf8", "leaf8"): ("Leaf8", "Leaf", "Merged", "Plain"),
    ("b10x200", "default"): ("Chunked", "Plain", "TailGather", "TailLead"),
    ("b10x200", "sf0"): ("Chunked", "Plain", "TailGather", "TailLead"),
    ("quad", "default"): ("SyncFree",),
    ("quad", "sf0"): ("Leaf", "Plain"),
    ("quad", "visits"): ("SyncFree",),
}

# The paths of the GPU module: the variables a factor is built under (IPO_HIP_TAIL_DENSITY=1 with each)
PATHS = {
    "default": {},
    "sf0": {"IPO_HIP_SF": "0"},
    "sfw1": {"IPO_HIP_SF_WIDTH": "1"},
    "merge0": {"IPO_HIP_SF": "0", "IPO_HIP_MERGE_LEVELS": "0"},
    "leaf8": {"IPO_HIP_SF": "0", "IPO_HIP_SMALL_LEAVES": "1"},
    "split1": {"IPO_HIP_PANEL_SPLIT": "1"},
    "flat2": {"IPO_HIP_GATHER_FLAT": "2"},
    "occ1": {"IPO_HIP_UPDATE_OCC": "1"},
    "xcd1": {"IPO_HIP_UPDATE_XCD": "1"},
    "panel0": {"IPO_HIP_PANEL": "0"},
    "chunk16": {"IPO_HIP_MIN_CHUNK": "16"},
    "visits": {"IPO_HIP_VISITS": "1"},
    "visits_noquad": {"IPO_HIP_VISITS": "1", "IPO_HIP_GATHER_QUAD": "0"},
    "vslots16": {"IPO_HIP_VISITS": "1", "IPO_HIP_VISIT_SLOTS": "16"},
}
# occ1, xcd1 and panel0 choose kernels at launch: the schedule is the default's
SAME_SCHEDULE = ("occ1", "xcd1", "panel0")
CONTROLLED = sorted({v for e in PATHS.values() for v in e} | {"IPO_HIP_TAIL_DENSITY"})

KINDS = ("Chunked", "Plain", "Leaf8", "Merged", "Leaf", "Pre", "SyncFree", "TailGather", "TailLead", "TailChain",
         "TailPair", "TailBlock", "TailDscale")       # SweepKind (kkt_schedule.h)
LEVEL_KINDS = KINDS[:5]
NAMES = ["plan.dims", "plan.col0", "plan.rowptr", "plan.level_ptr", "panels.fu_ptr", "panels.small_ptr",
         "panels.small1_cnt", "panels.split_level", "chunks.chunk_ptr", "order.leaf_cnt", "order.leaf8_cnt", "sf.dims",
         "gather.ck_kind", "gather.ck_ptr", "gather.sp_n", "sweep.fwd", "sweep.bwd"]


class Env:
    """The controlled variables set to exactly `env` and IPO_HIP_TAIL_DENSITY=1
    (the others unset) for a block; the library reads them when a schedule or
    a factor is built."""

    def __init__(self, env):
        self.env = dict(env, IPO_HIP_TAIL_DENSITY="1")

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


@functools.lru_cache(maxsize=None)
def lp(sid):
    return kkt_ref.make_lp("blocks", SHAPES[sid], SEED)


def structure(sid, path):
    """What shape `sid` realises on path `path`, read from the schedule a
    device factor built under that path's variables would build."""
    p = lp(sid)
    with Env(PATHS[path]):
        d = ipo_amd.kkt_schedule(p.m, p.n, p.kA, p.iA, NAMES)
    T, nsup, nlevels, tail_c0, nt, ntb = (int(x) for x in d["plan.dims"])
    nc, hb = np.diff(d["plan.col0"]), np.diff(d["plan.rowptr"])
    assert len(nc) == len(hb) == nsup and T == p.m + p.n and tail_c0 + nt == T and int(nc.sum()) == tail_c0
    sups = {}
    for k in zip(nc.tolist(), hb.tolist()):
        sups[k] = sups.get(k, 0) + 1
    per_level = lambda a: tuple(int(x) for x in np.diff(a))      # noqa: E731
    kinds = lambda a: tuple(KINDS[k] for k in a.reshape(-1, 5)[:, 0])       # noqa: E731
    return dict(
        sups=sups, nt=nt, widths=per_level(d["plan.level_ptr"]),
        # per level: fused panel units, small panels, of them eight to a wave
        panels=tuple(zip(per_level(d["panels.fu_ptr"]), per_level(d["panels.small_ptr"]),
                         (int(x) for x in d["panels.small1_cnt"]))),
        split_levels=tuple(int(x) for x in np.flatnonzero(d["panels.split_level"])),
        chunks=per_level(d["chunks.chunk_ptr"]),
        leaves=tuple(zip((int(x) for x in d["order.leaf_cnt"]), (int(x) for x in d["order.leaf8_cnt"]))),
        sf_level=int(d["sf.dims"][0]), fwd=kinds(d["sweep.fwd"]), bwd=kinds(d["sweep.bwd"]),
        ck_kind=tuple(int(x) for x in d["gather.ck_kind"]), ck=per_level(d["gather.ck_ptr"]), sp_n=tuple(int(x) for x in d["gather.sp_n"]))


# PINS[sid] = (the default path's structure, {path: the keys that differ from it}); a generated table:
# `python tests/test_sparse_shapes.py --write-pins` rewrites it from what the schedule realises (dump_pins below).
# Regenerate only after a deliberate change of a threshold or of SHAPES, and read the diff: it is the pin.
try:
    from sparse_shapes_pins import PINS  # noqa: E402
except ImportError:     # only while the table is being written for the first time
    PINS = {}


def pinned(sid, path):
    base, diff = PINS[sid]
    return dict(base, **diff.get(path, {}))


def check_pinned(sid, path):
    """the realised structure of (sid, path) is the pinned one (the GPU module
    re-asserts this before it builds a factor)"""
    got, want = structure(sid, path), pinned(sid, path)
    for k in want:
        assert got[k] == want[k], (sid, path, k, got[k], want[k])
    assert set(got) == set(want)


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("sid", SHAPE_IDS)
def test_structure_pinned(sid, path):
    """The supernodes (columns, rows below), the tail, the panels of every
    level, the two step lists, the gather kinds and the split units that
    each shape is there for, on the default path and on every path that
    changes the schedule."""
    check_pinned(sid, path)
    if path in SAME_SCHEDULE:
        assert path not in PINS[sid][1]
    base = PINS[sid][0]
    # the plan does not depend on the path
    assert all(k not in v for v in PINS[sid][1].values() for k in ("sups", "nt", "widths", "chunks"))
    assert sum(n * c for (n, _), c in base["sups"].items()) + base["nt"] == lp(sid).m + lp(sid).n <= 720


def has_sup(sid, nc, hb):
    return PINS[sid][0]["sups"].get((nc, hb), 0) > 0


def test_edges_realised():
    """The kernels' own edges, on the shapes named for them."""
    # small panel: nc <= 16 and h <= 64
    s = PINS["small"][0]
    assert all(has_sup("small", nc, 3) for nc in (15, 16, 17))
    assert s["widths"][1] == 3 and s["panels"][1] == (1, 2, 0)          # 17 columns fused, 15 and 16 small
    # panel heights 63 ... 66 and leaves of at most 64 rows below; widths 62, 63, 64 and one split into panels
    s = PINS["leafh"][0]
    assert all(s["sups"][(1, hb)] == 66 for hb in (62, 63, 64, 65))
    assert s["panels"][0] == (2 * 66, 2 * 66 + 7, 0) and s["leaves"][0] == (3 * 66 + 7, 0)
    assert all(has_sup("leafh", nc, 3) for nc in (62, 63, 64)) and has_sup("leafh", 64, 4) and has_sup("leafh", 4, 0)
    # h = 128 and 129: max(1, tiles - 1) = 1 and 2 fused units; 128 rows below are not chunked, 129 are
    s = PINS["rows128"][0]
    assert s["sups"][(1, 127)] == s["sups"][(1, 128)] == 139 and s["panels"][0] == (139 + 2 * 139, 0, 0)
    assert s["chunks"] == (0, 0) and s["nt"] == 129
    s = PINS["rows129"][0]
    assert s["sups"][(1, 128)] == s["sups"][(1, 129)] == 139 and s["panels"][0] == (2 * 139 + 2 * 139, 0, 0)
    assert s["chunks"] == (2 * 139 + 3 * 139, 0) and s["nt"] == 130
    assert pinned("rows129", "sf0")["fwd"][0] == "Chunked" and pinned("rows128", "sf0")["fwd"][0] == "Plain"
    # small leaves: 8 and 9 rows below; an update list of more than 8 entries
    s = pinned("leaf8", "leaf8")
    assert has_sup("leaf8", 1, 8) and has_sup("leaf8", 1, 9) and PINS["leaf8"][0]["sups"][(1, 3)] == 2
    n8 = sum(c for (nc, hb), c in s["sups"].items() if nc == 1 and hb <= 8) - 2
    assert s["leaves"][0] == (n8 + s["sups"][(1, 9)], n8) and s["leaves"][1] == (2, 1)
    assert s["panels"][0][2] == sum(c for (nc, hb), c in s["sups"].items() if nc == 1 and hb <= 7) - 2
    assert s["panels"][1][2] == 2
    assert s["fwd"] == ("Leaf8", "Leaf", "Leaf8", "Merged", "Plain")
    # k-slot counts around kSlab: the leaves of a block are its supernode's sources
    p = lp("kslots")
    with Env({}):
        k = ipo_amd.kkt_schedule(p.m, p.n, p.kA, p.iA, ["plan.kslot", "plan.kslot_ptr"])
    ptr = k["plan.kslot_ptr"]
    assert np.all(np.diff(ptr) % 16 == 0)
    real = sorted(int((k["plan.kslot"][a:b] >= 0).sum()) for a, b in zip(ptr[:-1], ptr[1:]) if b > a)
    assert real == [15, 16, 17, 31, 32, 33, 179]
    # quadrant edges: tiles of 31 ... 35 rows and 29 ... 33 columns, gathered by k_update_quad
    assert all(has_sup("quad", nc, 2) for nc in (29, 30, 31, 32, 33))
    assert pinned("quad", "visits")["ck_kind"] == (0, 2, 2, 0) and pinned("quad", "visits_noquad")["ck_kind"] == (0, 1, 1, 0)
    # the quadrant gathers' bitwise partners: the flat schedule splits no unit the quadrant schedule gathers whole
    assert all(has_sup("quad0", nc, 0) for nc in (29, 30, 31, 32, 33)) and has_sup("quad31", 31, 2)
    for sid in ("quad0", "quad31"):
        assert 2 in pinned(sid, "visits")["ck_kind"] and 2 not in pinned(sid, "visits_noquad")["ck_kind"]
        assert pinned(sid, "visits")["sp_n"] == pinned(sid, "visits_noquad")["sp_n"] == ()
    assert pinned("quad", "visits_noquad")["sp_n"] != pinned("quad", "visits")["sp_n"]
    # four fused units of one supernode alone on its level
    s = pinned("split", "split1")
    assert has_sup("split", 64, 193) and s["panels"][1] == (4, 0, 0) and s["split_levels"] == (1,)
    assert PINS["split"][0]["split_levels"] == ()


def test_every_kernel_choice_is_reached():
    """Over the whole table: every level kind of the sweeps, the pre-pass and
    the sync-free launch, each gather kind, a unit split at least four ways,
    a split level and eight-to-a-wave panels occur on some shape and path, so
    a change of thresholds cannot silently empty the GPU module."""
    kinds, ck, sp, split, small1 = set(), set(), 0, False, 0
    for sid in SHAPE_IDS:
        for path in PATHS:
            s = pinned(sid, path)
            kinds |= set(s["fwd"]) | set(s["bwd"])
            ck |= set(s["ck_kind"][1:])
            sp = max([sp, *s["sp_n"]])
            split |= bool(s["split_levels"])
            small1 = max([small1, *(p[2] for p in s["panels"])])
    assert kinds >= set(LEVEL_KINDS) | {"Pre", "SyncFree", "TailGather", "TailLead", "TailChain"}, kinds
    assert ck == {0, 1, 2} and sp >= 4 and split and small1 > 0


def test_xcd_order_is_a_bijection():
    """IPO_HIP_UPDATE_XCD=1 walks the chunks of every gather launch through
    xcd_chunk (kkt_kernels.h).  This checks a restatement of its formula, not
    the device function: a bijection on [0, G) for launches smaller than one
    round of eight and with every remainder, which is why the GPU module may
    set the knob to 1 on launches of two or three chunks.  A change to the
    header does not fail this test; the check of the device's walk is path
    xcd1 in tests A and B of tests/test_gpu_sparse_shapes.py."""
    def xcd_chunk(b, G):
        q, r, x, i = G >> 3, G & 7, b & 7, b >> 3
        return (x * (q + 1) if x < r else r * (q + 1) + (x - r) * q) + i
    for G in range(1, 700):
        assert sorted(xcd_chunk(b, G) for b in range(G)) == list(range(G)), G


@functools.lru_cache(maxsize=None)
def oracle_case(sid, kind):
    """The oracle on case (sid, SEED, kind) under its three summation orders
    (tests/test_tail_shapes.py: oracle_case)."""
    c = kkt_ref.case("blocks", SHAPES[sid], SEED, kind)
    L = oracle_lib.lib()
    runs = []
    try:
        for order in (0, 1, 2):
            L.orc_set_perturb(order)
            o = oracle_lib.OracleKkt(c.p)
            o.factor(c.E, c.D)
            assert np.array_equal(o.perm(), c.perm)
            y, x, _ = o.solve(c.E, c.D, c.fy, c.fx)
            runs.append((o.info()["ndep"], o.live().copy(), o.diag().copy(), (y, x), o.info()["passes"]))
    finally:
        L.orc_set_perturb(0)
    dpiv = [c.pivot_distance(r[2]) for r in runs]
    dsol = [c.solution_distance(*r[3]) for r in runs]
    return dict(runs=runs, pivot=dpiv, solution=dsol, passes=max(r[4] for r in runs))


@pytest.mark.parametrize("kind", SCALINGS)
@pytest.mark.parametrize("sid", SHAPE_IDS)
def test_oracle_against_reference(sid, kind):
    """The fp64 oracle under its three summation orders: no dependent pivot,
    every node live, one refinement pass at unit scaling and at most two at
    wide scaling; its pivot and solution distances from the long-double
    reference are printed.  The GPU module's bounds are multiples of these
    distances, so a reference or oracle gone wrong must not widen them
    unnoticed: at unit scaling they stay inside the suite's own oracle bars
    for well-scaled systems (1e-9 and 1e-8, tests/test_gpu_kkt.py)."""
    o = oracle_case(sid, kind)
    for ndep, live, _, _, passes in o["runs"]:
        assert ndep == 0
        assert live.all()
        assert passes == 1 if kind == "unit" else 1 <= passes <= 2
    print(f"{sid} {kind}: oracle pivot distance {['%.2e' % v for v in o['pivot']]}, "
          f"solution distance {['%.2e' % v for v in o['solution']]}, passes {[r[4] for r in o['runs']]}")
    assert 0 < max(o["pivot"]) < np.inf and max(o["solution"]) < np.inf
    if kind == "unit":
        assert max(o["pivot"]) <= 1e-9
        assert max(o["solution"]) <= 1e-8


@functools.lru_cache(maxsize=None)
def oracle_hsd(sid):
    """The oracle's HSD solve of shape `sid` under its three summation orders."""
    L = oracle_lib.lib()
    out = []
    try:
        for order in (0, 1, 2):
            L.orc_set_perturb(order)
            out.append(oracle_lib.solve_arrays(lp(sid), "hsd"))
    finally:
        L.orc_set_perturb(0)
    return out


def test_solve_paths_reach_every_level_kind():
    """The whole solves of the GPU module (Test D) run the two-right-hand-side
    sweeps: each (shape, path) holds the kinds SOLVE_KINDS says, and between
    them every level kind, the sync-free launch and the tail steps."""
    seen = set()
    for (sid, path), kinds in SOLVE_KINDS.items():
        assert sid in SOLVE_SHAPES
        s = pinned(sid, path)
        assert set(s["fwd"]) == set(kinds) and set(s["bwd"]) >= set(kinds) - {"TailGather", "TailLead"}, (sid, path)
        seen |= set(s["fwd"]) | set(s["bwd"])
    assert seen >= set(LEVEL_KINDS) | {"SyncFree", "TailGather", "TailLead", "TailChain"}, seen


@pytest.mark.parametrize("sid", SOLVE_SHAPES)
def test_solve_shapes_oracle_orders_agree(sid):
    """What makes the whole solves of these LPs a property a device solve can
    be held to: the oracle's three summation orders end with status 0 after
    the same number of iterations, at objectives equal to 1e-9 relative (the
    device is held to 1e-6)."""
    runs = oracle_hsd(sid)
    print(f"{sid}: iterations {[r['iters'] for r in runs]}, pobj {[r['final_pobj'] for r in runs]}")
    assert [r["status"] for r in runs] == [0, 0, 0]
    assert len({r["iters"] for r in runs}) == 1
    for key in ("final_pobj", "final_dobj"):
        v = [r[key] for r in runs]
        assert max(v) - min(v) <= 1e-9 * max(1.0, abs(v[0]))


# ------------------------------------------------------------ the pins' writer
_PIN_KEYS = ("sups", "nt", "widths", "panels", "split_levels", "chunks", "leaves", "sf_level", "fwd", "bwd", "ck_kind",
             "ck", "sp_n")
_PIN_DOC = '''"""What the shapes of tests/test_sparse_shapes.py realise, pinned: per shape the structure on the default
path, then for each path of the GPU module that builds another schedule the entries that differ.  Written by
`python tests/test_sparse_shapes.py --write-pins` (dump_pins there); not edited by hand.

sups: (columns, rows below) -> supernodes; nt: tail size; widths: supernodes per level; panels: per level
(fused units, small panels, of them eight to a wave); split_levels: levels on k_diag + k_trsm; chunks: solve
chunks per level; leaves: per level (leaves, of them small); sf_level: first level of the sync-free range;
fwd, bwd: the kinds of the two step lists; ck_kind: per gather group 0 k_update, 1 k_update_flat,
2 k_update_quad; ck: its chunks (workgroups); sp_n: chunks of every split unit (sparse levels, then the tail)."""'''


def _wrap(items, ind, width=116):
    lines, cur = [], ""
    for it in items:
        if cur and len(cur) + len(it) + 2 + ind > width:
            lines.append(cur.rstrip())
            cur = ""
        cur += it + ", "
    lines.append(cur.rstrip().rstrip(","))
    return ("\n" + " " * ind).join(lines)


def _entry(d, ind):
    out = []
    for k in _PIN_KEYS:
        if k not in d:
            continue
        head, v = f'"{k}": ', d[k]
        if isinstance(v, dict):
            text = "{" + _wrap([f"{key}: {c}" for key, c in sorted(v.items())], ind + len(head) + 1) + "}"
        elif isinstance(v, tuple) and len(repr(v)) + ind + len(head) > 112:
            text = "(" + _wrap([repr(x) for x in v], ind + len(head) + 1) + ("," if len(v) == 1 else "") + ")"
        else:
            text = repr(v)
        out.append(head + text)
    return "{\n" + " " * ind + (",\n" + " " * ind).join(out) + ",\n" + " " * (ind - 4) + "}"


def dump_pins():
    """The text of tests/sparse_shapes_pins.py for what the schedule realises now."""
    lines = [_PIN_DOC, "PINS = {"]
    for sid in SHAPE_IDS:
        base = structure(sid, "default")
        lines.append(f'    "{sid}": ({_entry(base, 8)}, {{')
        for path in PATHS:
            diff = {k: v for k, v in structure(sid, path).items() if v != base[k]}
            if diff:
                lines.append(f'        "{path}": {_entry(diff, 12)},')
        lines.append("    }),")
    return "\n".join(lines + ["}"]) + "\n"


if __name__ == "__main__":
    if sys.argv[1:] != ["--write-pins"]:
        sys.exit("usage: python tests/test_sparse_shapes.py --write-pins")
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "sparse_shapes_pins.py"), "w") as f:
        f.write(dump_pins())
