"""The trailing forward tail lead (IPO_HIP_LEAD_TRAIL):
where the forward pre-pass is eligible, the factorisation also enqueues the
first solve's forward dense-tail sweep, k_tail_fwd_lead in its trailing form,
behind k_tail_run on its stream (1) or beside it on the side stream, reading
each block column once the run's counter says it is final (2).  The
arithmetic is the lead's, so an HSD solve is bit for bit the solve without it
(0): x, y, w, z, the iteration count and the final values, mu among them.

Tails: dense LPs whose whole KKT matrix is the tail, of 2 block columns (nt =
128, the smallest tail a plan forms: no tail of one block column exists), 3
(nt = 129, a last block of one row; no helper workgroup), 4 (nt = 199 and
193: the first helper, ragged last blocks); brandy (3, nt = 155), 25fv47 (7,
nt = 396) and greenbea (12, nt = 732: nine blocks with a helper against the
eight helper workgroups of the launch beside the run, so one of them draws a
second block); dfl001 (70) with forced bails.

A bail of the run (not a fault: a panel's software exit, flags[2]) must end
every poll of the trailing lead: IPO_HIP_TAIL_SPEC=2 makes every speculated
drop of dfl001's tail fail its check, so k_tail_run ends short of its last
column while the lead waits for it (2) or before the lead starts (1).  A poll
that did not end would keep the solve from returning."""
import functools
import os
import re

import numpy as np
import pytest

import ipo_amd
import kkt_ref
from conftest import mps_path
from test_tail_shapes import SEED

pytestmark = pytest.mark.gpu

MODES = ("0", "1", "2")
# name -> (problem, tail density or None, block columns of its tail)
DENSE = {"dense127x135-rho1": ((127, 135), 1.0, 2), "dense60x69": ((60, 69), None, 3),
         "dense90x110": ((90, 110), None, 4), "dense192x200-rho1": ((192, 200), 1.0, 4)}
MPS = {"brandy": 3, "25fv47": 7, "greenbea": 12}


class _Env:
    def __init__(self, env):
        self.env = {k: v for k, v in env.items() if v is not None}
        self.names = list(env)

    def __enter__(self):
        self.old = {v: os.environ.get(v) for v in self.names}
        for v in self.names:
            os.environ.pop(v, None)
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for v, x in self.old.items():
            if x is None:
                os.environ.pop(v, None)
            else:
                os.environ[v] = x


def _problem(name):
    if name in DENSE:
        shape, density, ntb = DENSE[name]
        return kkt_ref.dense_lp(*shape, SEED), density, ntb
    return ipo_amd.load_mps(mps_path(name)), None, MPS.get(name)


def _run(name, mode, extra=()):
    p, density, ntb = _problem(name)
    env = {"IPO_HIP_LEAD_TRAIL": mode, "IPO_HIP_TAIL_DENSITY": None if density is None else repr(density)}
    env.update(dict(extra))
    with _Env(env):
        if ntb is not None:
            assert ipo_amd.symbolic_tail(p.m, p.n, p.kA, p.iA)["ntb"] == ntb      # the tail this case is there for
        r = ipo_amd.solver(p, "hsd")
    st = r["stats"]
    return dict(status=r["status"], x=r["x"], y=r["y"], w=r["w"], z=r["z"], iters=st["iters"],
                final={k: st[k] for k in sorted(st) if k.startswith("final")}, repairs=st["tail_repairs"])


@functools.lru_cache(maxsize=None)
def _solve(name, mode, extra=()):
    """one HSD solve at IPO_HIP_LEAD_TRAIL=mode (computed once, shared, never changed)"""
    return _run(name, mode, extra)


def _same(a, b, what):
    assert a["status"] == b["status"], what
    assert a["iters"] == b["iters"], what
    assert a["final"] == b["final"], what            # mu, objectives, infeasibilities: equal floats
    for key in ("x", "y", "w", "z"):
        assert np.array_equal(a[key], b[key]), (what, key)


def _lead_counts(err):
    m = re.search(r"kkt: trailing leads used (\d+), discarded (\d+)", err)
    assert m, err
    p = re.search(r"kkt: forward pre-passes used (\d+), discarded (\d+)", err)
    assert p, err
    return (int(m.group(1)), int(m.group(2))), (int(p.group(1)), int(p.group(2)))


@pytest.mark.parametrize("name", list(DENSE) + list(MPS))
def test_lead_trail_bitwise(name):
    ref = _solve(name, "0")
    assert ref["status"] == 0
    for mode in ("1", "2"):
        _same(_solve(name, mode), ref, (name, mode))


@pytest.mark.parametrize("mode", ["1", "2"])
@pytest.mark.parametrize("name", ["dense60x69", "dense90x110", "25fv47"])
def test_lead_trail_taken(name, mode, capfd):
    """The path is taken: every pre-pass carries a trailing lead, those that
    stand are used with it, and most of a solve's factorisations use theirs
    (conditions on the mechanism: the counts printed with IPO_HIP_DEBUG_REDO
    when the solver is destroyed).  Mode 0 enqueues none."""
    capfd.readouterr()
    got = _run(name, mode, (("IPO_HIP_DEBUG_REDO", "1"),))
    (used, dropped), (pre_used, pre_dropped) = _lead_counts(capfd.readouterr().err)
    print(name, "mode", mode, "trailing leads used", used, "discarded", dropped, "pre-passes", pre_used, pre_dropped,
          "iterations", got["iters"])
    _same(got, _solve(name, "0"), (name, mode))
    assert (used, dropped) == (pre_used, pre_dropped)
    assert used >= 1
    assert used + dropped <= got["iters"] + 1     # one per factorisation; the last one's is never used
    capfd.readouterr()
    _run(name, "0", (("IPO_HIP_DEBUG_REDO", "1"),))
    (used0, dropped0), (pre_used0, _) = _lead_counts(capfd.readouterr().err)
    assert (used0, dropped0) == (0, 0) and pre_used0 == pre_used


def test_lead_trail_survives_a_bailing_run(capfd):
    spec = (("IPO_HIP_TAIL_SPEC", "2"),)
    ref = _solve("dfl001", "0", spec)
    assert ref["repairs"] > 0, "dfl001's HSD solve no longer bails in the dense tail"
    for mode in ("1", "2"):
        capfd.readouterr()
        got = _run("dfl001", mode, spec + (("IPO_HIP_DEBUG_REDO", "1"),))
        (used, dropped), _ = _lead_counts(capfd.readouterr().err)
        print("dfl001 TAIL_SPEC=2 mode", mode, "trailing leads used", used, "discarded", dropped, "repairs",
              got["repairs"])
        _same(got, ref, ("dfl001 spec 2", mode))
        assert got["repairs"] == ref["repairs"]
        assert dropped >= 1                  # a bailed factorisation drops its lead
        assert used >= 1
