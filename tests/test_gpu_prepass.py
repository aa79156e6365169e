"""The forward pre-pass of the overlapped HSD iteration (KktDevice::PrePass,
IPO_HIP_PREPASS, default on): the factorisation enqueues the first solve's
maxbc reduction, k_perm_in2 and the forward steps up to k_tail_gather on the
side stream beside the dense tail's factor, and the solve starts its first
sweep at the tail lead.  The kernels, their arguments and their order are the
sequential pass's, so a solve with the pre-pass is bit for bit the solve
without it (IPO_HIP_PREPASS=0): status, trace text, iteration count and final
values.  A pre-pass is used only when the factorisation's first pass stood
with no dropped pivot; dfl001's last iterations drop pivots and repair the
tail, so both the use and the discard run there."""
import functools
import os
import re

import pytest

import ipo_amd
from conftest import mps_path

pytestmark = pytest.mark.gpu


def _with_env(var, val, fn):
    old = os.environ.get(var)
    os.environ[var] = val
    try:
        return fn()
    finally:
        if old is None:
            del os.environ[var]
        else:
            os.environ[var] = old


def _solve_env(var, val, name="dfl001", extra=()):
    def run():
        return ipo_amd.run_mps(mps_path(name), "hsd")
    fn = run
    for v2, x2 in extra:
        fn = (lambda f, v2=v2, x2=x2: (lambda: _with_env(v2, x2, f)))(fn)
    status, text, st = _with_env(var, val, fn)
    return status, text, {k: st[k] for k in sorted(st) if k.startswith("final") or k == "iters"}


@functools.lru_cache(maxsize=None)
def _solve(name, prepass, extra=()):
    """one HSD solve at IPO_HIP_PREPASS=prepass (computed once, shared, never changed)"""
    return _solve_env("IPO_HIP_PREPASS", prepass, name, extra)


def _counts(err):
    m = re.search(r"kkt: forward pre-passes used (\d+), discarded (\d+)", err)
    assert m, err
    return int(m.group(1)), int(m.group(2))


@pytest.mark.parametrize("name", ["dfl001", "25fv47", "brandy", "afiro"])
def test_prepass_bitwise(name):
    """Tails of 70 block columns (dfl001: its last iterations have ndep > 0
    and two tail repairs, the discard path), 7 (25fv47) and 3 (brandy: no
    helper workgroups of the lead), and no tail (afiro: the path is inactive)."""
    off, on = _solve(name, "0"), _solve(name, "1")
    assert off[0] == on[0]
    assert off[1] == on[1]
    assert off[2] == on[2]


def test_prepass_forced_repairs_bitwise():
    """IPO_HIP_TAIL_SPEC=2: every speculated drop of the look-ahead tail fails
    its check, restores and goes to the host repair; those factorisations
    discard their pre-pass."""
    spec = (("IPO_HIP_TAIL_SPEC", "2"),)
    assert _solve("dfl001", "0", spec) == _solve("dfl001", "1", spec)


def test_prepass_used_and_discarded(capfd):
    """The path is taken: of dfl001's 117 iterations more than half use their
    pre-pass, and at least one discards it (conditions on the mechanism, not
    measurements).  The counts come with IPO_HIP_DEBUG_REDO's line when the
    solver is destroyed."""
    capfd.readouterr()
    got = _solve_env("IPO_HIP_PREPASS", "1", "dfl001", (("IPO_HIP_DEBUG_REDO", "1"),))
    used, discarded = _counts(capfd.readouterr().err)
    print("pre-passes used", used, "discarded", discarded, "iterations", got[2]["iters"])
    assert got == _solve("dfl001", "1")
    assert used > 117 / 2
    assert discarded >= 1
    assert used + discarded <= got[2]["iters"] + 1     # one per factorisation; the last one's is never used


def test_prepass_inactive_without_overlap(capfd):
    """The sequential iteration (IPO_HIP_OVERLAP=0) requests no pre-pass:
    IPO_HIP_PREPASS=1 changes nothing there, and the solve is the default one."""
    capfd.readouterr()
    seq = _solve_env("IPO_HIP_PREPASS", "1", "dfl001", (("IPO_HIP_OVERLAP", "0"), ("IPO_HIP_DEBUG_REDO", "1")))
    assert _counts(capfd.readouterr().err) == (0, 0)
    assert seq == _solve("dfl001", "1")
