"""Host side of the trailing forward tail lead (IPO_HIP_LEAD_TRAIL, DESIGN.md
section 6.6; host code, no GPU).

SweepSteps::lead_end ("sweep.lead_end" of ipo_hip_kkt_schedule) is where a
solve's first sweep starts when the pre-pass also ran the tail lead: the step
after the forward list's TailLead, and 0 exactly when the list has none.

The trailing lead reads block column t of the tail once k_tail_run's counter
cdone[t] has reached lead_col_target(nt, t) (ipo_hip_lead_col_targets).  Every
panel item of step t in the run's schedule adds one to that counter, and
nothing else does, so the target must be the number of panel items the
schedule holds for step t -- fewer would let the lead read an unfinished
column, more would leave it waiting for ever."""
import ctypes as C
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "linear-programming-vanderbei_amd"))
import ipo_amd  # noqa: E402
from conftest import mps_path  # noqa: E402

PC = 64
K_LEAD = 2          # kLeadBlocks (kkt_sweep.hip): block K + 1 is the first with a helper
TAIL_GATHER, TAIL_LEAD, TAIL_CHAIN = 7, 8, 9     # SweepKind (kkt_schedule.h)
SWEEP_KNOBS = ("IPO_HIP_VISITS", "IPO_HIP_MERGE_LEVELS", "IPO_HIP_SMALL_LEAVES", "IPO_HIP_SF", "IPO_HIP_CHAIN_PAIRS",
               "IPO_HIP_CHAIN_LEAD")


def sweep(name, monkeypatch, env=()):
    for k in SWEEP_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env:
        monkeypatch.setenv(k, v)
    p = ipo_amd.load_mps(mps_path(name))
    d = ipo_amd.kkt_schedule(p.m, p.n, p.kA, p.iA, ["sweep.fwd", "sweep.split", "sweep.lead_end"])
    assert d["sweep.lead_end"].size == 1
    return d["sweep.fwd"].reshape(-1, 5)[:, 0].tolist(), int(d["sweep.split"][0]), int(d["sweep.lead_end"][0])


@pytest.mark.parametrize("name", ["dfl001", "25fv47", "brandy"])
def test_lead_end_is_one_past_the_tail_lead(name, monkeypatch):
    kinds, split, lead_end = sweep(name, monkeypatch)
    assert kinds.count(TAIL_LEAD) == 1
    assert lead_end == kinds.index(TAIL_LEAD) + 1
    assert lead_end == split + 1 and lead_end == len(kinds)     # the lead closes the forward list


@pytest.mark.parametrize("name,env", [("afiro", ()), ("dfl001", (("IPO_HIP_CHAIN_LEAD", "0"),))])
def test_no_tail_lead_no_lead_end(name, env, monkeypatch):
    """no tail, and the per-block chain in the lead's place"""
    kinds, split, lead_end = sweep(name, monkeypatch, env)
    assert TAIL_LEAD not in kinds
    assert lead_end == 0 and split == 0


def targets(nt):
    f = ipo_amd.lib().ipo_hip_lead_col_targets
    f.argtypes = [C.c_int, C.POINTER(C.c_int), C.c_int]
    f.restype = C.c_int
    ntb = f(nt, None, 0)
    assert ntb == (nt + PC - 1) // PC, ipo_amd.last_error()
    out = (C.c_int * ntb)()
    assert f(nt, out, ntb) == ntb
    return list(out)


def panel_items(nt, K=4, L=4, cap=256):
    f = ipo_amd.lib().ipo_hip_tail_run_schedule
    f.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint), C.c_int, C.POINTER(C.c_int)]
    f.restype = C.c_int
    n = f(nt, K, L, cap, None, 0, None)
    assert n > 0, ipo_amd.last_error()
    ntb = (nt + PC - 1) // PC
    items = (C.c_uint * (2 * n))()
    ptr = (C.c_int * (ntb + 1))()
    assert f(nt, K, L, cap, items, n, ptr) == n
    count = [0] * ntb
    for i in range(n):
        y = items[2 * i + 1]
        if y >> 31:
            count[y & 0xff] += 1
    return count


# ntb = 1, 2, 3 (no helper), K + 1 = 3, K + 2 = 4 (the first helper), ragged last blocks, a small
# cap (first chunks moved between launches), and dfl001's 70 block columns
@pytest.mark.parametrize("nt", [1, 37, 64, 65, 128, 129, 191, 192, 193, 256, 70 * 64 - 13])
@pytest.mark.parametrize("cap", [256, 8])
def test_targets_are_the_steps_panel_items(nt, cap):
    ntb = (nt + PC - 1) // PC
    assert {1: 1, 64: 1, 65: 2, 128: 2, 129: 3, 192: 3, 193: 4, 256: 4}.get(nt, ntb) == ntb
    want = panel_items(nt, cap=cap)
    got = targets(nt)
    assert got == want
    assert all(g >= 1 for g in got)


def test_first_helper_block():
    """K + 2 block columns is the smallest tail with a helper: the cases above cover both sides of it"""
    assert (193 + PC - 1) // PC == K_LEAD + 2 and (192 + PC - 1) // PC == K_LEAD + 1


def test_targets_reject_bad_size():
    f = ipo_amd.lib().ipo_hip_lead_col_targets
    f.argtypes = [C.c_int, C.POINTER(C.c_int), C.c_int]
    f.restype = C.c_int
    assert f(0, None, 0) == -1
