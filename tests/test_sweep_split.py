"""The split point of a substitution sweep's forward list (csrc/kkt_schedule.cpp
sweep_split, SweepSteps::split, through ipo_hip_kkt_schedule as "sweep.split";
host code, no GPU).

KktDevice's forward pre-pass enqueues the forward steps [0, split) beside the
dense tail's factorisation, and the solve that uses it starts its first sweep
at step `split`.  So the steps before the split may read only the sparse
panels and the right-hand side (the kinds that sweep the sparse supernodes --
the level kinds, Pre and SyncFree -- and, last, the TailGather, which sums the
update values those left), and step `split` must be the TailLead.  Where the
list has no such pair -- no tail, or the per-block chain
(IPO_HIP_CHAIN_LEAD=0), which keeps the sequential sweep -- the split is 0."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "linear-programming-vanderbei_amd"))
import ipo_amd  # noqa: E402
from conftest import mps_path  # noqa: E402

# SweepKind (kkt_schedule.h); a step is (kind, q0, n, a, b)
(CHUNKED, PLAIN, LEAF8, MERGED, LEAF, PRE, SYNC_FREE, TAIL_GATHER, TAIL_LEAD, TAIL_CHAIN, TAIL_PAIR, TAIL_BLOCK,
 TAIL_DSCALE) = range(13)
SPARSE_KINDS = (CHUNKED, PLAIN, LEAF8, MERGED, LEAF, PRE, SYNC_FREE)
SWEEP_KNOBS = ("IPO_HIP_VISITS", "IPO_HIP_MERGE_LEVELS", "IPO_HIP_SMALL_LEAVES", "IPO_HIP_SF", "IPO_HIP_CHAIN_PAIRS",
               "IPO_HIP_CHAIN_LEAD")


def schedule(name, monkeypatch, env=()):
    for k in SWEEP_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env:
        monkeypatch.setenv(k, v)
    p = ipo_amd.load_mps(mps_path(name))
    d = ipo_amd.kkt_schedule(p.m, p.n, p.kA, p.iA, ["plan.dims", "sweep.fwd", "sweep.split"])
    nt = int(d["plan.dims"][4])
    kinds = d["sweep.fwd"].reshape(-1, 5)[:, 0].tolist()
    assert d["sweep.split"].size == 1
    return nt, kinds, int(d["sweep.split"][0])


@pytest.mark.parametrize("name", ["dfl001", "25fv47", "brandy"])
def test_split_follows_the_tail_gather(name, monkeypatch):
    nt, kinds, split = schedule(name, monkeypatch)
    assert nt > 0
    assert kinds.count(TAIL_GATHER) == 1
    assert split == kinds.index(TAIL_GATHER) + 1
    assert split >= 2, "a tail gathers what sparse steps left"
    assert all(k in SPARSE_KINDS for k in kinds[:split - 1]), kinds[:split]
    assert kinds[split] == TAIL_LEAD and split == len(kinds) - 1


@pytest.mark.parametrize("env", [(), (("IPO_HIP_SF", "0"),), (("IPO_HIP_MERGE_LEVELS", "0"),)])
def test_split_under_the_sweep_knobs(env, monkeypatch):
    """other shapes of the sparse part of the list: per-level launches only, separate leaf launches"""
    _, kinds, split = schedule("25fv47", monkeypatch, env)
    assert split == kinds.index(TAIL_GATHER) + 1 and kinds[split] == TAIL_LEAD
    assert all(k in SPARSE_KINDS for k in kinds[:split - 1])


def test_no_tail_no_split(monkeypatch):
    nt, kinds, split = schedule("afiro", monkeypatch)
    assert nt == 0 and TAIL_GATHER not in kinds
    assert split == 0


def test_chain_path_has_no_split(monkeypatch):
    """IPO_HIP_CHAIN_LEAD=0: the per-block chain follows the gather; that path keeps the sequential sweep"""
    _, kinds, split = schedule("dfl001", monkeypatch, (("IPO_HIP_CHAIN_LEAD", "0"),))
    assert kinds[kinds.index(TAIL_GATHER) + 1] == TAIL_CHAIN
    assert split == 0
