"""The device factor, bit for bit, against a recording of an earlier commit.

The bitwise tests of tests/test_gpu_tail_shapes.py and tests/test_gpu_panel.py
compare paths that all go through the same visit_tile512 (kkt_dense.hip), so
an error inside it -- a row pair staged one row off, a pivot broadcast from
the wrong lane, a masked element of a diagonal tile stored -- moves every
path alike and they still agree with one another.  This module compares with
something outside the build: tests/golden/visit_bits_parent.json holds, per
case, the SHA-256 of the bytes of KktFactor.pivots()[0] and of the refined
(y, x) of solve(), recorded on an MI355X by tools/record_visit_bits.py from a
build of the commit named in the file.  A change to the visits that keeps
every product and every sum (thread mapping, access width, instruction
order) keeps these bits; one that is meant to change them records the file
again and says so.  The test never builds or reads that commit.

Cases (tests/test_tail_shapes.py's shapes, the smallest at which each piece
of the visit's operand path can go wrong), at both scalings, on the
persistent run and on one launch per step, chunks pinned at 4 / 4:
  S1-nt256, S1-nt257   even and odd leading dimension: every operand column
                       16-byte aligned / every second one 8 bytes off;
  S1-nt321             6 block columns, the first tail with a chunk of more
                       than one block; last block of 1 row;
  S1-nt577             10 block columns, full chunks of four; the last row
                       block has 1 row, so a row pair straddles nt - 1;
  S1-nt145, S1-nt193   last blocks of 17 rows and of 1 row;
  S3-r200-dflt         nt 506: a gather below the tail, last block of 58 rows;
  S2-127x135           nt 262: the whole matrix as the tail.
"""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import ipo_amd
import kkt_ref
from test_gpu_tail_shapes import BY_ID, PATHS, _Env, _factor_solve
from test_tail_shapes import SCALINGS, SEED

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "visit_bits_parent.json")
SIDS = ("S1-nt256", "S1-nt257", "S1-nt321", "S1-nt577", "S1-nt145", "S1-nt193", "S3-r200-dflt", "S2-127x135")
BIT_PATHS = ("default", "run0")


def case_key(sid, kind, path):
    return f"{sid}/{kind}/{path}"


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, np.float64).tobytes())
    return h.hexdigest()


def visit_bits(sid, kind, path):
    """A fresh device factor and solve of case (sid, kind) on `path`: the
    hashes the fixture holds, and what the self-check reads."""
    _, family, shape, density, nt = BY_ID[sid]
    c = kkt_ref.case(family, shape, SEED, kind)
    with _Env(PATHS[path], density):
        assert ipo_amd.symbolic_tail(c.p.m, c.p.n, c.p.kA, c.p.iA)["nt"] == nt
        k = ipo_amd.KktFactor(c.p.m, c.p.n, c.p.kA, c.p.iA, c.p.A)
    try:
        g = _factor_solve(k, c)
    finally:
        k.close()
    return dict(pivots=_sha(g["d"]), solution=_sha(g["y"], g["x"]), ndep=int(g["ndep"]),
                live=bool(g["live"].all()), ok=int(g["ok"]))


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


@pytest.mark.parametrize("path", BIT_PATHS)
@pytest.mark.parametrize("kind", SCALINGS)
@pytest.mark.parametrize("sid", SIDS)
def test_factor_bits_recorded(sid, kind, path):
    want = golden()["cases"][case_key(sid, kind, path)]
    g = visit_bits(sid, kind, path)
    assert g["ndep"] == 0 and g["live"] and g["ok"] == 1      # a broken run fails here, not only by hash
    assert g["pivots"] == want["pivots"], "pivots differ from commit " + golden()["commit"]
    assert g["solution"] == want["solution"], "refined solution differs from commit " + golden()["commit"]


def test_fixture_covers_the_cases():
    assert sorted(golden()["cases"]) == sorted(case_key(s, k, p) for s in SIDS for k in SCALINGS for p in BIT_PATHS)
