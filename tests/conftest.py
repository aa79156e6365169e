"""pytest configuration: markers, shared paths and fixtures.

`-m "not gpu"` runs here (no GPU): oracle vs golden traces, front end,
symbolic analysis, ABI exports, multi-rank harness.  `-m gpu` runs on the
MI355X box: HIP path vs the oracle / golden traces through the C ABI.
"""
import gzip
import os
import shutil
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "linear-programming-vanderbei_amd")
GOLDEN = os.path.join(REPO, "tests", "golden", "netlib")
for p in (REPO, PKG, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs an MI355X (runs through libipo_hip.so on the device)")
    config.addinivalue_line("markers", "slow: long CPU oracle runs (set IPO_SLOW=1)")


def pytest_collection_modifyitems(config, items):
    if os.environ.get("IPO_SLOW") == "1":
        return
    skip = pytest.mark.skip(reason="slow oracle run; set IPO_SLOW=1")
    for it in items:
        if "slow" in it.keywords:
            it.add_marker(skip)


# per user: a cache left behind by another user is not writable
_MPS_CACHE = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"ipo_hip_mps_cache_{os.getuid()}")


def mps_path(name: str) -> str:
    """Decompress tests/golden/netlib/<name>.mps.gz once and return its path."""
    os.makedirs(_MPS_CACHE, exist_ok=True)
    dst = os.path.join(_MPS_CACHE, name + ".mps")
    if not os.path.exists(dst):
        src = os.path.join(GOLDEN, name + ".mps.gz")
        tmp = dst + f".{os.getpid()}.tmp"
        with gzip.open(src, "rb") as fi, open(tmp, "wb") as fo:
            shutil.copyfileobj(fi, fo)
        os.replace(tmp, dst)
    return dst


def golden_trace(name: str) -> str:
    with open(os.path.join(GOLDEN, name + ".mps.sol")) as fh:
        return fh.read()


def available_problems():
    return sorted(f[:-7] for f in os.listdir(GOLDEN) if f.endswith(".mps.gz"))
