"""bench.py's command line: a plain run does the headline solves alone,
--dump-outputs writes what the last timed solve left for its caller, --full
adds the other legs.  The GPU test runs the benchmark itself (afiro, 2
solves: about a second)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO, mps_path

FULL_ONLY = ("end_to_end", "intpt_25fv47", "banded", "hbm_roofline", "block_angular")


def test_dump_outputs_writes_float64_arrays(tmp_path):
    """dump_outputs on a stand-in context: one float64 .npy per vector, the
    objectives beside them, the directory created."""
    sys.path.insert(0, REPO)
    import bench

    class Ctx:
        def solution(self):
            return (np.arange(5.0), np.arange(3.0) - 1, np.zeros(3), np.ones(5, np.float32))

    d = tmp_path / "a" / "b"
    bench.dump_outputs(str(d), Ctx(), {"final_pobj": -1.5, "final_dobj": -1.25})
    assert sorted(os.listdir(d)) == ["objective.npy", "w.npy", "x.npy", "y.npy", "z.npy"]
    for name, want in zip("xywz", Ctx().solution()):
        got = np.load(d / (name + ".npy"))
        assert got.dtype == np.float64 and np.array_equal(got, want)
    assert np.array_equal(np.load(d / "objective.npy"), [-1.5, -1.25])


def test_full_is_off_by_default():
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--help"], capture_output=True, text=True)
    assert out.returncode == 0
    assert "--full" in out.stdout and "--dump-outputs" in out.stdout


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_solution(tmp_path):
    """A plain run on afiro: --steps sets the number of timed solves, the line
    carries the headline keys and none of the --full legs, and the dump is
    bitwise the solution of the same solve on a Context of this process
    (consecutive solves are identical, test_gpu_ipm)."""
    import ipo_amd
    d = tmp_path / "dump"
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "0",
                          "--problem", "afiro", "--dump-outputs", str(d)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["steps"] == 2 and len(line["config"]["iterations_per_solve"]) == 2
    assert line["metric_condition_met"] and line["value"] > 0
    assert line["unit"] == "iterations/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    iters = sum(line["config"]["iterations_per_solve"])
    assert line["ms_per_step"] == pytest.approx(1e3 * iters / line["value"] / 2, rel=1e-9)
    assert line["roofline"] is None and line["cpu_baseline"] is None and not line["phases"]
    assert not any(k in line for k in FULL_ONLY)

    p = ipo_amd.load_mps(mps_path("afiro"))
    ctx = ipo_amd.Context(p)
    try:
        status, st, _ = ctx.run("hsd")
        sol = ctx.solution()
    finally:
        ctx.close()
    assert status == 0
    for name, want in zip("xywz", sol):
        got = np.load(d / (name + ".npy"))
        assert got.dtype == np.float64 and np.array_equal(got, want), name
    assert np.array_equal(np.load(d / "objective.npy"), [st["final_pobj"], st["final_dobj"]])
