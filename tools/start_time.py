#!/usr/bin/env python3
"""Time the start rule "mehrotra" against the default start on one build
(DESIGN.md section 10.4): a method's run from "every variable 1000" and under
the rule, on netlib LPs and on tools/qp_dense_time.py's factor QP.

The protocol of section 10.1, as tools/pc_time.py: one persistent context per
problem; per leg one warm-up solve with the trace (its lines are counted),
then `--repeats` solves timed by the solver's own clock around the iteration
loop (t_solve_s, which under the rule includes the start's factorisation and
two solves) and `--repeats` more in timing mode for the device time of the
factorisations and the refined solves (HIP events), given per Newton system.
The start's own time is the wall time of Context.start_point("mehrotra") on
a synchronised device, the download of the four vectors included.  One JSON
line per problem and leg with the medians and the spread (min, max); a leg is
recorded whatever its status.

--pkg DIR: the package directory (the one that holds ipo_amd/ and lib/) of
the build to time -- this checkout's by default.  A build from before the
rule has no Context.set_start_rule: only its default legs are run, which is
how the parent commit is timed alternately in one session to show that the
default start did not move.

usage: start_time.py [--pkg DIR] [--label L] [--repeats R] --method pc netlib:25fv47 factor:2048 netlib:dfl001
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def leg(ctx, method, repeats):
    st, s, text = ctx.run(method, trace=True)                  # warm-up
    lines = sum(1 for ln in text.splitlines() if ln[:9].strip().isdigit())
    plain = [ctx.run(method)[1] for _ in range(repeats)]
    timed = [ctx.run(method, timing=True)[1] for _ in range(repeats)]
    systems = max(s["factors"], 1)                             # factorisations: the Newton systems, and the start's one
    return {"status": st, "lines": lines, "factors": s["factors"], "solves": s["solves"],
            "refine_passes": s["refine_passes"],
            "t_solve_s": spread([r["t_solve_s"] for r in plain]),
            "ms_per_line": spread([1e3 * r["t_solve_s"] / max(lines, 1) for r in plain]),
            "kkt_ms_per_factor": spread([(r["factor_ms"] + r["solve_ms"]) / systems for r in timed])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pkg", default=os.path.join(REPO, "linear-programming-vanderbei_amd"))
    ap.add_argument("--label", default="")
    ap.add_argument("--method", required=True)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("problems", nargs="+", help="netlib:NAME or factor:N")
    a = ap.parse_args()
    sys.path[:0] = [os.path.abspath(a.pkg), os.path.join(REPO, "tools")]
    import ipo_amd
    import pc_time                  # netlib() only
    import qp_dense_time            # make_problem only (it imports ipo_amd: the one chosen above)
    assert os.path.dirname(os.path.dirname(os.path.abspath(ipo_amd.__file__))) == os.path.abspath(a.pkg)
    ipo_amd.require_gpu()
    has_rule = hasattr(ipo_amd.Context, "set_start_rule")
    with tempfile.TemporaryDirectory() as tmp:
        for spec in a.problems:
            kind, arg = spec.split(":")
            p = pc_time.netlib(arg, ipo_amd, tmp) if kind == "netlib" else qp_dense_time.make_problem(kind, int(arg))
            ctx = ipo_amd.Context(p)
            try:
                head = {"label": a.label, "method": a.method, "problem": spec, "m": p.m, "n": p.n,
                        "t_setup_s": round(ctx.setup_seconds, 3), "repeats": a.repeats}
                print(json.dumps({**head, "start": "default", **leg(ctx, a.method, a.repeats)}), flush=True)
                if not has_rule:
                    continue
                ctx.start_point("mehrotra")                    # warm-up
                ms = []
                for _ in range(a.repeats):
                    ipo_amd.device_synchronize()
                    t0 = time.perf_counter()
                    ctx.start_point("mehrotra")
                    ms.append(1e3 * (time.perf_counter() - t0))
                ctx.set_start_rule("mehrotra")
                print(json.dumps({**head, "start": "mehrotra", **leg(ctx, a.method, a.repeats),
                                  "start_point_ms": spread(ms)}), flush=True)
            finally:
                ctx.close()


if __name__ == "__main__":
    main()
