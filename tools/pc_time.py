#!/usr/bin/env python3
"""Time one method on one build: method "pc" against
"intpt" on netlib LPs and against "qp" on tools/qp_dense_time.py's factor QP.

The protocol of section 10.1: one persistent context per problem, one warm-up
solve, then `--repeats` solves timed by the solver's own clock around the
iteration loop (t_solve_s) and `--repeats` more in timing mode for the device
time of the factorisations and the refined solves (HIP events).  One JSON
line per problem with the medians and the spread (min, max).

--pkg DIR: the package directory (the one that holds ipo_amd/ and lib/) of
the build to time -- this checkout's by default, another commit's build to
time the two alternately in one session.  The tool uses nothing but the
package's public Python API.

usage: pc_time.py [--pkg DIR] [--label L] [--repeats R] --method pc netlib:25fv47 netlib:dfl001 factor:2048
"""
import argparse
import gzip
import json
import os
import shutil
import statistics
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def netlib(name, ipo_amd, tmp):
    dst = os.path.join(tmp, name + ".mps")
    with gzip.open(os.path.join(REPO, "tests", "golden", "netlib", name + ".mps.gz"), "rb") as fi, open(dst, "wb") as fo:
        shutil.copyfileobj(fi, fo)
    return ipo_amd.load_mps(dst)


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
    import qp_dense_time            # make_problem only (it imports ipo_amd: the one chosen above)
    assert os.path.dirname(os.path.dirname(os.path.abspath(ipo_amd.__file__))) == os.path.abspath(a.pkg)
    ipo_amd.require_gpu()
    with tempfile.TemporaryDirectory() as tmp:
        for spec in a.problems:
            kind, arg = spec.split(":")
            p = netlib(arg, ipo_amd, tmp) if kind == "netlib" else qp_dense_time.make_problem(kind, int(arg))
            ctx = ipo_amd.Context(p)
            try:
                st, s, text = ctx.run(a.method, trace=True)                  # warm-up
                lines = sum(1 for ln in text.splitlines() if ln[:9].strip().isdigit())
                plain = [ctx.run(a.method)[1] for _ in range(a.repeats)]
                timed = [ctx.run(a.method, timing=True)[1] for _ in range(a.repeats)]
                systems = max(s["factors"], 1)                               # Newton systems formed
                out = {"label": a.label, "method": a.method, "problem": spec, "m": p.m, "n": p.n, "status": st,
                       "lines": lines, "factors": s["factors"], "solves": s["solves"],
                       "refine_passes": s["refine_passes"], "t_setup_s": round(ctx.setup_seconds, 3),
                       "repeats": a.repeats,
                       "t_solve_s": spread([r["t_solve_s"] for r in plain]),
                       "ms_per_iter": spread([1e3 * r["t_solve_s"] / systems for r in plain]),
                       "solve_ms_per_iter": spread([r["solve_ms"] / systems for r in timed]),
                       "factor_ms_per_iter": spread([r["factor_ms"] / systems for r in timed])}
            finally:
                ctx.close()
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
