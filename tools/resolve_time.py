#!/usr/bin/env python3
"""What re-solving on one context buys: a measurement
tool, not a test.  Section 10.1's protocol: one session, a warm-up, medians of
`--repeats` with the spread (min, max), one JSON line per measurement.

Legs:

  create   wall time of Context(p) + run(method), a fresh context each time.
           Uses nothing newer than Context / run, so it runs on another
           commit's build too (--pkg DIR, as tools/pc_time.py): parent and
           change alternate in one session.
  update   on one context: wall time of update(A, b, c, f[, q]) + run(method),
           every array uploaded; the members alternate between the problem and
           a copy with c (and Q) scaled, so that every update changes numbers.
           The update's own time is split into its uploads with their
           validation and the device refresh (Context.update_seconds).
  sweep    a ten-point sweep of one QP with Q scaled by lambda from 0.5 to 2
           (geometric), method pc: cold legs from the default start, warm legs
           from start_from_last(floor) with floor = mult x sqrt(final gamma /
           (n + m)) of the previous solve, mult in --mults.  Printed lines,
           seconds (the solver's clock around its loop) and every status.
  table    read the JSON lines of --out files and print section 10.3's tables.

Problems: netlib:NAME (method hsd), factor:N and arrow:N of
tools/qp_dense_time.py (method pc).

usage: resolve_time.py create [--pkg DIR] [--label L] [--repeats R] netlib:25fv47 factor:2048
       resolve_time.py update [--repeats R] netlib:25fv47 factor:2048 arrow:200000
       resolve_time.py sweep [--repeats R] factor:2048
       resolve_time.py table profiles/resolve_time.jsonl
"""
import argparse
import gzip
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def load(spec, ipo_amd, tmp):
    """(problem, method) of a problem spec."""
    import qp_dense_time            # make_problem only (it imports ipo_amd: the one chosen in main)
    kind, arg = spec.split(":")
    if kind == "netlib":
        dst = os.path.join(tmp, arg + ".mps")
        with gzip.open(os.path.join(REPO, "tests", "golden", "netlib", arg + ".mps.gz"), "rb") as fi, \
                open(dst, "wb") as fo:
            shutil.copyfileobj(fi, fo)
        return ipo_amd.load_mps(dst), "hsd"
    p = qp_dense_time.make_problem(kind, int(arg))
    if kind == "arrow" and p.n + p.m >= 100000:
        os.environ.setdefault("IPO_HIP_ORDER", "md")      # tools/qp_dense_time.py main: nested dissection's plan is too large
    return p, "pc"


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as fh:
            fh.write(line + "\n")


def count_lines(text):
    return sum(1 for ln in text.splitlines() if ln[:9].strip().isdigit())


def leg_create(a, ipo_amd, tmp):
    for spec in a.problems:
        p, method = load(spec, ipo_amd, tmp)
        wall, setup, solve, st = [], [], [], None
        for r in range(-1, a.repeats):                  # one warm-up
            t0 = time.perf_counter()
            ctx = ipo_amd.Context(p)
            try:
                st, s, _ = ctx.run(method)
                t = time.perf_counter() - t0
            finally:
                ctx.close()
            print(f"# {spec} {a.label}: context + run {t:.3f} s", file=sys.stderr, flush=True)
            if r >= 0:
                wall.append(t)
                setup.append(ctx.setup_seconds)
                solve.append(s["t_solve_s"])
        emit({"leg": "create", "label": a.label, "problem": spec, "method": method, "m": p.m, "n": p.n, "status": st,
              "iters": s["iters"], "repeats": a.repeats, "wall_s": spread(wall), "t_setup_s": spread(setup),
              "t_solve_s": spread(solve)}, a.out)


def leg_update(a, ipo_amd, tmp):
    import numpy as np
    for spec in a.problems:
        p, method = load(spec, ipo_amd, tmp)
        rng = np.random.default_rng(1)
        c2 = p.c * rng.uniform(0.95, 1.05, p.n)
        q = getattr(p, "q", None)
        members = [dict(A=p.A, b=p.b, c=p.c, f=p.f), dict(A=p.A, b=p.b, c=c2, f=p.f)]
        if q is not None:
            members[0]["q"], members[1]["q"] = q[2], 1.25 * q[2]
        t0 = time.perf_counter()
        ctx = ipo_amd.Context(p)
        t_create = time.perf_counter() - t0
        try:
            st0, s0, _ = ctx.run(method)                # warm-up, and the fresh context's figures
            wall, upd, up, refresh, solve, stats = [], [], [], [], [], []
            for r in range(-1, 2 * a.repeats):          # one warm-up update; then the members alternating
                kw = members[(r + 1) % 2]
                t0 = time.perf_counter()
                ctx.update(**kw)
                t1 = time.perf_counter()
                st, s, _ = ctx.run(method)
                t2 = time.perf_counter()
                if r >= 0:
                    u, f = ctx.update_seconds()
                    wall.append(t2 - t0); upd.append(t1 - t0); up.append(u); refresh.append(f)
                    solve.append(s["t_solve_s"]); stats.append((st, s["iters"]))
        finally:
            ctx.close()
        emit({"leg": "update", "label": a.label, "problem": spec, "method": method, "m": p.m, "n": p.n,
              "nz": int(p.nz), "q_entries": int(q[0][-1]) if q is not None else 0,
              "create_s": t_create, "t_setup_s": ctx.setup_seconds, "first_status": st0, "first_iters": s0["iters"],
              "status_iters": sorted(set(stats)), "repeats": 2 * a.repeats, "wall_s": spread(wall),
              "update_s": spread(upd), "upload_s": spread(up), "refresh_s": spread(refresh),
              "t_solve_s": spread(solve)}, a.out)


def leg_sweep(a, ipo_amd, tmp):
    import numpy as np
    for spec in a.problems:
        p, method = load(spec, ipo_amd, tmp)
        lams = [0.5 * 4.0 ** (k / 9.0) for k in range(10)]
        Q = p.q[2]
        ctx = ipo_amd.Context(p)
        try:
            ctx.run(method)                             # warm-up
            for mult in [None] + [float(v) for v in a.mults.split(",")]:
                runs = []                               # per repeat: per point (status, lines, seconds, floor)
                for _ in range(a.repeats):
                    pts, gamma = [], None
                    ctx.clear_start()
                    for k, lam in enumerate(lams):
                        ctx.update(q=lam * Q)
                        floor = None
                        if mult is not None and k > 0:
                            floor = mult * float(np.sqrt(gamma / (p.n + p.m)))
                            ctx.start_from_last(floor)
                        st, s, text = ctx.run(method, trace=True)
                        gamma = s["final_mu"]           # pc: the last line's gamma = z'x + y'w
                        pts.append((st, count_lines(text), s["t_solve_s"], floor))
                    runs.append(pts)
                ctx.clear_start()
                emit({"leg": "sweep", "label": a.label, "problem": spec, "method": method, "m": p.m, "n": p.n,
                      "start": "cold" if mult is None else "warm", "floor_mult": mult, "repeats": a.repeats,
                      "lambda": [round(v, 4) for v in lams],
                      "status": [runs[0][k][0] for k in range(10)], "lines": [runs[0][k][1] for k in range(10)],
                      "lines_same_every_repeat": all([q[1] for q in r] == [q[1] for q in runs[0]] for r in runs),
                      "floor": [runs[0][k][3] for k in range(10)],
                      "seconds": [spread([r[k][2] for r in runs]) for k in range(10)],
                      "total_lines": sum(q[1] for q in runs[0]),
                      "total_seconds": spread([sum(q[2] for q in r) for r in runs])}, a.out)
        finally:
            ctx.close()


def fmt(sp, scale=1.0, digits=3):
    return f"{scale * sp['median']:.{digits}f} [{scale * sp['min']:.{digits}f}–{scale * sp['max']:.{digits}f}]"


def leg_table(a):
    recs = []
    for path in a.problems:
        with open(path) as fh:
            recs += [json.loads(ln) for ln in fh if ln.strip()]
    print("| problem | leg | build | status, lines | wall s | of it: setup / update s | upload ms | refresh ms | solve s |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in recs:
        if r.get("leg") == "create":
            print(f"| {r['problem']} | create + run | {r['label']} | {r['status']}, {r['iters']} | {fmt(r['wall_s'])} | "
                  f"{fmt(r['t_setup_s'])} | | | {fmt(r['t_solve_s'], digits=4)} |")
        elif r.get("leg") == "update":
            si = "; ".join(f"{s}, {i}" for s, i in r["status_iters"])
            print(f"| {r['problem']} | update + run | {r['label']} | {si} | {fmt(r['wall_s'], digits=4)} | "
                  f"{fmt(r['update_s'], digits=5)} | {fmt(r['upload_s'], 1e3)} | {fmt(r['refresh_s'], 1e3)} | "
                  f"{fmt(r['t_solve_s'], digits=4)} |")
    print()
    print("| start | floor, units of sqrt(gamma / (n + m)) | status per point | lines per point | lines | seconds |")
    print("|---|---|---|---|---|---|")
    for r in recs:
        if r.get("leg") == "sweep":
            print(f"| {r['start']} | {'' if r['floor_mult'] is None else r['floor_mult']} | "
                  f"{' '.join(str(s) for s in r['status'])} | {' '.join(str(s) for s in r['lines'])} | "
                  f"{r['total_lines']} | {fmt(r['total_seconds'])} |")
    for r in recs:
        if r.get("leg") == "bench":
            print(f"\nbench {r['label']}: {r['it_per_s']}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("leg", choices=["create", "update", "sweep", "table"])
    ap.add_argument("--pkg", default=os.path.join(REPO, "linear-programming-vanderbei_amd"))
    ap.add_argument("--label", default="change")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--mults", default="1e-2,1,10")
    ap.add_argument("--out", default="", help="append the JSON lines to this file too")
    ap.add_argument("problems", nargs="+", help="netlib:NAME, factor:N or arrow:N (table: JSON-lines files)")
    a = ap.parse_args()
    if a.leg == "table":
        return leg_table(a)
    sys.path[:0] = [os.path.abspath(a.pkg), os.path.join(REPO, "tools")]
    import ipo_amd
    assert os.path.dirname(os.path.dirname(os.path.abspath(ipo_amd.__file__))) == os.path.abspath(a.pkg)
    ipo_amd.require_gpu()
    with tempfile.TemporaryDirectory() as tmp:
        {"create": leg_create, "update": leg_update, "sweep": leg_sweep}[a.leg](a, ipo_amd, tmp)


if __name__ == "__main__":
    main()
