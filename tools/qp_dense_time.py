#!/usr/bin/env python3
"""Time method "qp" on QPs whose Q has long columns.

Problems, in the style of tests/qp_dense.py's generators (feasible and
bounded by construction from an interior point), built vectorised here so
that the tool needs nothing but the package's public Python API and runs on
any commit that has method "qp":

  factor N   m = 512, n = N, Q = F F' / 4 + diag (F n x 4): n^2 stored entries
  arrow N    m = 512, n = N, three dense rows and columns in a diagonal Q
             (from 100,000 nodes by the minimum-degree order, IPO_HIP_ORDER=md
             unless the environment says otherwise: see main)

Per problem: one warm-up solve on a persistent context, then `--repeats`
solves timed by the solver's own clock around the iteration loop
(t_solve_s: host time from the first launch to the last synchronise), and
`--repeats` more in timing mode for the device time of the refined solves
(solve_ms, HIP events).  Prints one JSON line per problem with the medians
and the spread (min, max).  IPO_HIP_Q_LONG is honoured by commits that have it.

usage: qp_dense_time.py [--repeats R] [--max-iter K] factor:2048 factor:4096 arrow:200000
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import scipy.sparse as sp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "linear-programming-vanderbei_amd")]
import ipo_amd  # noqa: E402


def make_a(m, n, rng):
    """Row 0 all positive (x >= 0 is bounded), every other row with an entry
    at column i % n, two more random entries per column (duplicates summed)."""
    sign = lambda k: rng.choice([-1.0, 1.0], k)      # noqa: E731
    r = [np.zeros(n, np.int64), np.arange(1, m), rng.integers(1, m, 2 * n)]
    c = [np.arange(n), np.arange(1, m) % n, np.repeat(np.arange(n), 2)]
    v = [rng.uniform(0.5, 1.5, n), rng.uniform(0.5, 1.5, m - 1) * sign(m - 1), rng.uniform(0.5, 1.5, 2 * n) * sign(2 * n)]
    A = sp.coo_matrix((np.concatenate(v), (np.concatenate(r), np.concatenate(c))), shape=(m, n)).tocsc()
    A.sum_duplicates()
    A.sort_indices()
    return A


def make_q(n, kind, rng):
    if kind == "factor":
        F = rng.uniform(-1.0, 1.0, (n, 4))
        M = np.triu(F @ F.T / 4 + np.diag(rng.uniform(0.1, 2.0, n)))
        M = M + np.triu(M, 1).T                       # mirrored: symmetric bit for bit
        return sp.csc_matrix(M)
    R = rng.uniform(-0.1, 0.1, (3, n))
    R[:, :3] = 0.0
    top = sp.vstack([sp.csr_matrix(R), sp.csr_matrix((n - 3, n))])
    off = (top + top.T).tocsc()
    d = np.asarray(abs(off).sum(0)).ravel() + rng.uniform(0.5, 1.5, n)      # diagonally dominant: PSD
    Q = (off + sp.diags(d)).tocsc()
    Q.sort_indices()
    return Q


def make_problem(kind, n, m=512, seed=0):
    rng = np.random.default_rng([seed, m, n, 0 if kind == "factor" else 1])
    A, Q = make_a(m, n, rng), make_q(n, kind, rng)
    xs, zs = rng.uniform(0.5, 1.5, n), rng.uniform(0.5, 1.5, n)
    ys, ws = rng.uniform(0.5, 1.5, m), rng.uniform(0.5, 1.5, m)
    b = A @ xs + ws
    c = A.T @ ys - zs + Q @ xs
    q = (Q.indptr.astype(np.int32), Q.indices.astype(np.int32), Q.data.astype(np.float64))
    return ipo_amd.SolverForm(m, n, A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64),
                              b, c, 0.0, q=q)


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--max-iter", type=int, default=200)
    ap.add_argument("--label", default="")
    ap.add_argument("problems", nargs="+", help="factor:N or arrow:N")
    a = ap.parse_args()
    ipo_amd.require_gpu()
    for spec in a.problems:
        kind, n = spec.split(":")
        t0 = time.perf_counter()
        p = make_problem(kind, int(n))
        t_gen = time.perf_counter() - t0
        lens = np.diff(p.q[0])
        if kind == "arrow" and p.n + p.m >= 100000:
            # nested dissection (the default from 100,000 nodes) cuts through the
            # three hub columns: its plan for n = 200,000 exceeds 2^31 entries of
            # L, minimum degree's has 1.3e6 (and takes the host about a minute)
            os.environ.setdefault("IPO_HIP_ORDER", "md")
        ctx = ipo_amd.Context(p)
        try:
            st, s, _ = ctx.run("qp", max_iter=a.max_iter)                   # warm-up
            plain = [ctx.run("qp", max_iter=a.max_iter)[1] for _ in range(a.repeats)]
            timed = [ctx.run("qp", max_iter=a.max_iter, timing=True)[1] for _ in range(a.repeats)]
            out = {"label": a.label, "problem": spec, "m": p.m, "n": p.n, "q_entries": int(p.q[0][-1]),
                   "q_longest_column": int(lens.max()), "q_columns_256": int((lens >= 256).sum()),
                   "q_long": ctx.q_long() if hasattr(ctx, "q_long") else None,
                   "env_q_long": os.environ.get("IPO_HIP_Q_LONG"), "order": os.environ.get("IPO_HIP_ORDER"),
                   "status": st, "iters": s["iters"],
                   "refine_passes": s["refine_passes"], "t_generate_s": round(t_gen, 2),
                   "t_setup_s": round(ctx.setup_seconds, 3), "repeats": a.repeats,
                   "t_solve_s": spread([r["t_solve_s"] for r in plain]),
                   "ms_per_iter": spread([1e3 * r["t_solve_s"] / r["iters"] for r in plain]),
                   "solve_ms_per_iter": spread([r["solve_ms"] / r["iters"] for r in timed]),
                   "factor_ms_per_iter": spread([r["factor_ms"] / r["iters"] for r in timed])}
        finally:
            ctx.close()
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
