#!/usr/bin/env python3
"""Similarity ICP (kss_icp_sim_dev) against trimmed ICP on the point metric (kss_icp_trimmed_dev) on one pair of wrong scale: us per
pass in fixed-iteration mode (difference of a `passes`- and a 2 x `passes`-pass run, so setup and the first pass drop out, median
of --rounds), then passes to convergence, the scale found and max |[sR | t] - truth| in PCL mode.  Scenes: make_pair(1, n, 8 degrees
about (1, 2, 3), scale 0.9, bumpy) at overlap 1, and make_partial_pair(1, n, 10.0, -0.35, 0.5) with the source scaled about its
centroid by 0.95 at 0.8 x the true overlap.  --root DIR loads the package of another checkout (a build of the parent commit has no
kss_icp_sim: --mode trimmed); one process is one sample, so a comparison alternates processes.  Run every process under a time
limit of its own.
usage: timeout -k 10 120 python tools/sim_time.py [--n 10000] [--passes 50] [--rounds 5] [--mode both|sim|trimmed] [--root DIR]"""
import argparse, os, sys, time
import numpy as np
ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=10000)
ap.add_argument("--passes", type=int, default=50)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--mode", default="both", choices=["both", "sim", "trimmed"])
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
import __graft_entry__ as g
import torch
pkg = g.load_package(); S = pkg.synth
ctx = pkg.Context(0)
F32, F64 = np.float32, np.float64


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, time.perf_counter() - t0


def scenes(n):
    R = S.rot_axis_angle([1.0, 2.0, 3.0], np.deg2rad(8.0))
    t = np.array([0.02, -0.01, 0.03])
    src, tgt = S.make_pair(1, n, R=R, scale=0.9, t=t, shape="bumpy")
    A = R.T / 0.9
    yield "full, scale 0.9", src, tgt, np.concatenate([A, (-A @ t)[:, None]], 1), 1.0
    src, tgt, R, t, ov = S.make_partial_pair(1, n, 10.0, -0.35, 0.5)
    c = src.astype(F64).mean(0)
    A = R.T / 0.95
    yield ("partial, source x 0.95", (c + 0.95 * (src.astype(F64) - c)).astype(F32), tgt,
           np.concatenate([A, (R.T @ (c - c / 0.95 - t))[:, None]], 1), 0.8 * ov)


for name, src, tgt, truth, ov in scenes(args.n):
    ds, dt = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (src, tgt))
    torch.cuda.synchronize()
    print("== %s: %d x %d, overlap %.3f" % (name, len(src), len(tgt), ov), flush=True)
    runs = {}
    if args.mode in ("both", "trimmed"):
        runs["trimmed point"] = lambda p: ctx.icp_trimmed_dev(ds.data_ptr(), len(src), dt.data_ptr(), len(tgt), None, p, overlap=ov,
                                                              metric=pkg.METRIC_POINT)
    if args.mode in ("both", "sim"):
        sp = pkg.sim_params(overlap=ov)
        runs["similarity"] = lambda p: ctx.icp_sim_dev(ds.data_ptr(), len(src), dt.data_ptr(), len(tgt), p, sp)
    pa = ctx.icp_params(max_iterations=args.passes, fixed_iterations=1, compute_fitness=0)
    pb = ctx.icp_params(max_iterations=2 * args.passes, fixed_iterations=1, compute_fitness=0)
    per = {k: [] for k in runs}
    for k, run in runs.items():      # warm-up (allocations, cell list sizes)
        run(pa); run(pb)
    for r in range(args.rounds):
        order = list(runs)
        if r % 2:
            order.reverse()
        for k in order:
            ta = timed(lambda: runs[k](pa))[1]
            tb = timed(lambda: runs[k](pb))[1]
            per[k].append((tb - ta) / args.passes * 1e6)
    for k, v in per.items():
        print("%-14s %8.1f us per pass  (median of %d; min %.1f, max %.1f)" % (k, float(np.median(v)), len(v), min(v), max(v)), flush=True)
    for k, run in runs.items():
        (r, info), dt_s = timed(lambda: run(ctx.icp_params()))
        T = r.matrix()
        print("%-14s PCL mode: %d passes, state %d, converged %d, scale %s, fitness %.3e, max|[sR | t] - truth| %.2e, %.2f ms" % (
            k, r.iterations, r.state, r.converged, "%.6f" % info[5] if len(info) > 4 else "-", r.fitness,
            np.abs(T[:3].astype(F64) - truth).max(), dt_s * 1e3), flush=True)
ctx.close()
