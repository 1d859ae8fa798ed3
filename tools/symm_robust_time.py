#!/usr/bin/env python3
"""Robust symmetric ICP, us per pass on one pair: kss_icp_symm_robust_dev with Tukey weights, fixed and automatic scale, beside its
siblings from the same build in the same process -- kss_icp_symm_dev and kss_icp_robust_dev (plane metric, Tukey, fixed and
automatic).  The pair is two disjoint halves of one surface (as tests/gicp_ref.halves_pair makes them), both clouds' normals
precomputed (kss_normals at k = 20) and passed as device pointers.  The per-pass time is the difference of a 2 x passes and a passes
fixed_iterations run divided by passes (setup drops out: DESIGN.md 2.12's method), no fitness pass, default nn_mode.  The variants
alternate --rounds times after one warm-up round; the median and min - max of each are reported, and the two expectations of
DESIGN.md 2.19: fixed robust symmetric - symmetric, and what the automatic scale adds on either metric.
usage: python tools/symm_robust_time.py [--n 100000] [--passes 50] [--rounds 5] [--deg 10]"""
import argparse, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g
import torch
ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=100000)
ap.add_argument("--passes", type=int, default=50)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--deg", type=float, default=10.0)
ap.add_argument("--scale", type=float, default=0.05, help="the fixed scale")
args = ap.parse_args()
pkg = g.load_package(); S = pkg.synth
ctx = pkg.Context(0)


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, time.perf_counter() - t0


n = args.n
M = S.bumpy(8, 2 * n)[S.permutation(3008, 2 * n)]
R = S.rot_axis_angle([0.3, -0.5, 1.0], np.deg2rad(args.deg))
src = (M[n:] @ R.T + np.array([0.02, -0.01, 0.03])).astype(np.float32)
tgt = M[:n].astype(np.float32)
sn = ctx.normals(src.astype(np.float64), 20).astype(np.float32)
tn = ctx.normals(tgt.astype(np.float64), 20).astype(np.float32)
ds, dt, dsn, dtn = (torch.from_numpy(x).cuda() for x in (src, tgt, sn, tn))
torch.cuda.synchronize()
print("== one pair of %d x %d, disjoint halves, %.0f degrees; %d and %d fixed passes" % (n, n, args.deg, args.passes, 2 * args.passes), flush=True)
TUKEY, PLANE = pkg.LOSS_TUKEY, pkg.METRIC_PLANE
rp_fixed = pkg.robust_params(TUKEY, PLANE, scale=args.scale)
rp_auto = pkg.robust_params(TUKEY, PLANE)
a = (ds.data_ptr(), n, dsn.data_ptr(), dt.data_ptr(), n, dtn.data_ptr())
runs = {
    "symm": lambda p: ctx.icp_symm_dev(a[0], a[1], a[2], a[3], a[4], a[5], p),
    "symm robust, fixed": lambda p: ctx.icp_symm_robust_dev(a[0], a[1], a[2], a[3], a[4], a[5], p, rp=rp_fixed)[0],
    "symm robust, automatic": lambda p: ctx.icp_symm_robust_dev(a[0], a[1], a[2], a[3], a[4], a[5], p, rp=rp_auto)[0],
    "plane robust, fixed": lambda p: ctx.icp_robust_dev(a[0], a[1], a[3], a[4], a[5], p, rp=rp_fixed)[0],
    "plane robust, automatic": lambda p: ctx.icp_robust_dev(a[0], a[1], a[3], a[4], a[5], p, rp=rp_auto)[0],
}
P1 = ctx.icp_params(max_iterations=args.passes, fixed_iterations=1, compute_fitness=0)
P2 = ctx.icp_params(max_iterations=2 * args.passes, fixed_iterations=1, compute_fitness=0)
for k, run in runs.items():      # warm-up of every variant (allocations, cell list sizes) -- and that both lengths run to the end
    r1, r2 = run(P1), run(P2)
    print("%-24s %d and %d passes, state %d" % (k, r1.iterations, r2.iterations, r2.state), flush=True)
pp = {k: [] for k in runs}
for r in range(args.rounds):
    order = list(runs)
    if r % 2:
        order.reverse()
    for k in order:
        t1 = timed(lambda: runs[k](P1))[1]
        t2 = timed(lambda: runs[k](P2))[1]
        pp[k].append((t2 - t1) / args.passes * 1e6)
med = {k: float(np.median(v)) for k, v in pp.items()}
for k, v in pp.items():
    print("%-24s %9.1f us per pass  (min %.1f, max %.1f over %d rounds)" % (k, med[k], min(v), max(v), len(v)), flush=True)
print("fixed robust symmetric - symmetric: %+.1f us per pass (expected: 0 within the spread)" % (med["symm robust, fixed"] - med["symm"]))
print("automatic - fixed: symmetric %+.1f us, plane %+.1f us per pass (expected: equal within the spread)" % (
    med["symm robust, automatic"] - med["symm robust, fixed"], med["plane robust, automatic"] - med["plane robust, fixed"]), flush=True)
ctx.close()
