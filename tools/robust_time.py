#!/usr/bin/env python3
"""Robust ICP (kss_icp_robust_dev) per pass: every loss with both metrics, with the automatic scale (median key per pass) and
with a fixed one, next to kss_icp_trimmed_dev at overlap 0.5 and kss_icp_p2l_dev from the same build: us per pass in
fixed-iteration mode (difference of a 50- and a 100-pass run, so setup and the first pass drop out), on the bumpy 100k x 100k
pair of tools/p2l_time.py; all variants run alternately, --rounds times, and the median is reported with the spread.  The
comparisons that matter: automatic point pass against the trimmed point pass (the same launches), automatic plane pass minus the
trimmed plane pass = the key launch, fixed-scale plane pass against kss_icp_p2l.  Then PCL mode on the outlier pair of the tests
scaled to n = 100000 (iterations, error against the true motion).  Under rocprofv3 --kernel-trace --stats the per-kernel times
come from the trace.
usage: python tools/robust_time.py [--rounds 5] [--passes 50] [--quick]"""
import argparse, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g
import torch
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--passes", type=int, default=50)
ap.add_argument("--quick", action="store_true", help="one round, no PCL mode (for a profiler run)")
args = ap.parse_args()
pkg = g.load_package(); S = pkg.synth
ctx = pkg.Context(0)
if args.quick:
    args.rounds = 1
LOSSES = [("l2", pkg.LOSS_L2), ("huber", pkg.LOSS_HUBER), ("tukey", pkg.LOSS_TUKEY), ("cauchy", pkg.LOSS_CAUCHY)]
METRICS = [("point", pkg.METRIC_POINT), ("plane", pkg.METRIC_PLANE)]


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, time.perf_counter() - t0


def device(src, tgt):
    nrm = ctx.normals(tgt.astype(np.float64), 20).astype(np.float32)
    ds, dt, dn = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (src, tgt, nrm))
    return (ds.data_ptr(), len(src), dt.data_ptr(), len(tgt)), dn, (ds, dt)


def robust(a, dn, loss, metric, **kw):
    rp = pkg.robust_params(loss, metric, **kw)
    return lambda p: ctx.icp_robust_dev(*a, dn.data_ptr() if metric == pkg.METRIC_PLANE else None, p, rp=rp)[0]


Rb = S.rot_axis_angle([0.3, -0.5, 1.0], np.deg2rad(10.0))
tb = np.array([0.02, -0.01, 0.03])
src, tgt = S.make_pair(0, 100000, R=Rb, t=tb, shape="bumpy")
a, dn, keep = device(src, tgt)
print("== bumpy, %d x %d" % (len(src), len(tgt)), flush=True)
runs = {"p2l": lambda p: ctx.icp_p2l_dev(*a, dn.data_ptr(), p),
        "trim point 0.5": lambda p: ctx.icp_trimmed_dev(*a, None, p, overlap=0.5, metric=pkg.METRIC_POINT)[0],
        "trim plane 0.5": lambda p: ctx.icp_trimmed_dev(*a, dn.data_ptr(), p, overlap=0.5, metric=pkg.METRIC_PLANE)[0]}
for ln, loss in LOSSES:
    for mn, metric in METRICS:
        runs["%s %s auto" % (ln, mn)] = robust(a, dn, loss, metric)
        runs["%s %s fixed" % (ln, mn)] = robust(a, dn, loss, metric, scale=0.02)
P = [ctx.icp_params(max_iterations=it, fixed_iterations=1, compute_fitness=0) for it in (args.passes, 2 * args.passes)]
for run in runs.values():      # warm-up of every variant (allocations, cell list sizes)
    for p in P:
        run(p)
per = {k: [] for k in runs}
for r in range(args.rounds):
    for k in (list(runs) if r % 2 == 0 else list(runs)[::-1]):
        ts = [timed(lambda: runs[k](p))[1] for p in P]
        per[k].append((ts[1] - ts[0]) / args.passes * 1e6)
med = {k: float(np.median(v)) for k, v in per.items()}
for k, v in per.items():
    print("%-22s %7.1f us per pass  (min %.1f, max %.1f over %d rounds)" % (k, med[k], min(v), max(v), len(v)), flush=True)
print("huber point auto - trim point 0.5: %.1f us;  huber plane auto - trim plane 0.5 (the key launch): %.1f us;  "
      "huber plane fixed - p2l: %.1f us" % (med["huber point auto"] - med["trim point 0.5"], med["huber plane auto"] - med["trim plane 0.5"],
                                            med["huber plane fixed"] - med["p2l"]), flush=True)
if not args.quick:
    src, tgt, R, t = S.make_outlier_pair(2, 100000, 10.0, 0.3)
    a, dn, keep = device(src, tgt)
    R_true, t_true = R.T, -R.T @ t
    print("== outlier pair 2 (30 %% of the sources off the surface), %d x %d" % (len(src), len(tgt)), flush=True)
    pcl = {"p2p": lambda p: ctx.icp_dev(*a, p), "p2l": lambda p: ctx.icp_p2l_dev(*a, dn.data_ptr(), p)}
    for ln, loss in LOSSES[1:]:
        for mn, metric in METRICS:
            pcl["%s %s auto" % (ln, mn)] = robust(a, dn, loss, metric)
    for k, run in pcl.items():
        r, dt_s = timed(lambda: run(ctx.icp_params(max_iterations=200)))
        T = r.matrix()
        print("%-22s PCL mode: %3d iterations, state %d, fitness %.3e, |R - R_true| %.2e, |t - t_true| %.2e, %.2f ms"
              % (k, r.iterations, r.state, r.fitness, np.abs(T[:3, :3] - R_true).max(), np.abs(T[:3, 3] - t_true).max(), dt_s * 1e3), flush=True)
ctx.close()
