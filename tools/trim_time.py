#!/usr/bin/env python3
"""Trimmed ICP (kss_icp_trimmed_dev) per pass, both metrics at overlap 1.0 and 0.5, next to kss_icp_p2l_dev / kss_icp_dev:
us per pass in fixed-iteration mode (difference of a 50- and a 100-pass run, so setup and the first pass drop out), on the
bumpy 100k x 100k pair of tools/p2l_time.py and on partial pair 1 of the tests scaled to n = 200000.  With --baseline LIB
every variant is also timed from that build of libkssicp.so (the parent commit's), loaded beside the current one
(binding.load_library(path)); all variants run alternately, --rounds times, and the median is reported with the spread.  The comparison
that matters: trimmed plane pass minus kss_icp_p2l pass = the cost of the selection.  Then PCL mode (iterations, error
against the true motion).  Under rocprofv3 --kernel-trace --stats the per-kernel times come from the trace.
usage: python tools/trim_time.py [--baseline path/to/parent/libkssicp.so] [--rounds 5] [--passes 50] [--quick]"""
import argparse, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g
import torch
ap = argparse.ArgumentParser()
ap.add_argument("--baseline", default=None)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--passes", type=int, default=50)
ap.add_argument("--quick", action="store_true", help="one round, no PCL mode (for a profiler run)")
args = ap.parse_args()
pkg = g.load_package(); S = pkg.synth; B = pkg.binding
ctx = pkg.Context(0)
if args.quick:
    args.rounds = 1

# the parent commit's build, loaded beside the current one: every variant is timed from both
base = pkg.Context(0, lib=B.load_library(args.baseline)) if args.baseline else None


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, time.perf_counter() - t0


Rb = S.rot_axis_angle([0.3, -0.5, 1.0], np.deg2rad(10.0))
tb = np.array([0.02, -0.01, 0.03])
ps, pt, pR, ptt, pov = S.make_partial_pair(1, 200000, 10.0, -0.35, 0.5)
for name, src, tgt, R, t in (("bumpy", *S.make_pair(0, 100000, R=Rb, t=tb, shape="bumpy"), Rb, tb),
                             ("partial pair 1 (true overlap %.3f)" % pov, ps, pt, pR, ptt)):
    ns, nt = len(src), len(tgt)
    nrm = ctx.normals(tgt.astype(np.float64), 20).astype(np.float32)
    ds, dt, dn = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (src, tgt, nrm))
    print("== %s, %d x %d" % (name, ns, nt), flush=True)
    a = (ds.data_ptr(), ns, dt.data_ptr(), nt)
    variants = {"p2p": lambda cx, p: cx.icp_dev(*a, p),
                "p2l": lambda cx, p: cx.icp_p2l_dev(*a, dn.data_ptr(), p)}
    for ov in (1.0, 0.5):
        variants["trim point %.1f" % ov] = lambda cx, p, ov=ov: cx.icp_trimmed_dev(*a, None, p, overlap=ov, metric=pkg.METRIC_POINT)[0]
        variants["trim plane %.1f" % ov] = lambda cx, p, ov=ov: cx.icp_trimmed_dev(*a, dn.data_ptr(), p, overlap=ov, metric=pkg.METRIC_PLANE)[0]
    runs = {}      # each variant from this build, then from the parent's
    for k, v in variants.items():
        runs[k] = lambda p, v=v: v(ctx, p)
        if base:
            runs[k + " parent"] = lambda p, v=v: v(base, p)
    P = [ctx.icp_params(max_iterations=it, fixed_iterations=1, compute_fitness=0) for it in (args.passes, 2 * args.passes)]
    for run in runs.values():      # warm-up of every variant and shape (allocations, cell list sizes)
        for p in P:
            run(p)
    per = {k: [] for k in runs}
    for r in range(args.rounds):
        order = list(runs)
        if base and r % 2:      # the parent's first in every other round: whichever build runs second finds the caches warm
            order = [k for i in range(0, len(order), 2) for k in (order[i + 1], order[i])]
        for k in order:
            ts = [timed(lambda: runs[k](p))[1] for p in P]
            per[k].append((ts[1] - ts[0]) / args.passes * 1e6)
    med = {k: float(np.median(v)) for k, v in per.items()}
    for k, v in per.items():
        print("%-22s %7.1f us per pass  (min %.1f, max %.1f over %d rounds)" % (k, med[k], min(v), max(v), len(v)), flush=True)
    print("selection = trim plane 1.0 - p2l: %.1f us;  trim plane 0.5 - p2l: %.1f us;  trim point 1.0 - p2p: %.1f us" % (
        med["trim plane 1.0"] - med["p2l"], med["trim plane 0.5"] - med["p2l"], med["trim point 1.0"] - med["p2p"]), flush=True)
    if args.quick:
        continue
    R_true, t_true = R.T, -R.T @ t
    for k, run in runs.items():
        r, dt_s = timed(lambda: run(ctx.icp_params(max_iterations=200)))
        T = r.matrix()
        print("%-22s PCL mode: %3d iterations, state %d, fitness %.3e, |R - R_true| %.2e, |t - t_true| %.2e, %.2f ms"
              % (k, r.iterations, r.state, r.fitness, np.abs(T[:3, :3] - R_true).max(), np.abs(T[:3, 3] - t_true).max(), dt_s * 1e3), flush=True)
if base:
    base.close()
ctx.close()
