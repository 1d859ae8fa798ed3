#!/usr/bin/env python3
"""Reciprocal ICP (kss_icp_recip_dev) beside one-to-one ICP (kss_icp_o2o_dev) at overlap 1, point metric, same build, same process,
alternating, --rounds times after one warm-up round; medians with min - max.  No threshold is fixed in advance: one-to-one's figure
behind the NN pass is what reciprocal's is set beside, and the values go into DESIGN.md 2.25.
  1  tools/o2o_time.py's partly overlapping pair (partial pair 1 of the tests at n = 137000: 100 074 x 91 614) and
     make_outlier_pair(1, 100000, 10, 0.2): us per whole pass in fixed-iteration mode (difference of a --passes and a 2 x --passes
     run, so setup and the first pass drop out) and the launches behind the NN pass alone from the library's own event pairs
     (KSS_K_CORR_REDUCE): there reciprocal minus one-to-one = two more launches and the reverse search.
  2  the filter alone (kss_recip_filter_dev) on 100 000 sources: a converged map (the source is the target plus 1e-3 jitter), a
     far-apart map (the same source moved by 3 along x: the balls span the whole grid and most winners take the escape), and every
     source at one point (one cell holds them all).
With --baseline LIB every variant also runs on a second context on that library (the parent commit's build), "parent " in front of its
name, alternating with this build's in the same process: the one-to-one rows, whose code a change to the reciprocal filter does not
touch, are the control for what the machine itself moves.
usage: python tools/recip_time.py [--baseline path/to/parent/libkssicp.so] [--rounds 5] [--passes 20] [--only 12]"""
import argparse, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g
import torch
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--passes", type=int, default=20)
ap.add_argument("--only", default="12")
ap.add_argument("--baseline", default=None)
args = ap.parse_args()
pkg = g.load_package(); S = pkg.synth
ctx = pkg.Context(0)
# name prefix -> context: every run below is a (context, function of that context) pair
CTXS = {"": ctx}
if args.baseline:
    CTXS["parent "] = pkg.Context(0, lib=pkg.binding.load_library(args.baseline))
POINT = pkg.METRIC_POINT


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, time.perf_counter() - t0


def report(per, unit):
    for k, v in per.items():
        print("%-40s %9.2f %s  (min %.2f, max %.2f over %d rounds)" % (k, float(np.median(v)), unit, min(v), max(v), len(v)), flush=True)


def alternating(runs, measure):
    per = {k: [] for k in runs}
    for r in range(args.rounds):
        order = list(runs)
        if r % 2:
            order.reverse()
        for k in order:
            per[k].append(measure(runs[k]))
    return per


def per_pass(runs, passes):
    """us per whole pass of each run, from the difference of two fixed-iteration runs"""
    P = [ctx.icp_params(max_iterations=it, fixed_iterations=1, compute_fitness=0) for it in (passes, 2 * passes)]
    for cx, run in runs.values():      # warm-up of every variant and shape (allocations, cell list sizes)
        for p in P:
            run(cx, p)

    def measure(cr):
        cx, run = cr
        ts = [timed(lambda: run(cx, p))[1] for p in P]
        return (ts[1] - ts[0]) / passes * 1e6
    per = alternating(runs, measure)
    report(per, "us per pass")
    return {k: float(np.median(v)) for k, v in per.items()}


def behind_nn(runs, passes):
    """us per pass of the launches behind the NN pass alone (kss_profile_get of KSS_K_CORR_REDUCE)"""
    p = ctx.icp_params(max_iterations=passes, fixed_iterations=1, compute_fitness=0)

    def measure(cr):
        cx, run = cr
        cx.profile_reset()
        run(cx, p)
        cx.synchronize()
        ms, n = cx.profile_get(pkg.K_CORR_REDUCE)
        return ms / max(n, 1) * 1e3
    for cx in CTXS.values():
        cx.profile_enable(1)
    per = alternating(runs, measure)
    for cx in CTXS.values():
        cx.profile_enable(0)
    report({k + ", behind the NN pass": v for k, v in per.items()}, "us per pass")
    return {k: float(np.median(v)) for k, v in per.items()}


if "1" in args.only:
    scenes = {"partial pair": S.make_partial_pair(1, 137000, 10.0, -0.35, 0.5)[:2], "outlier pair": S.make_outlier_pair(1, 100000, 10.0, 0.2)[:2]}
    for name, (src, tgt) in scenes.items():
        ns, nt = len(src), len(tgt)
        ds, dt = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (src, tgt))
        torch.cuda.synchronize()
        print("== 1: %s, %d x %d" % (name, ns, nt), flush=True)
        a = (ds.data_ptr(), ns, dt.data_ptr(), nt, None)
        runs = {}
        for pre, cx in CTXS.items():
            runs[pre + "o2o point 1.0"] = (cx, lambda cx, p: cx.icp_o2o_dev(*a, p, overlap=1.0, metric=POINT)[0])
            runs[pre + "recip point 1.0"] = (cx, lambda cx, p: cx.icp_recip_dev(*a, p, overlap=1.0, metric=POINT)[0])
        med = per_pass(runs, args.passes)
        beh = behind_nn(runs, args.passes)
        print("%s: recip - o2o = %.1f us per whole pass, %.1f us behind the NN pass" % (
            name, med["recip point 1.0"] - med["o2o point 1.0"], beh["recip point 1.0"] - beh["o2o point 1.0"]), flush=True)
        for it in (1, 2 * args.passes):
            _, info = ctx.icp_recip_dev(*a, ctx.icp_params(max_iterations=it, fixed_iterations=1, compute_fitness=0), overlap=1.0, metric=POINT)
            print("pass %d: m = %d candidates, u = %d winners, r = %d mutual" % (it, info[4], info[5], info[0]), flush=True)

if "2" in args.only:
    n = 100000
    base, tgt = S.make_pair(0, n, shape="bumpy")
    sets = {"converged": (base, 1.0), "far apart (escape)": ((base + np.array([3.0, 0.0, 0.0], np.float32)).astype(np.float32), 100.0),
            "all sources at one point": (np.tile(base[:1], (n, 1)), 1.0)}
    print("== 2: the filter alone, %d sources x %d targets (the call: the target's box, five launches, the counters' copy back)" % (n, len(tgt)),
          flush=True)
    dt = torch.from_numpy(tgt).cuda()
    oi, od = torch.empty(n, dtype=torch.int32).cuda(), torch.empty(n, dtype=torch.float32).cuda()
    dev = {}
    for k, (src, max_d2) in sets.items():
        idx, d2 = ctx.nn(src, tgt)
        dev[k] = (torch.from_numpy(np.ascontiguousarray(src)).cuda(), torch.from_numpy(idx).cuda(), torch.from_numpy(d2).cuda(), max_d2)
    torch.cuda.synchronize()

    def call(cx, k, recip):
        ds, di, dd, max_d2 = dev[k]
        if recip:
            return cx.recip_filter_dev(ds.data_ptr(), n, dt.data_ptr(), len(tgt), di.data_ptr(), dd.data_ptr(), max_d2, 0, oi.data_ptr(), od.data_ptr())
        return cx.o2o_filter_dev(di.data_ptr(), dd.data_ptr(), n, len(tgt), max_d2, oi.data_ptr(), od.data_ptr())
    runs = {}
    for k in dev:
        for pre, cx in CTXS.items():
            print("%-28s {m, u, r} = %s" % (pre + k, call(cx, k, True)), flush=True)
            call(cx, k, False)
            runs[pre + "o2o filter, " + k] = (cx, lambda cx, k=k: call(cx, k, False))
            runs[pre + "recip filter, " + k] = (cx, lambda cx, k=k: call(cx, k, True))
    report(alternating(runs, lambda cr: timed(lambda: [cr[1](cr[0]) for _ in range(20)])[1] / 20 * 1e6), "us per call")
for cx in CTXS.values():
    cx.close()
