#!/usr/bin/env python3
"""One-to-one ICP (kss_icp_o2o_dev, kss_icp_o2o_batch_dev) against trimmed ICP at the same overlap, same build, same session,
alternating, --rounds times after one warm-up round; medians with min - max.
  1  a partly overlapping pair of about 100k sources (partial pair 1 of the tests at n = 137000): us per pass in fixed-iteration
     mode (difference of a --passes and a 2 x --passes run, so setup and the first pass drop out), and the launches behind the NN
     pass alone from the library's own event pairs (KSS_K_CORR_REDUCE): there o2o minus trimmed = the table reset, the claim and
     the resolve launches; the whole passes also differ by what the two trajectories cost the NN pass.  Point metric; --plane adds
     the plane metric.
  2  --pairs pairs of --n points (the tests' three partial pairs, cycled): the same per pass for the batched calls, and the batched
     o2o call against a loop of single-pair calls over the same device-resident pairs.
  3  the filter alone (kss_o2o_filter_dev) on 100 000 sources: every source on ONE target (the worst contention of the claim's
     atomic), uniform over 25 000 targets, and an injective map.
usage: python tools/o2o_time.py [--rounds 5] [--passes 20] [--pairs 1024] [--n 10000] [--plane] [--only 123]"""
import argparse, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g
import torch
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--passes", type=int, default=20)
ap.add_argument("--pairs", type=int, default=1024)
ap.add_argument("--n", type=int, default=10000)
ap.add_argument("--plane", action="store_true")
ap.add_argument("--only", default="123")
args = ap.parse_args()
pkg = g.load_package(); S = pkg.synth
ctx = pkg.Context(0)
POINT, PLANE = pkg.METRIC_POINT, pkg.METRIC_PLANE
METRICS = [("point", POINT)] + ([("plane", PLANE)] if args.plane else [])


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, time.perf_counter() - t0


def report(per, unit):
    for k, v in per.items():
        print("%-34s %9.2f %s  (min %.2f, max %.2f over %d rounds)" % (k, float(np.median(v)), unit, min(v), max(v), len(v)), flush=True)


def per_pass(runs, passes):
    """runs: {name: fn(params)}; us per pass of each, alternating order, from the difference of two fixed-iteration runs"""
    P = [ctx.icp_params(max_iterations=it, fixed_iterations=1, compute_fitness=0) for it in (passes, 2 * passes)]
    for run in runs.values():      # warm-up of every variant and shape (allocations, cell list sizes)
        for p in P:
            run(p)
    per = {k: [] for k in runs}
    for r in range(args.rounds):
        order = list(runs)
        if r % 2:
            order.reverse()
        for k in order:
            ts = [timed(lambda: runs[k](p))[1] for p in P]
            per[k].append((ts[1] - ts[0]) / passes * 1e6)
    report(per, "us per pass")
    return {k: float(np.median(v)) for k, v in per.items()}


def behind_nn(runs, passes):
    """us per pass of the launches behind the NN pass alone (the library's event pairs around them, kss_profile_get of
    KSS_K_CORR_REDUCE): the whole passes above also differ by what the two trajectories cost the NN pass"""
    p = ctx.icp_params(max_iterations=passes, fixed_iterations=1, compute_fitness=0)
    per = {k: [] for k in runs}
    ctx.profile_enable(1)
    for r in range(args.rounds):
        order = list(runs)
        if r % 2:
            order.reverse()
        for k in order:
            ctx.profile_reset()
            runs[k](p)
            ctx.synchronize()
            ms, n = ctx.profile_get(pkg.K_CORR_REDUCE)
            per[k].append(ms / max(n, 1) * 1e3)
    ctx.profile_enable(0)
    report({k + ", behind the NN pass": v for k, v in per.items()}, "us per pass")
    return {k: float(np.median(v)) for k, v in per.items()}


if "1" in args.only:
    src, tgt, _, _, ov = S.make_partial_pair(1, 137000, 10.0, -0.35, 0.5)
    ns, nt = len(src), len(tgt)
    nrm = ctx.normals(tgt.astype(np.float64), 20).astype(np.float32) if args.plane else np.zeros((1, 3), np.float32)
    ds, dt, dn = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (src, tgt, nrm))
    torch.cuda.synchronize()
    print("== 1: partial pair, %d x %d (true overlap %.3f)" % (ns, nt, ov), flush=True)
    a = (ds.data_ptr(), ns, dt.data_ptr(), nt)
    runs = {}
    for nm, metric in METRICS:
        d_n = dn.data_ptr() if metric == PLANE else None
        runs["trimmed %s 1.0" % nm] = lambda p, d_n=d_n, metric=metric: ctx.icp_trimmed_dev(*a, d_n, p, overlap=1.0, metric=metric)[0]
        runs["o2o %s 1.0" % nm] = lambda p, d_n=d_n, metric=metric: ctx.icp_o2o_dev(*a, d_n, p, overlap=1.0, metric=metric)[0]
    med = per_pass(runs, args.passes)
    beh = behind_nn(runs, args.passes)
    for nm, _ in METRICS:
        print("%s: o2o - trimmed = %.1f us per whole pass, %.1f us behind the NN pass (the reset, claim and resolve launches)" % (
            nm, med["o2o %s 1.0" % nm] - med["trimmed %s 1.0" % nm], beh["o2o %s 1.0" % nm] - beh["trimmed %s 1.0" % nm]), flush=True)
    r, info = ctx.icp_o2o_dev(*a, None, ctx.icp_params(max_iterations=1, compute_fitness=0), overlap=1.0, metric=POINT)
    print("first pass: m = %d candidates, u = %d survivors" % (info[4], info[0]), flush=True)

if "2" in args.only and args.pairs > 0:
    specs = [(10.0, -0.35, 0.5), (15.0, -0.2, 0.6), (8.0, -0.5, 0.3)]      # the tests' three partial pairs, cycled over the ids
    t0 = time.perf_counter()
    clouds = [S.make_partial_pair(i + 1, args.n, *specs[i % 3])[:2] for i in range(args.pairs)]
    so = np.concatenate([[0], np.cumsum([len(s) for s, _ in clouds])]).astype(np.int64)
    to = np.concatenate([[0], np.cumsum([len(t) for _, t in clouds])]).astype(np.int64)
    ds = torch.from_numpy(np.concatenate([s for s, _ in clouds])).cuda()
    dt = torch.from_numpy(np.concatenate([t for _, t in clouds])).cuda()
    torch.cuda.synchronize()
    print("== 2: %d partial pairs at n = %d: %d sources, %d targets in all (clouds and upload %.1f s)" % (
        len(clouds), args.n, so[-1], to[-1], time.perf_counter() - t0), flush=True)
    b = (ds.data_ptr(), so, dt.data_ptr(), to, None)
    one = [(ds.data_ptr() + 12 * int(so[i]), int(so[i + 1] - so[i]), dt.data_ptr() + 12 * int(to[i]), int(to[i + 1] - to[i]), None)
           for i in range(len(clouds))]
    runs = {"trimmed point 1.0 batch": lambda p: ctx.icp_trimmed_batch_dev(*b, p, overlap=1.0, metric=POINT)[0],
            "o2o point 1.0 batch": lambda p: ctx.icp_o2o_batch_dev(*b, p, overlap=1.0, metric=POINT)[0]}
    passes = max(2, args.passes // 4)
    med = per_pass(runs, passes)
    beh = behind_nn(runs, passes)
    print("batch: o2o - trimmed = %.1f us per whole pass, %.1f us behind the NN pass, for the whole batch" % (
        med["o2o point 1.0 batch"] - med["trimmed point 1.0 batch"], beh["o2o point 1.0 batch"] - beh["trimmed point 1.0 batch"]), flush=True)
    # one batched call against a loop of single-pair calls, PCL mode
    P = ctx.icp_params(max_iterations=60)
    whole = {"o2o point 1.0 batch": lambda: ctx.icp_o2o_batch_dev(*b, P, overlap=1.0, metric=POINT)[0],
             "o2o point 1.0 loop": lambda: [ctx.icp_o2o_dev(*a, P, overlap=1.0, metric=POINT)[0] for a in one]}
    out = {k: run() for k, run in whole.items()}
    per = {k: [] for k in whole}
    for r in range(args.rounds):
        order = list(whole)
        if r % 2:
            order.reverse()
        for k in order:
            per[k].append(timed(whole[k])[1] * 1e3)
    report(per, "ms")
    same = all(x.iterations == y.iterations and bytes(x.T) == bytes(y.T) for x, y in zip(*out.values()))
    bb, ll = per["o2o point 1.0 batch"], per["o2o point 1.0 loop"]
    print("loop / batch = %.1f x (medians); batch range %s the loop's; %d passes in all; same T and passes in both: %s" % (
        np.median(ll) / np.median(bb), "below" if max(bb) < min(ll) else "NOT below", sum(x.iterations for x in out["o2o point 1.0 batch"]), same),
        flush=True)

if "3" in args.only:
    n = 100000
    rng = np.random.default_rng(1)
    d2 = torch.from_numpy(rng.uniform(0.0, 1.0, n).astype(np.float32)).cuda()
    oi, od = torch.empty(n, dtype=torch.int32).cuda(), torch.empty(n, dtype=torch.float32).cuda()
    print("== 3: the filter alone, %d sources (the call: staging of the descriptor, three launches, the counters' copy back)" % n, flush=True)
    sets = {"all on one target": (np.zeros(n, np.int32), 25000), "uniform over 25000 targets": (rng.integers(0, 25000, n).astype(np.int32), 25000),
            "injective": (rng.permutation(n).astype(np.int32), n)}
    dev = {k: (torch.from_numpy(i).cuda(), nt) for k, (i, nt) in sets.items()}
    torch.cuda.synchronize()
    for k, (di, nt) in dev.items():
        ctx.o2o_filter_dev(di.data_ptr(), d2.data_ptr(), n, nt, 1.0, oi.data_ptr(), od.data_ptr())
    per = {k: [] for k in dev}
    for r in range(max(args.rounds, 5)):
        order = list(dev)
        if r % 2:
            order.reverse()
        for k in order:
            di, nt = dev[k]
            _, t = timed(lambda: [ctx.o2o_filter_dev(di.data_ptr(), d2.data_ptr(), n, nt, 1.0, oi.data_ptr(), od.data_ptr()) for _ in range(20)])
            per[k].append(t / 20 * 1e6)
    report(per, "us per call")
ctx.close()
