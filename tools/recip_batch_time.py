#!/usr/bin/env python3
"""Reciprocal ICP for many pairs: ONE batched call (kss_icp_recip_pairs_dev) against (a) a loop of the single-pair kss_icp_recip_dev
calls -- what the batch replaces -- and (b) kss_icp_o2o_batch_dev -- which prices the reverse search -- over the same device-resident
pairs, point metric, overlap 1, fixed-iteration mode (--passes passes, no fitness pass), same build, same process, alternating,
--rounds times after one warm-up round; medians with min - max.  No threshold is fixed in advance beyond: the batch's whole range
below the loop's.  The values go into DESIGN.md 2.28.
  1  --pairs config_c3_pair-style pairs of --n points, the first fifth of each source moved off the surface by (u - 0.5) * 1.2:
     ms per whole call, the launches behind the NN pass alone from the library's own event pairs (KSS_K_CORR_REDUCE), and the
     bytes the per-pass reset sets (the batch's workspace: claim table, counters, every pair's cell counts).
  2  the filter alone on --pairs converged maps of --n x --n (the source is the target plus 1e-3 jitter): kss_recip_filter_batch_dev
     against --pairs kss_recip_filter_dev calls and against kss_o2o_filter_batch_dev.
With --baseline LIB the batched calls also run on a second context on that library (the parent commit's build), "parent " in front
of their names, alternating with this build's in the same process; the one-to-one batch is the control.
Run the process under a time limit of its own.
usage: timeout -k 10 900 python tools/recip_batch_time.py [--baseline path/to/parent/libkssicp.so] [--pairs 1024] [--n 10000] [--rounds 5] [--passes 40] [--only 12]"""
import argparse, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g
import torch
ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=1024)
ap.add_argument("--n", type=int, default=10000)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--passes", type=int, default=40)
ap.add_argument("--only", default="12")
ap.add_argument("--baseline", default=None)
args = ap.parse_args()
pkg = g.load_package(); S = pkg.synth
ctx = pkg.Context(0)
base = pkg.Context(0, lib=pkg.binding.load_library(args.baseline)) if args.baseline else None
POINT = pkg.METRIC_POINT


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, time.perf_counter() - t0


def report(per, unit):
    for k, v in per.items():
        print("%-44s %10.2f %s  (min %.2f, max %.2f over %d rounds)" % (k, float(np.median(v)), unit, min(v), max(v), len(v)), flush=True)


def alternating(runs, measure):
    per = {k: [] for k in runs}
    for r in range(args.rounds):
        order = list(runs)
        if r % 2:
            order.reverse()
        for k in order:
            per[k].append(measure(runs[k], base if k.startswith("parent ") else ctx))
    return per


def verdict(name, per, batch, loop):
    b, l = per[batch], per[loop]
    print("%s: loop / batch = %.1f x (medians); the batch's range is %s the loop's" % (
        name, np.median(l) / np.median(b), "below" if max(b) < min(l) else "NOT below"), flush=True)


def outlier_pair(i, n):
    src, tgt = S.config_c3_pair(i, n)
    k = n // 5
    u = np.stack([S.u01(9100 + i, k, j * k) for j in range(3)], axis=1)
    out = src.astype(np.float64)
    out[:k] += (u - 0.5) * 1.2
    return out.astype(np.float32), tgt


def pack(clouds):
    so = np.concatenate([[0], np.cumsum([len(s) for s, _ in clouds])]).astype(np.int64)
    to = np.concatenate([[0], np.cumsum([len(t) for _, t in clouds])]).astype(np.int64)
    ds = torch.from_numpy(np.concatenate([s for s, _ in clouds])).cuda()
    dt = torch.from_numpy(np.concatenate([t for _, t in clouds])).cuda()
    torch.cuda.synchronize()
    return so, to, ds, dt


if "1" in args.only:
    so, to, ds, dt = pack([outlier_pair(i, args.n) for i in range(args.pairs)])
    one = [(ds.data_ptr() + 12 * int(so[i]), int(so[i + 1] - so[i]), dt.data_ptr() + 12 * int(to[i]), int(to[i + 1] - to[i]), None)
           for i in range(args.pairs)]
    print("== 1: %d pairs of %d x %d, a fifth of each source off the surface; point metric, overlap 1, %d passes" % (
        args.pairs, args.n, args.n, args.passes), flush=True)
    def batch_runs(pre, cx):
        return {pre + "o2o batch": lambda p: cx.icp_o2o_batch_dev(ds.data_ptr(), so, dt.data_ptr(), to, None, p, overlap=1.0, metric=POINT),
                pre + "recip batch": lambda p: cx.icp_recip_batch_dev(ds.data_ptr(), so, dt.data_ptr(), to, None, p, overlap=1.0, metric=POINT)}
    runs = batch_runs("", ctx)
    runs["recip loop"] = lambda p: [ctx.icp_recip_dev(*a, p, overlap=1.0, metric=POINT) for a in one]
    P = ctx.icp_params(max_iterations=args.passes, fixed_iterations=1, compute_fitness=0)
    res_b, info_b = runs["recip batch"](P)      # warm-up of every variant -- and what the forms computed
    loop = runs["recip loop"](P)
    runs["o2o batch"](P)
    if base:
        runs.update(batch_runs("parent ", base))
        res_p, info_p = runs["parent recip batch"](P)
        runs["parent o2o batch"](P)
        same = all(np.array_equal(a.matrix().view(np.uint32), b.matrix().view(np.uint32)) for a, b in zip(res_b, res_p))
        print("every pair's T and info of the batch equal the parent build's bit for bit: %s" % (
            same and np.array_equal(info_b.view(np.uint64), info_p.view(np.uint64))), flush=True)
    same = all(np.array_equal(a.matrix().view(np.uint32), b[0].matrix().view(np.uint32)) and np.array_equal(i.view(np.uint64), b[1].view(np.uint64))
               for a, i, b in zip(res_b, info_b, loop))
    print("every pair's T and info of the batch equal the loop's bit for bit: %s; last pass, all pairs: m %d u %d r %d" % (
        same, info_b[:, 4].sum(), info_b[:, 5].sum(), info_b[:, 0].sum()), flush=True)
    per = alternating(runs, lambda run, cx: timed(lambda: run(P))[1] * 1e3)
    report(per, "ms per call")
    verdict("whole call", per, "recip batch", "recip loop")
    print("recip batch - o2o batch = %.2f ms per call, %.1f us per lockstep pass" % (
        np.median(per["recip batch"]) - np.median(per["o2o batch"]),
        (np.median(per["recip batch"]) - np.median(per["o2o batch"])) * 1e3 / args.passes), flush=True)

    def behind(run, cx):
        cx.profile_reset()
        run(P)
        cx.synchronize()
        ms, n = cx.profile_get(pkg.K_CORR_REDUCE)
        return ms      # of the whole call: the loop brackets passes * pairs launches groups, a batch passes of them
    for cx in (ctx, base) if base else (ctx,):
        cx.profile_enable(1)
    per = alternating(runs, behind)
    for cx in (ctx, base) if base else (ctx,):
        cx.profile_enable(0)
    report({k + ", behind the NN pass": v for k, v in per.items()}, "ms per call")
    verdict("behind the NN pass", per, "recip batch", "recip loop")
    # the per-pass reset: 8 bytes per target, 16 per pair, 4 per cell; the cells by recip_grid_of's rule, min(n / 2, 32768) aimed at
    print("the reset per pass sets at least %d bytes of claim table and counters plus 4 bytes per cell (about %d cells aimed at)" % (
        8 * int(to[-1]) + 16 * args.pairs, args.pairs * min(args.n // 2, 32768)), flush=True)

if "2" in args.only:
    n = args.n
    clouds = [S.make_pair(i, n, shape="bumpy") for i in range(args.pairs)]
    so, to, ds, dt = pack(clouds)
    print("== 2: the filter alone, %d converged maps of %d x %d" % (args.pairs, n, n), flush=True)
    idx = np.empty(int(so[-1]), np.int32); d2 = np.empty(int(so[-1]), np.float32)
    di, dd = torch.from_numpy(idx).cuda(), torch.from_numpy(d2).cuda()
    for i in range(args.pairs):      # the exact NN map of every pair, on the device
        ctx.nn_dev(ds.data_ptr() + 12 * int(so[i]), n, dt.data_ptr() + 12 * int(to[i]), n, di.data_ptr() + 4 * int(so[i]), dd.data_ptr() + 4 * int(so[i]))
    oi, od = torch.empty_like(di), torch.empty_like(dd)
    nts = np.diff(to).astype(np.int64)
    info2 = np.zeros((args.pairs, 2))
    torch.cuda.synchronize()
    def filter_runs(pre, cx):
        return {pre + "o2o filter batch": lambda: cx.L.kss_o2o_filter_batch_dev(cx.h, di.data_ptr(), dd.data_ptr(), so.ctypes.data, nts.ctypes.data,
                                                                               args.pairs, 1.0, oi.data_ptr(), od.data_ptr(), info2.ctypes.data),
                pre + "recip filter batch": lambda: cx.recip_filter_batch_dev(ds.data_ptr(), so, dt.data_ptr(), to, di.data_ptr(), dd.data_ptr(), 1.0, 0,
                                                                              oi.data_ptr(), od.data_ptr())}
    runs = filter_runs("", ctx)
    if base:
        runs.update(filter_runs("parent ", base))
        assert np.array_equal(runs["parent recip filter batch"](), runs["recip filter batch"]()) and runs["parent o2o filter batch"]() == 0
    runs.update({
            "recip filter loop": lambda: [ctx.recip_filter_dev(ds.data_ptr() + 12 * int(so[i]), n, dt.data_ptr() + 12 * int(to[i]), n,
                                                               di.data_ptr() + 4 * int(so[i]), dd.data_ptr() + 4 * int(so[i]), 1.0, 0,
                                                               oi.data_ptr() + 4 * int(so[i]), od.data_ptr() + 4 * int(so[i])) for i in range(args.pairs)]})
    info = runs["recip filter batch"]()
    loop = np.array(runs["recip filter loop"](), np.float64)
    assert runs["o2o filter batch"]() == 0
    print("{m, u, r} of every segment equal the loop's: %s; all segments: m %d u %d r %d" % (
        np.array_equal(info, loop), info[:, 0].sum(), info[:, 1].sum(), info[:, 2].sum()), flush=True)
    per = alternating(runs, lambda run, cx: timed(run)[1] * 1e3)
    report(per, "ms per call")
    verdict("filter", per, "recip filter batch", "recip filter loop")
ctx.close()
if base:
    base.close()
