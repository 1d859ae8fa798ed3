#!/usr/bin/env python3
"""Robust ICP for many pairs: ONE batched call (kss_icp_robust_batch_dev) against a loop of the single-pair kss_icp_robust_dev calls
over the same device-resident pairs -- the yardstick: the single-pair code does not change with the batch -- with
kss_icp_trimmed_batch_dev at overlap 0.5 and kss_icp_p2l_batch_dev from the same process as neighbours.  PCL mode (max_iterations
60, fitness on), default nn_mode.
  A  full overlap: --pairs-a bumpy pairs of n x n (tools/pairs_batch_time.py's scenario A)
  C  gross outliers: --pairs-c make_outlier_pair(i, n, deg, 0.3) pairs
Each scenario runs Huber, Tukey and Cauchy at the automatic scale and Huber at a fixed scale, with both metrics.  All variants of
a scenario run in one process, alternating, --rounds times after one warm-up round; the median and min - max are reported, whether
the batch's whole range lies below the loop's, the passes in all, whether both forms ran the same number of passes, and us per
(pair, pass).  Under rocprofv3 --kernel-trace --stats (with --quick) the per-launch times of the batched kernels come from the trace.
usage: python tools/robust_batch_time.py [--pairs-a 1024] [--pairs-c 256] [--n 10000] [--rounds 5] [--quick] [--only A|C]"""
import argparse, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g
import torch
ap = argparse.ArgumentParser()
ap.add_argument("--pairs-a", type=int, default=1024)
ap.add_argument("--pairs-c", type=int, default=256)
ap.add_argument("--n", type=int, default=10000)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--only", default="AC")
ap.add_argument("--fixed-scale", type=float, default=0.02)
ap.add_argument("--quick", action="store_true", help="one round and the batched variants only (for a profiler run)")
args = ap.parse_args()
pkg = g.load_package(); S = pkg.synth
ctx = pkg.Context(0)
POINT, PLANE = pkg.METRIC_POINT, pkg.METRIC_PLANE
if args.quick:
    args.rounds = 1


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, time.perf_counter() - t0


def variants(b, one):
    """b: the batch's (src, src_off, tgt, tgt_off, normals) device arguments, one: the same per pair -> {name: (batch fn, loop fn or None)}"""
    v = {"p2l (neighbour)": (lambda p: ctx.icp_p2l_batch_dev(*b, p), None)}
    for nm, metric in (("point", POINT), ("plane", PLANE)):
        v["trim %s 0.5 (neighbour)" % nm] = (
            lambda p, metric=metric: ctx.icp_trimmed_batch_dev(b[0], b[1], b[2], b[3], b[4] if metric == PLANE else None, p, overlap=0.5,
                                                               metric=metric)[0], None)
    specs = [("huber", pkg.LOSS_HUBER, 0.0), ("tukey", pkg.LOSS_TUKEY, 0.0), ("cauchy", pkg.LOSS_CAUCHY, 0.0),
             ("huber", pkg.LOSS_HUBER, args.fixed_scale)]
    for ln, loss, scale in specs:
        for nm, metric in (("point", POINT), ("plane", PLANE)):
            rp = pkg.robust_params(loss, metric, scale=scale)
            v["%s %s %s" % (ln, nm, "fixed" if scale else "auto")] = (
                lambda p, rp=rp, metric=metric: ctx.icp_robust_batch_dev(b[0], b[1], b[2], b[3], b[4] if metric == PLANE else None, p, rp=rp)[0],
                lambda p, rp=rp, metric=metric: [ctx.icp_robust_dev(a[0], a[1], a[2], a[3], a[4] if metric == PLANE else None, p, rp=rp)[0]
                                                 for a in one])
    return v


def scenario(name, clouds):
    t0 = time.perf_counter()
    nrm = [ctx.normals(t.astype(np.float64), 20).astype(np.float32) for _, t in clouds]
    so = np.concatenate([[0], np.cumsum([len(s) for s, _ in clouds])]).astype(np.int64)
    to = np.concatenate([[0], np.cumsum([len(t) for _, t in clouds])]).astype(np.int64)
    ds = torch.from_numpy(np.concatenate([s for s, _ in clouds])).cuda()
    dt = torch.from_numpy(np.concatenate([t for _, t in clouds])).cuda()
    dn = torch.from_numpy(np.concatenate(nrm)).cuda()
    torch.cuda.synchronize()
    print("== %s: %d pairs, %d sources, %d targets in all (normals and upload %.1f s)" % (name, len(clouds), so[-1], to[-1], time.perf_counter() - t0), flush=True)
    one = [(ds.data_ptr() + 12 * int(so[i]), int(so[i + 1] - so[i]), dt.data_ptr() + 12 * int(to[i]), int(to[i + 1] - to[i]),
            dn.data_ptr() + 12 * int(to[i])) for i in range(len(clouds))]
    runs = {}
    for k, (fb, fl) in variants((ds.data_ptr(), so, dt.data_ptr(), to, dn.data_ptr()), one).items():
        runs[k + " batch" if fl else k] = fb
        if fl and not args.quick:
            runs[k + " loop"] = fl
    P = ctx.icp_params(max_iterations=60)
    out = {}
    for k, run in runs.items():      # warm-up of every variant (allocations, cell list sizes) -- and what the two forms computed
        res = run(P)
        out[k] = (int(np.sum([r.iterations for r in res])), int(np.sum([r.converged for r in res])))
    per = {k: [] for k in runs}
    for r in range(args.rounds):
        order = list(runs)
        if r % 2:
            order.reverse()
        for k in order:
            per[k].append(timed(lambda: runs[k](P))[1] * 1e3)
    for k, v in per.items():
        print("%-30s %9.2f ms  (min %.2f, max %.2f over %d rounds)   %d passes in all, %d of %d converged, %.2f us per (pair, pass)" % (
            k, float(np.median(v)), min(v), max(v), len(v), out[k][0], out[k][1], len(clouds), float(np.median(v)) * 1e3 / max(out[k][0], 1)), flush=True)
    for k in list(per):
        if k.endswith(" batch") and k[:-6] + " loop" in per:
            b, l = per[k], per[k[:-6] + " loop"]
            print("%-22s loop / batch = %.1f x (medians); batch range %s the loop's; same passes: %s" % (
                k[:-6], np.median(l) / np.median(b), "below" if max(b) < min(l) else "NOT below", out[k] == out[k[:-6] + " loop"]), flush=True)


def bumpy(i, n):
    axis = S.sphere(7000 + i, 1)[0]
    deg = 3.0 + 9.0 * S.u01(9000 + i, 1)[0]
    return S.make_pair(i, n, R=S.rot_axis_angle(axis, np.deg2rad(deg)), t=(0.02, -0.01, 0.03), shape="bumpy")


if "A" in args.only and args.pairs_a > 0:
    scenario("A full overlap, bumpy %d x %d" % (args.n, args.n), [bumpy(i, args.n) for i in range(args.pairs_a)])
if "C" in args.only and args.pairs_c > 0:
    scenario("C gross outliers (30 %% of the sources), n = %d" % args.n,
             [S.make_outlier_pair(i, args.n, 3.0 + 9.0 * S.u01(9000 + i, 1)[0], 0.3)[:2] for i in range(args.pairs_c)])
ctx.close()
