#!/usr/bin/env python3
"""Point-to-plane and trimmed ICP for many pairs: ONE batched call (kss_icp_p2l_batch_dev / kss_icp_trimmed_batch_dev) against a
loop of the single-pair _dev calls over the same device-resident pairs -- the yardstick: the single-pair code does not change
with the batch -- and kss_icp_batch_dev as the point-to-point floor.  PCL mode (max_iterations 60, fitness on), default nn_mode.
  A  full overlap: --pairs-a bumpy pairs of n x n (tests' _bumpy, 3 to 12 degrees): p2l, trimmed point / plane at overlap 1.0 and 0.5
  B  partial overlap: --pairs-b make_partial_pair pairs at n, trimmed 0.5, both metrics
All variants of a scenario run in one process, alternating, --rounds times after one warm-up round; the median and min - max are
reported, and whether the batch's whole range lies below the loop's.  Under rocprofv3 --kernel-trace --stats (with --quick) the
per-launch times of the three batched kernels come from the trace.
usage: python tools/pairs_batch_time.py [--pairs-a 1024] [--pairs-b 256] [--n 10000] [--rounds 5] [--quick] [--only A|B]"""
import argparse, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g
import torch
ap = argparse.ArgumentParser()
ap.add_argument("--pairs-a", type=int, default=1024)
ap.add_argument("--pairs-b", type=int, default=256)
ap.add_argument("--n", type=int, default=10000)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--only", default="AB")
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


def scenario(name, clouds, variants_of):
    """clouds: list of (src, tgt); variants_of(batch args, per-pair args) -> {name: (batch fn, loop fn or None)}"""
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
    for k, (fb, fl) in variants_of((ds.data_ptr(), so, dt.data_ptr(), to, dn.data_ptr()), one).items():
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
        print("%-28s %9.2f ms  (min %.2f, max %.2f over %d rounds)   %d passes in all, %d of %d converged" % (
            k, float(np.median(v)), min(v), max(v), len(v), out[k][0], out[k][1], len(clouds)), flush=True)
    for k in list(per):
        if k.endswith(" batch") and k[:-6] + " loop" in per:
            b, l = per[k], per[k[:-6] + " loop"]
            print("%-22s loop / batch = %.1f x (medians); batch range %s the loop's; same passes: %s" % (
                k[:-6], np.median(l) / np.median(b), "below" if max(b) < min(l) else "NOT below", out[k] == out[k[:-6] + " loop"]), flush=True)


def variants_a(b, one):
    v = {"p2p icp_batch (floor)": (lambda p: ctx.icp_batch_dev(b[0], b[1], b[2], b[3], p), None),
         "p2l": (lambda p: ctx.icp_p2l_batch_dev(*b, p), lambda p: [ctx.icp_p2l_dev(*a, p) for a in one])}
    for ov in (1.0, 0.5):
        for nm, metric in (("point", POINT), ("plane", PLANE)):
            v["trim %s %.1f" % (nm, ov)] = (
                lambda p, ov=ov, metric=metric: ctx.icp_trimmed_batch_dev(b[0], b[1], b[2], b[3], b[4] if metric == PLANE else None, p,
                                                                         overlap=ov, metric=metric)[0],
                lambda p, ov=ov, metric=metric: [ctx.icp_trimmed_dev(a[0], a[1], a[2], a[3], a[4] if metric == PLANE else None, p,
                                                                     overlap=ov, metric=metric)[0] for a in one])
    return v


def variants_b(b, one):
    v = {}
    for nm, metric in (("point", POINT), ("plane", PLANE)):
        v["trim %s 0.5" % nm] = (
            lambda p, metric=metric: ctx.icp_trimmed_batch_dev(b[0], b[1], b[2], b[3], b[4] if metric == PLANE else None, p, overlap=0.5,
                                                               metric=metric)[0],
            lambda p, metric=metric: [ctx.icp_trimmed_dev(a[0], a[1], a[2], a[3], a[4] if metric == PLANE else None, p, overlap=0.5,
                                                          metric=metric)[0] for a in one])
    return v


def bumpy(i, n):
    axis = S.sphere(7000 + i, 1)[0]
    deg = 3.0 + 9.0 * S.u01(9000 + i, 1)[0]
    return S.make_pair(i, n, R=S.rot_axis_angle(axis, np.deg2rad(deg)), t=(0.02, -0.01, 0.03), shape="bumpy")


if "A" in args.only and args.pairs_a > 0:
    scenario("A full overlap, bumpy %d x %d" % (args.n, args.n), [bumpy(i, args.n) for i in range(args.pairs_a)], variants_a)
if "B" in args.only and args.pairs_b > 0:
    specs = [(10.0, -0.35, 0.5), (15.0, -0.2, 0.6), (8.0, -0.5, 0.3)]      # the tests' three partial pairs, cycled over the ids
    scenario("B partial overlap, n = %d" % args.n,
             [S.make_partial_pair(i + 1, args.n, *specs[i % 3])[:2] for i in range(args.pairs_b)], variants_b)
ctx.close()
