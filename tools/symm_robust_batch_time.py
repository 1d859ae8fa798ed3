#!/usr/bin/env python3
"""Robust symmetric ICP for many pairs: ONE batched call (kss_icp_symm_robust_batch_dev) against a loop of the single-pair
kss_icp_symm_robust_dev calls over the same device-resident pairs -- the yardstick: the single-pair code does not change with the
batch -- with kss_icp_symm_batch_dev and kss_icp_robust_batch_dev (plane metric) on the same batch as neighbours.  Tukey weights, at
the automatic scale and at a fixed one.  Two scenes, both clouds' normals precomputed (kss_normals at k = 20) and passed as device
pointers:
  halves   --pairs pairs of --n x --n points, disjoint halves of one surface (as tests/gicp_ref.halves_pair makes them) 3 to 12
           degrees apart, the first 20 % of every source pushed off the surface (as tests/symm_robust_ref.outliers does it);
  views    --views pairs of partial views (as tests/symm_robust_ref.scene_b makes them, from 2 x --n points): the target keeps
           x > -0.5, the source x < 0.5, 65 degrees apart.
Per scene: fixed --passes passes, no fitness pass, default nn_mode; the variants alternate --rounds times after one warm-up round;
the median and min - max of each are reported and whether each batch's whole range lies below its loop's with the same number of
passes in both.  Then, for the batched variants alone, us per lockstep pass as the difference of a 2 x passes and a passes run
(setup drops out), and one PCL-mode run (max_iterations 60) of both forms at either scale: the pass totals, and whether every T,
iteration count and state is bit-equal.  Under rocprofv3 --kernel-trace --stats (with --quick) the per-launch times of the batched
kernels come from the trace.
usage: python tools/symm_robust_batch_time.py [--pairs 1024] [--views 256] [--n 10000] [--passes 20] [--rounds 5] [--scale 0.05]
                                              [--scene both|halves|views] [--quick]"""
import argparse, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g
import torch
ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=1024)
ap.add_argument("--views", type=int, default=256)
ap.add_argument("--n", type=int, default=10000)
ap.add_argument("--passes", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--scale", type=float, default=0.05, help="the fixed scale")
ap.add_argument("--scene", choices=("both", "halves", "views"), default="both")
ap.add_argument("--quick", action="store_true", help="one round and the batched variants only (for a profiler run)")
args = ap.parse_args()
pkg = g.load_package(); S = pkg.synth
ctx = pkg.Context(0)
if args.quick:
    args.rounds = 1
AXIS = [0.3, -0.5, 1.0]
T3 = np.array([0.02, -0.01, 0.03])
TUKEY, PLANE = pkg.LOSS_TUKEY, pkg.METRIC_PLANE
rp_fixed = pkg.robust_params(TUKEY, PLANE, scale=args.scale)
rp_auto = pkg.robust_params(TUKEY, PLANE)


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, time.perf_counter() - t0


def halves(i, n):
    M = S.bumpy(i, 2 * n)[S.permutation(3000 + i, 2 * n)]
    R = S.rot_axis_angle(S.sphere(7000 + i, 1)[0], np.deg2rad(3.0 + 9.0 * S.u01(9000 + i, 1)[0]))
    src = M[n:] @ R.T + T3
    k = int(0.2 * n)
    u = np.stack([S.u01(9000 + i, k, j * k) for j in range(3)], axis=1)
    src[:k] += (u - 0.5) * 2.0 * 0.3
    return src.astype(np.float32), M[:n].astype(np.float32)


def views(i, n):
    M = S.bumpy(i, 2 * n)[S.permutation(3000 + i, 2 * n)]
    A, B = M[:n], M[n:]
    R = S.rot_axis_angle(AXIS, np.deg2rad(65.0))
    return (B[B[:, 0] < 0.5] @ R.T + T3).astype(np.float32), A[A[:, 0] > -0.5].astype(np.float32)


def bit_equal(a, b):
    return all(x.iterations == y.iterations and x.state == y.state and np.array_equal(x.matrix().view(np.uint32), y.matrix().view(np.uint32))
               for x, y in zip(a, b))


def scene(name, make, npairs):
    t0 = time.perf_counter()
    clouds = [make(i, args.n) for i in range(npairs)]
    sn = [ctx.normals(s.astype(np.float64), 20).astype(np.float32) for s, _ in clouds]
    tn = [ctx.normals(t.astype(np.float64), 20).astype(np.float32) for _, t in clouds]
    so = np.concatenate([[0], np.cumsum([len(s) for s, _ in clouds])]).astype(np.int64)
    to = np.concatenate([[0], np.cumsum([len(t) for _, t in clouds])]).astype(np.int64)
    ds = torch.from_numpy(np.concatenate([s for s, _ in clouds])).cuda()
    dt = torch.from_numpy(np.concatenate([t for _, t in clouds])).cuda()
    dsn = torch.from_numpy(np.concatenate(sn)).cuda()
    dtn = torch.from_numpy(np.concatenate(tn)).cuda()
    torch.cuda.synchronize()
    print("== %s: %d pairs, %d source and %d target points in all (clouds, normals and upload %.1f s)" % (
        name, npairs, so[-1], to[-1], time.perf_counter() - t0), flush=True)
    one = [(ds.data_ptr() + 12 * int(so[i]), int(so[i + 1] - so[i]), dsn.data_ptr() + 12 * int(so[i]), dt.data_ptr() + 12 * int(to[i]),
            int(to[i + 1] - to[i]), dtn.data_ptr() + 12 * int(to[i])) for i in range(npairs)]

    def sr_batch(rp):
        return lambda p: ctx.icp_symm_robust_batch_dev(ds.data_ptr(), so, dsn.data_ptr(), dt.data_ptr(), to, dtn.data_ptr(), params=p, rp=rp)[0]

    def sr_loop(rp):
        return lambda p: [ctx.icp_symm_robust_dev(a[0], a[1], a[2], a[3], a[4], a[5], p, rp=rp)[0] for a in one]

    BATCHED = {
        "symm robust batch, automatic": sr_batch(rp_auto),
        "symm robust batch, fixed": sr_batch(rp_fixed),
        "symm batch": lambda p: ctx.icp_symm_batch_dev(ds.data_ptr(), so, dsn.data_ptr(), dt.data_ptr(), to, dtn.data_ptr(), params=p)[0],
        "plane robust batch, automatic": lambda p: ctx.icp_robust_batch_dev(ds.data_ptr(), so, dt.data_ptr(), to, dtn.data_ptr(), p, rp=rp_auto)[0],
        "plane robust batch, fixed": lambda p: ctx.icp_robust_batch_dev(ds.data_ptr(), so, dt.data_ptr(), to, dtn.data_ptr(), p, rp=rp_fixed)[0],
    }
    runs = dict(BATCHED)
    if not args.quick:
        runs["symm robust loop, automatic"] = sr_loop(rp_auto)
        runs["symm robust loop, fixed"] = sr_loop(rp_fixed)
    P1 = ctx.icp_params(max_iterations=args.passes, fixed_iterations=1, compute_fitness=0)
    P2 = ctx.icp_params(max_iterations=2 * args.passes, fixed_iterations=1, compute_fitness=0)
    out, first = {}, {}
    for k, run in runs.items():      # warm-up of every variant (allocations, cell list sizes) -- and what the forms computed
        first[k] = run(P1)
        out[k] = int(np.sum([r.iterations for r in first[k]]))
        if k in BATCHED:
            run(P2)
    per = {k: [] for k in runs}
    for r in range(args.rounds):
        order = list(runs)
        if r % 2:
            order.reverse()
        for k in order:
            per[k].append(timed(lambda: runs[k](P1))[1] * 1e3)
    for k, v in per.items():
        print("%-30s %9.2f ms  (min %.2f, max %.2f over %d rounds)   %d passes in all, %.2f us per (pair, pass)" % (
            k, float(np.median(v)), min(v), max(v), len(v), out[k], float(np.median(v)) * 1e3 / max(out[k], 1)), flush=True)
    for m in ("automatic", "fixed"):
        bk, lk = "symm robust batch, " + m, "symm robust loop, " + m
        if lk in per:
            b, l = per[bk], per[lk]
            print("%s: loop / batch = %.1f x (medians); batch range %s the loop's; same passes: %s; every T / iterations / state bit-equal: %s" % (
                m, np.median(l) / np.median(b), "below" if max(b) < min(l) else "NOT below", out[bk] == out[lk],
                bit_equal(first[bk], first[lk])), flush=True)
    # us per lockstep pass of the whole batch: (2 x passes run - passes run) / passes, alternating
    pp = {k: [] for k in BATCHED}
    for r in range(args.rounds):
        for k in pp:
            a = timed(lambda: BATCHED[k](P1))[1]
            b = timed(lambda: BATCHED[k](P2))[1]
            pp[k].append((b - a) / args.passes * 1e6)
    for k, v in pp.items():
        print("%-30s %9.1f us per pass of the batch  (min %.1f, max %.1f over %d rounds)" % (k, float(np.median(v)), min(v), max(v), len(v)), flush=True)
    for a, b in (("symm robust batch, fixed", "symm batch"), ("symm robust batch, automatic", "plane robust batch, automatic")):
        apart = min(pp[a]) > max(pp[b]) or max(pp[a]) < min(pp[b])
        print("%s / %s (medians): %.3f, ranges %s" % (a, b, np.median(pp[a]) / np.median(pp[b]), "apart" if apart else "overlap"), flush=True)
    if not args.quick:   # PCL mode once per scale: what the two forms compute
        P = ctx.icp_params(max_iterations=60)
        for m, rp in (("automatic", rp_auto), ("fixed", rp_fixed)):
            rb, tb = timed(lambda: sr_batch(rp)(P))
            rl, tl = timed(lambda: sr_loop(rp)(P))
            print("PCL mode, %s: batch %.2f ms, loop %.2f ms, %d / %d passes in all, %d of %d converged, every T / iterations / state bit-equal: %s" % (
                m, tb * 1e3, tl * 1e3, sum(r.iterations for r in rb), sum(r.iterations for r in rl), sum(r.converged for r in rb), len(rb),
                bit_equal(rb, rl)), flush=True)


if args.scene in ("both", "halves"):
    scene("halves with 20 % outliers", halves, args.pairs)
if args.scene in ("both", "views"):
    scene("partial views, 65 degrees", views, args.views)
ctx.close()
