#!/usr/bin/env python3
"""Similarity ICP for many pairs: ONE batched call (kss_icp_sim_batch_dev) against a loop of the single-pair kss_icp_sim_dev calls
over the same device-resident pairs, with kss_icp_trimmed_batch_dev on the point metric beside it.  PCL mode (max_iterations 60,
fitness on), default nn_mode.  The pairs are bumpy n x n pairs (3 to 12 degrees) whose true scales cycle over 0.9 .. 1.1, at
overlap 1.  All variants run in one process, alternating, --rounds times after one warm-up round; the median and min - max are
reported, ms per call, us per lockstep pass (the call's time over the passes of the pair that ran longest) and the ratio loop / batch.
Run the process under a time limit of its own.
usage: timeout -k 10 600 python tools/sim_batch_time.py [--pairs 256] [--n 10000] [--rounds 5] [--quick]"""
import argparse, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g
import torch
ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=256)
ap.add_argument("--n", type=int, default=10000)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--quick", action="store_true", help="one round and the batched variants only (for a profiler run)")
args = ap.parse_args()
pkg = g.load_package(); S = pkg.synth
ctx = pkg.Context(0)
if args.quick:
    args.rounds = 1


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, time.perf_counter() - t0


def bumpy(i, n):
    axis = S.sphere(7000 + i, 1)[0]
    deg = 3.0 + 9.0 * S.u01(9000 + i, 1)[0]
    scale = (0.9, 0.95, 1.0, 1.05, 1.1)[i % 5]
    return S.make_pair(i, n, R=S.rot_axis_angle(axis, np.deg2rad(deg)), scale=scale, t=(0.02, -0.01, 0.03), shape="bumpy")


clouds = [bumpy(i, args.n) for i in range(args.pairs)]
so = np.concatenate([[0], np.cumsum([len(s) for s, _ in clouds])]).astype(np.int64)
to = np.concatenate([[0], np.cumsum([len(t) for _, t in clouds])]).astype(np.int64)
ds = torch.from_numpy(np.concatenate([s for s, _ in clouds])).cuda()
dt = torch.from_numpy(np.concatenate([t for _, t in clouds])).cuda()
torch.cuda.synchronize()
one = [(ds.data_ptr() + 12 * int(so[i]), int(so[i + 1] - so[i]), dt.data_ptr() + 12 * int(to[i]), int(to[i + 1] - to[i]))
       for i in range(len(clouds))]
print("== %d pairs of %d x %d" % (len(clouds), args.n, args.n), flush=True)
sp = pkg.sim_params(overlap=1.0)
runs = {"trimmed point batch": lambda p: ctx.icp_trimmed_batch_dev(ds.data_ptr(), so, dt.data_ptr(), to, None, p, overlap=1.0,
                                                                   metric=pkg.METRIC_POINT)[0],
        "similarity batch": lambda p: ctx.icp_sim_batch_dev(ds.data_ptr(), so, dt.data_ptr(), to, p, sp=sp)[0]}
if not args.quick:
    runs["similarity loop"] = lambda p: [ctx.icp_sim_dev(*a, p, sp)[0] for a in one]
P = ctx.icp_params(max_iterations=60)
out = {}
for k, run in runs.items():      # warm-up of every variant (allocations, cell list sizes) -- and what the forms computed
    res = run(P)
    out[k] = (int(np.sum([r.iterations for r in res])), int(np.sum([r.converged for r in res])), int(np.max([r.iterations for r in res])))
per = {k: [] for k in runs}
for r in range(args.rounds):
    order = list(runs)
    if r % 2:
        order.reverse()
    for k in order:
        per[k].append(timed(lambda: runs[k](P))[1] * 1e3)
for k, v in per.items():
    print("%-22s %9.2f ms per call (min %.2f, max %.2f over %d rounds)  %7.1f us per lockstep pass (%d)   %d passes in all, %d of %d converged" % (
        k, float(np.median(v)), min(v), max(v), len(v), float(np.median(v)) * 1e3 / max(out[k][2], 1), out[k][2], out[k][0], out[k][1],
        len(clouds)), flush=True)
if "similarity loop" in per:
    b, l = per["similarity batch"], per["similarity loop"]
    print("similarity: loop / batch = %.1f x (medians); batch range %s the loop's; same passes: %s" % (
        np.median(l) / np.median(b), "below" if max(b) < min(l) else "NOT below", out["similarity batch"] == out["similarity loop"]), flush=True)
ctx.close()
