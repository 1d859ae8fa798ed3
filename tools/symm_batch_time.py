#!/usr/bin/env python3
"""Symmetric ICP for many pairs: ONE batched call (kss_icp_symm_batch_dev) against a loop of the single-pair kss_icp_symm_dev
calls over the same device-resident pairs -- the yardstick: the single-pair code does not change with the batch -- with
kss_icp_p2l_batch_dev and kss_icp_gicp_batch_dev (and, unless --no-gicp-loop, a loop of kss_icp_gicp_dev: DESIGN.md 2.15's table)
on the same batch as neighbours.  The pairs are disjoint halves of one surface (two independent samplings, as
tests/gicp_ref.halves_pair makes them), both clouds' normals precomputed (kss_normals at k = 20) and passed as device pointers.
Fixed --passes passes, no fitness pass, default nn_mode.  The variants alternate --rounds times after one warm-up round; the
median and min - max of each are reported and whether each batch's whole range lies below its loop's.  Then, for the batched
variants alone, us per pass as the difference of a 2 x passes and a passes run (setup drops out), the symmetric and the
generalized batch once more with the per-pair pass table read across the bus instead of copied per pass
(KSS_GICP_TABLE_MAPPED=1, an A/B switch), and one PCL-mode run of both symmetric forms (passes in all, whether every record
agrees).  Under rocprofv3 --kernel-trace --stats (with --quick) the per-launch times of the batched kernels come from the trace.
usage: python tools/symm_batch_time.py [--pairs 1024] [--n 10000] [--passes 20] [--rounds 5] [--quick] [--no-gicp-loop]"""
import argparse, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g
import torch
ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=1024)
ap.add_argument("--n", type=int, default=10000)
ap.add_argument("--passes", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--quick", action="store_true", help="one round and the batched variants only (for a profiler run)")
ap.add_argument("--no-gicp-loop", action="store_true", help="leave the loop of kss_icp_gicp_dev out")
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


def halves(i, n):
    M = S.bumpy(i, 2 * n)[S.permutation(3000 + i, 2 * n)]
    R = S.rot_axis_angle(S.sphere(7000 + i, 1)[0], np.deg2rad(3.0 + 9.0 * S.u01(9000 + i, 1)[0]))
    return (M[n:] @ R.T + np.array([0.02, -0.01, 0.03])).astype(np.float32), M[:n].astype(np.float32)


def mapped(on):
    if on:
        os.environ["KSS_GICP_TABLE_MAPPED"] = "1"
    else:
        os.environ.pop("KSS_GICP_TABLE_MAPPED", None)


t0 = time.perf_counter()
clouds = [halves(i, args.n) for i in range(args.pairs)]
sn = [ctx.normals(s.astype(np.float64), 20).astype(np.float32) for s, _ in clouds]
tn = [ctx.normals(t.astype(np.float64), 20).astype(np.float32) for _, t in clouds]
so = np.concatenate([[0], np.cumsum([len(s) for s, _ in clouds])]).astype(np.int64)
to = np.concatenate([[0], np.cumsum([len(t) for _, t in clouds])]).astype(np.int64)
ds = torch.from_numpy(np.concatenate([s for s, _ in clouds])).cuda()
dt = torch.from_numpy(np.concatenate([t for _, t in clouds])).cuda()
dsn = torch.from_numpy(np.concatenate(sn)).cuda()
dtn = torch.from_numpy(np.concatenate(tn)).cuda()
torch.cuda.synchronize()
print("== %d pairs of %d x %d, disjoint halves (clouds, normals and upload %.1f s)" % (args.pairs, args.n, args.n, time.perf_counter() - t0),
      flush=True)
one = [(ds.data_ptr() + 12 * int(so[i]), int(so[i + 1] - so[i]), dsn.data_ptr() + 12 * int(so[i]), dt.data_ptr() + 12 * int(to[i]),
        int(to[i + 1] - to[i]), dtn.data_ptr() + 12 * int(to[i])) for i in range(args.pairs)]


def symm_batch(p):
    return ctx.icp_symm_batch_dev(ds.data_ptr(), so, dsn.data_ptr(), dt.data_ptr(), to, dtn.data_ptr(), params=p)[0]


def symm_loop(p):
    return [ctx.icp_symm_dev(a[0], a[1], a[2], a[3], a[4], a[5], p) for a in one]


def gicp_batch(p):
    return ctx.icp_gicp_batch_dev(ds.data_ptr(), so, dsn.data_ptr(), dt.data_ptr(), to, dtn.data_ptr(), params=p)[0]


def gicp_loop(p):
    return [ctx.icp_gicp_dev(a[0], a[1], a[2], a[3], a[4], a[5], p) for a in one]


def p2l_batch(p):
    return ctx.icp_p2l_batch_dev(ds.data_ptr(), so, dt.data_ptr(), to, dtn.data_ptr(), p)


BATCHED = {"symm batch": symm_batch, "gicp batch": gicp_batch, "p2l batch": p2l_batch}
runs = dict(BATCHED)
if not args.quick:
    runs["symm loop"] = symm_loop
    if not args.no_gicp_loop:
        runs["gicp loop"] = gicp_loop
P1 = ctx.icp_params(max_iterations=args.passes, fixed_iterations=1, compute_fitness=0)
P2 = ctx.icp_params(max_iterations=2 * args.passes, fixed_iterations=1, compute_fitness=0)
out = {}
for k, run in runs.items():      # warm-up of every variant (allocations, cell list sizes) -- and what the forms computed
    res = run(P1)
    out[k] = int(np.sum([r.iterations for r in res]))
    if k in BATCHED:
        run(P2)
mapped(True)
for fn in (symm_batch, gicp_batch):
    fn(P1); fn(P2)
mapped(False)
per = {k: [] for k in runs}
for r in range(args.rounds):
    order = list(runs)
    if r % 2:
        order.reverse()
    for k in order:
        per[k].append(timed(lambda: runs[k](P1))[1] * 1e3)
for k, v in per.items():
    print("%-12s %9.2f ms  (min %.2f, max %.2f over %d rounds)   %d passes in all, %.2f us per (pair, pass)" % (
        k, float(np.median(v)), min(v), max(v), len(v), out[k], float(np.median(v)) * 1e3 / max(out[k], 1)), flush=True)
for m in ("symm", "gicp"):
    if m + " loop" in per:
        b, l = per[m + " batch"], per[m + " loop"]
        print("%s: loop / batch = %.1f x (medians); batch range %s the loop's; same passes: %s" % (
            m, np.median(l) / np.median(b), "below" if max(b) < min(l) else "NOT below", out[m + " batch"] == out[m + " loop"]), flush=True)
# us per lockstep pass of the whole batch: (2 x passes run - passes run) / passes, alternating
pp = {"symm batch": [], "symm batch, table mapped": [], "gicp batch": [], "gicp batch, table mapped": [], "p2l batch": []}
for r in range(args.rounds):
    for k in pp:
        mapped("mapped" in k)
        fn = BATCHED[k.split(",")[0]]
        a = timed(lambda: fn(P1))[1]
        b = timed(lambda: fn(P2))[1]
        pp[k].append((b - a) / args.passes * 1e6)
    mapped(False)
for k, v in pp.items():
    print("%-26s %9.1f us per pass of the batch  (min %.1f, max %.1f over %d rounds)" % (k, float(np.median(v)), min(v), max(v), len(v)), flush=True)
print("symm pass / p2l pass (medians): %.3f" % (np.median(pp["symm batch"]) / np.median(pp["p2l batch"])), flush=True)
for m in ("symm", "gicp"):
    print("%s table copy per pass (copied - mapped, medians): %.1f us" % (
        m, np.median(pp[m + " batch"]) - np.median(pp[m + " batch, table mapped"])), flush=True)
if not args.quick:   # PCL mode once: what the two forms compute
    P = ctx.icp_params(max_iterations=60)
    rb, tb = timed(lambda: symm_batch(P))
    rl, tl = timed(lambda: symm_loop(P))
    same = all(x.iterations == y.iterations and x.state == y.state and np.array_equal(x.matrix().view(np.uint32), y.matrix().view(np.uint32))
               for x, y in zip(rb, rl))
    print("PCL mode: batch %.2f ms, loop %.2f ms, %d passes in all, %d of %d converged, every T / iterations / state bit-equal: %s" % (
        tb * 1e3, tl * 1e3, sum(r.iterations for r in rb), sum(r.converged for r in rb), len(rb), same), flush=True)
ctx.close()
