#!/usr/bin/env python3
"""Batched voxelized generalized ICP (kss_icp_vgicp_batch_dev) beside a loop of kss_icp_vgicp_dev calls over the same scans, the
same map and the same process.  The map: the 100k-point bumpy target of DESIGN.md 2.30 at leaf 0.02, normals
given.  The scans: subsets of the jittered copy of that target, each pre-moved by a small random motion inside the basin (at
most 2 degrees about a random axis and at most half a leaf along a random direction), its normals turned with it: 1024 scans of
10k points, then 64 scans of 100k points.
Per workload: the batch's records are checked against the loop's in bits, then the whole call in PCL mode (median of `reps`, with
the range), the time per pass in fixed-iteration mode without the fitness evaluation (difference of a 100- and a 50-pass run over
50, per call for the batch and summed over the scans for the loop), and the ratios loop / batch.  Batch and loop runs alternate.
Every GPU step runs under a time limit of its own: a watchdog thread ends the process (exit status 124) when a step overruns.
loop=0 leaves the loop out (the batch alone: what a kernel trace of the tool should hold).
usage: python tools/vgicp_batch_time.py [reps=5] [loop=1]"""
import os, sys, threading, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g
import torch
pkg = g.load_package(); S = pkg.synth
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
with_loop = int(sys.argv[2]) != 0 if len(sys.argv) > 2 else True
LEAF = 0.02


def step(what, limit_s, fn):
    """fn() under its own time limit (the main thread may sit in a C call, so the limit is kept by another thread)."""
    def overrun():
        print("step '%s' overran its %d s: giving up" % (what, limit_s), flush=True)
        os._exit(124)
    w = threading.Timer(limit_s, overrun)
    w.daemon = True
    w.start()
    try:
        return fn()
    finally:
        w.cancel()


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, time.perf_counter() - t0


def med(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


ctx = step("context", 120, lambda: pkg.Context(0))
src, tgt = S.make_pair(0, 100000, shape="bumpy")
tn = step("target normals", 60, lambda: ctx.normals(tgt.astype(np.float64), 20).astype(np.float32))
sn = step("source normals", 60, lambda: ctx.normals(src.astype(np.float64), 20).astype(np.float32))
dt, dtn = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (tgt, tn))
torch.cuda.synchronize()
m = step("map", 60, lambda: ctx.vmap_dev(dt.data_ptr(), len(tgt), LEAF, dtn.data_ptr()))
info = m.info()
print("map: %d targets, leaf %g, %d voxels, %.1f points each" % (len(tgt), LEAF, info[1], info[0] / info[1]), flush=True)

for nscans, ns in ((1024, 10000), (64, 100000)):
    rng = np.random.default_rng(nscans)
    scans, normals = np.empty((nscans * ns, 3), np.float32), np.empty((nscans * ns, 3), np.float32)
    for i in range(nscans):
        pick = np.sort(rng.choice(len(src), ns, replace=False)) if ns < len(src) else np.arange(len(src))
        axis = rng.normal(size=3)
        R = S.rot_axis_angle(axis, np.deg2rad(rng.uniform(0.0, 2.0)))
        d = rng.normal(size=3)
        t = d / np.linalg.norm(d) * rng.uniform(0.0, 0.5 * LEAF)
        scans[i * ns:(i + 1) * ns] = (src[pick].astype(np.float64) @ R.T + t).astype(np.float32)
        normals[i * ns:(i + 1) * ns] = (sn[pick].astype(np.float64) @ R.T).astype(np.float32)
    off = np.arange(nscans + 1, dtype=np.int64) * ns
    ds, dn = (torch.from_numpy(x).cuda() for x in (scans, normals))
    torch.cuda.synchronize()
    sp, np_ = ds.data_ptr(), dn.data_ptr()
    print("== %d scans of %d points (%.1f MB of positions)" % (nscans, ns, scans.nbytes / 1e6), flush=True)

    def batch(p):
        return ctx.icp_vgicp_batch_dev(sp, off, np_, m, p)

    def loop(p):
        return [ctx.icp_vgicp_dev(sp + 12 * int(off[i]), ns, np_ + 12 * int(off[i]), m, p) for i in range(nscans)]

    pcl = ctx.icp_params()
    fixed = [ctx.icp_params(max_iterations=it, fixed_iterations=1, compute_fitness=0) for it in (50, 100)]
    # warm-up of every shape the timed window uses, and the check that the batch computes what the loop computes
    (rb, ib), _ = step("batch warm-up", 120, lambda: timed(lambda: batch(pcl)))
    rl, _ = step("loop warm-up", 300, lambda: timed(lambda: loop(pcl) if with_loop else [(r, ib[i]) for i, r in enumerate(rb)]))
    same = all(np.array_equal(a.matrix().view(np.uint32), b[0].matrix().view(np.uint32)) and a.iterations == b[0].iterations and
               a.state == b[0].state and np.array_equal(np.array([a.fitness, a.last_mse]).view(np.uint64), np.array([b[0].fitness, b[0].last_mse]).view(np.uint64)) and
               np.array_equal(ib[i].view(np.uint64), b[1].view(np.uint64)) for i, (a, b) in enumerate(zip(rb, rl)))
    its = [r.iterations for r in rb]
    print("batch == loop in bits (T, iterations, state, fitness, last_mse, info): %s; passes min %d median %d max %d, states %s"
          % (same, min(its), sorted(its)[len(its) // 2], max(its), sorted({r.state for r in rb})), flush=True)
    for p in fixed:
        step("batch warm-up, fixed", 120, lambda: batch(p))
    if with_loop:
        step("loop warm-up, fixed", 300, lambda: loop(fixed[0]))
    whole = {"batch": [], "loop": []}
    per = {"batch": [], "loop": []}
    for _ in range(reps):
        for k, run in (("batch", batch), ("loop", loop))[:2 if with_loop else 1]:
            whole[k].append(step(k + " PCL mode", 300, lambda: timed(lambda: run(pcl))[1]) * 1e3)
            ts = [step(k + " fixed", 600, lambda: timed(lambda: run(p))[1]) for p in fixed]
            per[k].append((ts[1] - ts[0]) / 50 * 1e6)
    wb, pb = med(whole["batch"]), med(per["batch"])
    if not with_loop:
        print("batch alone: whole call %.2f ms (min %.2f, max %.2f), per lockstep pass %.1f us (min %.1f, max %.1f)" % (wb + pb), flush=True)
        continue
    wl, pl = med(whole["loop"]), med(per["loop"])
    print("whole call, PCL mode: batch %.2f ms (min %.2f, max %.2f), loop %.2f ms (min %.2f, max %.2f): loop / batch %.1f"
          % (wb + wl + (wl[0] / wb[0],)), flush=True)
    print("per lockstep pass: batch %.1f us (min %.1f, max %.1f), loop %.1f us summed over the scans (min %.1f, max %.1f): loop / batch %.1f"
          % (pb + pl + (pl[0] / pb[0],)), flush=True)
    print("per pass and scan: batch %.2f us, loop %.2f us; batch: %.2f ns per source and pass" % (pb[0] / nscans, pl[0] / nscans, pb[0] * 1e3 / (nscans * ns)), flush=True)
    del ds, dn
m.close()
ctx.close()
