#!/usr/bin/env python3
"""One shift of a voxel map's window (kss_vmap_shift) beside an insert of 100k points into the same map, for
scale: a shift touches the table at occupied cells alone, an insert makes a pass over the whole of it.  Two maps, those of
DESIGN.md 2.30: the 100k-point bumpy target at leaf 0.02 (1.54e6 cells) and the 1M-point one at leaf 0.006 (5.65e7 cells),
normals given.  Per map and shift -- (1, 0, 0), (8, -5, 3) and one along x that drops about half the voxels -- `reps` times: a
fresh map of the target (not timed), ONE timed shift, the map closed: the first shift after a build, which has to allocate its
destination.  Then shift after shift of ONE map, (1, 0, 0) and back, where the records only change places.  Median with the
range.  Every GPU step runs under a time limit of its own: a watchdog thread ends the process (exit status 124) when a step
overruns.
usage: python tools/vmap_shift_time.py [reps=5]"""
import os, sys, threading, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g
import torch
pkg = g.load_package(); S = pkg.synth
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5


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
    return r, (time.perf_counter() - t0) * 1e3


def med(v):
    v = sorted(v)
    return "%.3f ms (median of %d; min %.3f, max %.3f)" % (v[len(v) // 2], len(v), v[0], v[-1])


ctx = step("context", 120, lambda: pkg.Context(0))
for nt, nb, leaf in ((100000, 100000, 0.02), (1000000, 100000, 0.006)):
    new, tgt = S.make_pair(0, nt, shape="bumpy", n_src=nb)
    tn = step("target normals", 120, lambda: ctx.normals(tgt.astype(np.float64), 20).astype(np.float32))
    nn = step("new normals", 120, lambda: ctx.normals(new.astype(np.float64), 20).astype(np.float32))
    dt, dtn, dn, dnn = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (tgt, tn, new, nn))
    torch.cuda.synchronize()
    fresh = lambda: ctx.vmap_dev(dt.data_ptr(), nt, leaf, dtn.data_ptr())
    m = step("warm-up", 120, fresh)
    i = m.info()
    lin = m.read()[0]
    cx = np.sort(lin % int(i[2]))
    half = int(cx[len(cx) // 2])                          # the shift along x that drops the voxels below the median column
    m.close()
    print("== the map of %d at leaf %g: %d x %d x %d = %.3g cells, %d voxels" % (nt, leaf, i[2], i[3], i[4], i[2] * i[3] * i[4], i[1]), flush=True)
    for k in ((1, 0, 0), (8, -5, 3), (half, 0, 0)):
        ts = []
        for r in range(reps + 1):                         # (the first round warms up)
            m = step("fresh map", 120, fresh)
            info, t = step("shift", 120, lambda: timed(lambda: m.shift(k)))
            ts.append(t)
            m.close()
        print("shift %-14s first after the build: %s; kept %d, dropped %d voxels with %d points" % (
            k, med(ts[1:]), info[0], info[1], info[2]), flush=True)
    m = step("fresh map", 120, fresh)
    ts = [step("shift", 120, lambda: timed(lambda: m.shift((1 if r % 2 == 0 else -1, 0, 0))))[1] for r in range(2 * reps + 2)]
    print("shift (1, 0, 0) and back, shifts 3 to %d of one map: %s" % (2 * reps + 2, med(ts[2:])), flush=True)
    t_ins = [step("insert", 120, lambda: timed(lambda: m.insert_dev(dn.data_ptr(), nb, dnn.data_ptr(), None)))[1] for _ in range(reps + 1)]
    print("insert of %d into the same map, inserts 2 to %d: %s" % (nb, reps + 1, med(t_ins[1:])), flush=True)
    m.close()
ctx.close()
