#!/usr/bin/env python3
"""The voxel-map pyramid (kss_vmap_coarsen, kss_vmap_coarsen_into, kss_icp_vgicp_c2f) on the two maps of DESIGN.md
2.30 -- the 100k-point bumpy target at leaf 0.02 and the 1M-point one at leaf 0.006, normals given --, every configuration in a
process of its own (a child started afresh; the parent never opens the GPU):
  map100k, map1m   per k in 2, 4: kss_vmap_coarsen (a fresh coarse map each time, closed again); kss_vmap_coarsen_into behind an
                   insert of 100k points into the fine map (the insert not timed); what a caller without the pyramid does
                   instead, the same insert into a SECOND box map of leaf k * leaf over the target's box; and, for scale, the
                   insert into the fine map itself and a shift of it by (1, 0, 0) and back.  Median of `reps` with the range.
  ladder           the 1M column's 100k sources from 10 degrees: the fine map alone, then the ladder 4 2 1 from
                   kss_icp_vgicp_c2f -- where each ends and what the call costs --, and kss_icp_vgicp_c2f with NULL normals beside
                   the same levels as separate kss_icp_vgicp_from calls with NULL normals (normals once against once per level).
Every GPU step runs under a time limit of its own: a watchdog thread ends the process (exit status 124) when a step overruns, and
the parent stops at the first child that fails.
usage: python tools/vmap_pyramid_time.py [reps=5]            every configuration, one child each
       python tools/vmap_pyramid_time.py CONFIG [reps=5]     one configuration, in this process"""
import os, subprocess, sys, threading, time
import numpy as np

CONFIGS = ("map100k", "map1m", "ladder")
MAPS = {"map100k": (100000, 0.02), "map1m": (1000000, 0.006)}

if len(sys.argv) < 2 or sys.argv[1] not in CONFIGS:
    for cfg in CONFIGS:
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), cfg] + sys.argv[1:2], timeout=500).returncode
        if rc != 0:
            print("configuration %s ended with status %d: stopping" % (cfg, rc), flush=True)
            sys.exit(rc)
    sys.exit(0)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g
import torch
pkg = g.load_package(); S = pkg.synth
cfg = sys.argv[1]
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
F32, F64 = np.float32, np.float64


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


def dev(*arrays):
    out = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in arrays]
    torch.cuda.synchronize()
    return out


ctx = step("context", 120, lambda: pkg.Context(0))
normals = lambda x: ctx.normals(x.astype(F64), 20).astype(F32)

if cfg in MAPS:
    nt, leaf = MAPS[cfg]
    new, tgt = S.make_pair(0, nt, shape="bumpy", n_src=100000)
    tn, nn = step("target normals", 120, lambda: normals(tgt)), step("new normals", 120, lambda: normals(new))
    dt, dtn, dn, dnn = dev(tgt, tn, new, nn)
    fresh = lambda: ctx.vmap_dev(dt.data_ptr(), nt, leaf, dtn.data_ptr())
    put = lambda mp: mp.insert_dev(dn.data_ptr(), len(new), dnn.data_ptr())
    m = step("fine map", 120, fresh)
    i = m.info()
    print("== the map of %d at leaf %g: %d x %d x %d = %.3g cells, %d voxels" % (nt, leaf, i[2], i[3], i[4], i[2] * i[3] * i[4], i[1]), flush=True)
    for k in (2, 4):
        step("warm-up", 120, lambda: m.coarsen(k).close())
        ts = []
        for _ in range(reps):
            c, t = step("coarsen", 60, lambda: timed(lambda: m.coarsen(k)))
            ts.append(t)
            ci = c.info()
            c.close()
        print("k %d: %d x %d x %d = %.3g cells, %d voxels.  kss_vmap_coarsen %s" % (k, ci[2], ci[3], ci[4], ci[2] * ci[3] * ci[4], ci[1], med(ts)), flush=True)
    for k in (2, 4):
        m.close()
        m = step("fine map", 120, fresh)
        dst = step("coarse map", 60, lambda: m.coarsen(k))
        second = step("second box map", 60, lambda: ctx.vmap_box(tgt.min(0), tgt.max(0), k * leaf))
        step("second map's fill", 60, lambda: second.insert_dev(dt.data_ptr(), nt, dtn.data_ptr()))
        step("warm-up", 60, lambda: (put(m), m.coarsen_into(dst, k), put(second)))
        tr, ts2, ti = [], [], []
        for _ in range(reps):
            ti.append(step("insert", 60, lambda: timed(lambda: put(m)))[1])
            tr.append(step("refresh", 60, lambda: timed(lambda: m.coarsen_into(dst, k)))[1])
            ts2.append(step("second insert", 60, lambda: timed(lambda: put(second)))[1])
        print("k %d: kss_vmap_coarsen_into behind an insert of 100k  %s" % (k, med(tr)))
        print("      the same insert into a second map of leaf %g   %s" % (k * leaf, med(ts2)))
        print("      the insert into the fine map itself            %s" % med(ti), flush=True)
        dst.close(); second.close()
    ts = []
    for r in range(2 * reps):
        ts.append(step("shift", 60, lambda: timed(lambda: m.shift((1, 0, 0) if r % 2 == 0 else (-1, 0, 0))))[1])
    print("a shift of the fine map by (1, 0, 0) and back           %s" % med(ts), flush=True)
    m.close()
else:
    nt, leaf = MAPS["map1m"]
    Rz = S.rot_axis_angle([0, 0, 1], np.deg2rad(10.0))
    src, tgt = S.make_pair(0, nt, R=Rz, shape="bumpy", n_src=100000)
    tn, sn = step("target normals", 120, lambda: normals(tgt)), step("source normals", 120, lambda: normals(src))
    ds, dt, dsn, dtn = dev(src, tgt, sn, tn)
    m = step("fine map", 120, lambda: ctx.vmap_dev(dt.data_ptr(), nt, leaf, dtn.data_ptr()))
    maps = [step("coarse map", 60, lambda: m.coarsen(4)), step("coarse map", 60, lambda: m.coarsen(2)), m]
    R_true = Rz.T
    err = lambda T: (np.abs(T[:3, :3] - R_true).max(), np.abs(T[:3, 3]).max())
    p = ctx.icp_params()
    alone = lambda: ctx.icp_vgicp_dev(ds.data_ptr(), len(src), dsn.data_ptr(), m, p)[0]
    c2f = lambda nrm: ctx.icp_vgicp_c2f_dev(ds.data_ptr(), len(src), nrm, maps, None, p)[0]

    def separate():
        A, out = None, []
        for mp in maps:
            out.append(ctx.icp_vgicp_from_dev(ds.data_ptr(), len(src), None, mp, A, p)[0])
            A = out[-1].matrix()
        return out

    for what, fn in (("the fine map alone", alone), ("ladder 4 2 1, normals given", lambda: c2f(dsn.data_ptr())),
                     ("ladder 4 2 1, NULL normals, one call", lambda: c2f(None)), ("ladder 4 2 1, NULL normals, three calls", separate)):
        step("warm-up", 120, fn)
        ts = []
        for _ in range(reps):
            r, t = step(what, 120, lambda: timed(fn))
            ts.append(t)
        rs = r if isinstance(r, list) else [r]
        eR, et = err(rs[-1].matrix())
        print("%-42s passes %s states %s  |R - R_true| %.2e |t| %.2e  %s" % (what, [x.iterations for x in rs], [x.state for x in rs], eR, et, med(ts)),
              flush=True)
    for x in maps[:2]:
        x.close()
    m.close()
ctx.close()
