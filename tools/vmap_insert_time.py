#!/usr/bin/env python3
"""One insert into a live voxel map (kss_vmap_insert_dev) beside the only alternative a caller had before it:
kss_vmap_create_dev on the concatenation of everything mapped so far and the new cloud.  Two maps, those of DESIGN.md 2.30: the
100k-point bumpy target at leaf 0.02 (1.54e6 cells) and the 1M-point one at leaf 0.006 (5.65e7 cells), normals given.  The new
cloud: the first 100k points of the jittered copy of the target, its own normals, no pose and then a small one.
Per map and `reps` times, alternating: a fresh map of the target (not timed), ONE timed insert, the map closed; one timed create
of the concatenation, closed.  Median with the range.  Then what a scan-to-map loop does: insert after insert into ONE map.
The grown map is checked once, in bits, against kss_vmap_create of the target followed by the new points inside its box.
Every GPU step runs under a time limit of its own: a watchdog thread ends the process (exit status 124) when a step overruns.
On a tree without kss_vmap_insert the create times alone are printed (the parent's side of the comparison).
usage: python tools/vmap_insert_time.py [reps=5]"""
import os, sys, threading, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g
import torch
pkg = g.load_package(); S = pkg.synth
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
HAVE = hasattr(pkg.VoxelMap, "insert_dev")


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
    return "%.2f ms (median of %d; min %.2f, max %.2f)" % (v[len(v) // 2], len(v), v[0], v[-1])


ctx = step("context", 120, lambda: pkg.Context(0))
pose = np.eye(4, dtype=np.float32)
pose[:3, :3] = S.rot_axis_angle([0.3, -0.5, 1.0], np.deg2rad(0.2))
pose[:3, 3] = [0.002, -0.001, 0.003]
for nt, nb, leaf in ((100000, 100000, 0.02), (1000000, 100000, 0.006)):
    new, tgt = S.make_pair(0, nt, shape="bumpy", n_src=nb)
    tn = step("target normals", 120, lambda: ctx.normals(tgt.astype(np.float64), 20).astype(np.float32))
    nn = step("new normals", 120, lambda: ctx.normals(new.astype(np.float64), 20).astype(np.float32))
    cat, catn = np.concatenate([tgt, new]), np.concatenate([tn, nn])
    dt, dtn, dn, dnn, dc, dcn = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (tgt, tn, new, nn, cat, catn))
    torch.cuda.synchronize()
    fresh = lambda: ctx.vmap_dev(dt.data_ptr(), nt, leaf, dtn.data_ptr())
    create = lambda: ctx.vmap_dev(dc.data_ptr(), nt + nb, leaf, dcn.data_ptr())
    step("warm-up", 120, lambda: (fresh().close(), create().close()))
    t_ins, t_pose, t_cat, t_tgt = [], [], [], []
    for r in range(reps + 1):                             # (the first round warms up)
        if HAVE:
            for T, out in ((None, t_ins), (pose, t_pose)):
                m = step("fresh map", 120, fresh)
                info, t = step("insert", 120, lambda: timed(lambda: m.insert_dev(dn.data_ptr(), nb, dnn.data_ptr(), T)))
                out.append(t)
                if r == 0 and T is None:
                    i = m.info()
                    print("== %d new points into the map of %d at leaf %g: %d x %d x %d = %.3g cells; added %d, outside %d, %d voxels "
                          "created, %d afterwards" % (nb, nt, leaf, i[2], i[3], i[4], i[2] * i[3] * i[4], info[0], info[2], info[3], i[1]), flush=True)
                    # the map's own rule for "inside", in float32 as the library compares
                    f = np.floor((new - i[6:9].astype(np.float32)) * np.float32(i[9]))
                    inside = ((f >= 0) & (f < i[2:5].astype(np.float32))).all(1)
                    c = step("create", 120, lambda: ctx.vmap(np.concatenate([tgt, new[inside]]), leaf, normals=np.concatenate([tn, nn[inside]])))
                    (la, sa), (lb, sb) = m.read(), c.read()
                    same = np.array_equal(la, lb) and np.array_equal(sa.view(np.uint64), sb.view(np.uint64)) and np.array_equal(i, c.info())
                    print("grown map == created map of the target and the %d new points inside its box, in bits: %s" % (inside.sum(), same), flush=True)
                    c.close()
                m.close()
        for fn, out in ((create, t_cat), (fresh, t_tgt)):
            m, t = step("create", 120, lambda: timed(fn))
            out.append(t)
            m.close()
    if HAVE:
        # what a scan-to-map loop does: insert after insert into ONE map (the cloud again: from the second insert on no voxel is
        # created, N grows), so the allocator sees the same sizes call after call
        m = step("fresh map", 120, fresh)
        t_seq = [step("insert", 120, lambda: timed(lambda: m.insert_dev(dn.data_ptr(), nb, dnn.data_ptr(), None)))[1] for _ in range(reps + 1)]
        m.close()
        print("insert of %d, no pose:        %s" % (nb, med(t_ins[1:])), flush=True)
        print("  ... inserts 2 to %d into one map: %s" % (reps + 1, med(t_seq[1:])), flush=True)
        print("insert of %d, a small pose:   %s" % (nb, med(t_pose[1:])), flush=True)
    print("create of the %d concatenated: %s" % (nt + nb, med(t_cat[1:])), flush=True)
    print("create of the %d alone:        %s" % (nt, med(t_tgt[1:])), flush=True)
ctx.close()
