#!/usr/bin/env python3
"""Voxelized generalized ICP (kss_vmap_create_dev, kss_icp_vgicp_dev) beside generalized ICP (kss_icp_gicp_dev) on the same pairs,
normals given: the map build time (median of `reps` builds, each destroyed again), then us per pass in fixed-iteration mode
(difference of a 50- and a 100-pass run, so setup and the first pass drop out; the runs of the two methods alternate and the
median of `reps` differences is printed), then iterations to convergence and |T - T_true| in PCL mode.  Two pairs: config_c2's
size, 100k x 100k, and a 100k source against a 1M-point target -- the line that shows a pass's independence from the map's size.
KSS_VGICP_UNFUSED=1 (read once per process) times the form whose move is a launch of its own.
A third argument sets the map's neighbourhood (1, 7 or 27); without it the map stays at 1 and nothing more is printed.
usage: python tools/vgicp_time.py [passes=50] [reps=5] [neighbourhood=1]"""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g
import torch
pkg = g.load_package(); S = pkg.synth
passes = int(sys.argv[1]) if len(sys.argv) > 1 else 50
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
nb = int(sys.argv[3]) if len(sys.argv) > 3 else None
ctx = pkg.Context(0)
print("move: %s" % ("a launch of its own (KSS_VGICP_UNFUSED)" if os.environ.get("KSS_VGICP_UNFUSED", "0") not in ("", "0") else "fused into the rows launch"))


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, time.perf_counter() - t0


Rz = S.rot_axis_angle([0, 0, 1], np.deg2rad(10.0))
for nt, ns, leaf in ((100000, 100000, 0.02), (1000000, 100000, 0.006)):
    src, tgt = S.make_pair(0, nt, R=Rz, shape="bumpy", n_src=ns)
    tn = ctx.normals(tgt.astype(np.float64), 20).astype(np.float32)
    sn = ctx.normals(src.astype(np.float64), 20).astype(np.float32)
    ds, dt, dsn, dtn = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (src, tgt, sn, tn))
    torch.cuda.synchronize()
    build = []
    for _ in range(reps + 1):   # (the first build warms up)
        m, t = timed(lambda: ctx.vmap_dev(dt.data_ptr(), nt, leaf, dtn.data_ptr()))
        build.append(t * 1e3)
        m.close()
    m = ctx.vmap_dev(dt.data_ptr(), nt, leaf, dtn.data_ptr())
    if nb is not None:
        m.set_neighbourhood(nb)
        print("neighbourhood: %d" % m.neighbourhood, flush=True)
    info = m.info()
    lin, stats = m.read()
    b = sorted(build[1:])
    print("== bumpy, jittered copy: %d sources against %d targets, leaf %g: dims %d x %d x %d = %.3g cells, %d voxels, %.1f points each, largest %d"
          % (ns, nt, leaf, info[2], info[3], info[4], info[2] * info[3] * info[4], info[1], info[0] / info[1], int(stats[:, 0].max())), flush=True)
    print("map build: %.2f ms (median of %d; min %.2f, max %.2f)" % (b[len(b) // 2], reps, b[0], b[-1]), flush=True)
    runs = {"gicp": lambda p: ctx.icp_gicp_dev(ds.data_ptr(), ns, dsn.data_ptr(), dt.data_ptr(), nt, dtn.data_ptr(), p),
            "vgicp": lambda p: ctx.icp_vgicp_dev(ds.data_ptr(), ns, dsn.data_ptr(), m, p)[0]}
    ps = [ctx.icp_params(max_iterations=it, fixed_iterations=1, compute_fitness=0) for it in (passes, 2 * passes)]
    for run in runs.values():   # warm-up (allocations, cell list sizes)
        for p in ps:
            run(p)
    per = {k: [] for k in runs}
    for _ in range(reps):
        for k, run in runs.items():
            ts = [timed(lambda: run(p))[1] for p in ps]
            per[k].append((ts[1] - ts[0]) / passes * 1e6)
    for k in runs:
        v = sorted(per[k])
        print("%s: %.1f us per pass (median of %d; min %.1f, max %.1f)" % (k, v[len(v) // 2], reps, v[0], v[-1]), flush=True)
    R_true = Rz.T
    for k, run in runs.items():
        r, dt_s = timed(lambda: run(ctx.icp_params()))
        T = r.matrix()
        print("%s PCL mode: %d iterations, state %d, converged %d, fitness %.3e, |R - R_true| %.2e, |t| %.2e, %.2f ms"
              % (k, r.iterations, r.state, r.converged, r.fitness, np.abs(T[:3, :3] - R_true).max(), np.abs(T[:3, 3]).max(), dt_s * 1e3), flush=True)
    m.close()
ctx.close()
