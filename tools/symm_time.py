#!/usr/bin/env python3
"""Symmetric ICP (kss_icp_symm_dev) against point-to-plane (kss_icp_p2l_dev) and generalized ICP (kss_icp_gicp_dev) on
100k x 100k pairs with both clouds' computed normals: us per pass in fixed-iteration mode (difference of a 50- and a 100-pass
run, so setup, the normals and the first pass drop out; the runs of the three metrics alternate and the median of `reps`
differences is printed), then iterations to convergence and |T - T_true| in PCL mode (max_iterations 100).  Runs the two pairs
of tools/gicp_time.py (10 degrees: the source a jittered copy of the target, and disjoint halves of one surface) and the
disjoint halves turned by 65 degrees, the pair both other plane metrics lose.  Under rocprofv3 --kernel-trace --stats the
per-kernel times come from the trace.
usage: python tools/symm_time.py [n=100000] [passes=50] [reps=5]"""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g
import torch
pkg = g.load_package(); S = pkg.synth
n = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
passes = int(sys.argv[2]) if len(sys.argv) > 2 else 50
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
ctx = pkg.Context(0)


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, time.perf_counter() - t0


def halves(seed, n, R, t):
    M = S.bumpy(seed, 2 * n)[S.permutation(3000 + seed, 2 * n)]
    return (M[n:] @ R.T + t).astype(np.float32), M[:n].astype(np.float32)


tb = np.array([0.02, -0.01, 0.03])
R10, R65 = (S.rot_axis_angle([0.3, -0.5, 1.0], np.deg2rad(d)) for d in (10.0, 65.0))
for name, Rb, (src, tgt) in (("bumpy, jittered copy, 10 deg", R10, S.make_pair(0, n, R=R10, t=tb, shape="bumpy")),
                             ("bumpy, disjoint halves, 10 deg", R10, halves(0, n, R10, tb)),
                             ("bumpy, disjoint halves, 65 deg", R65, halves(0, n, R65, tb))):
    tn = ctx.normals(tgt.astype(np.float64), 20).astype(np.float32)
    sn = ctx.normals(src.astype(np.float64), 20).astype(np.float32)
    ds, dt, dsn, dtn = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (src, tgt, sn, tn))
    print("== %s, %d x %d, non-finite normals: %d + %d" % (name, n, n, int((~np.isfinite(sn).all(1)).sum()), int((~np.isfinite(tn).all(1)).sum())),
          flush=True)
    runs = {"p2l": lambda p: ctx.icp_p2l_dev(ds.data_ptr(), n, dt.data_ptr(), n, dtn.data_ptr(), p),
            "gicp": lambda p: ctx.icp_gicp_dev(ds.data_ptr(), n, dsn.data_ptr(), dt.data_ptr(), n, dtn.data_ptr(), p),
            "symm": lambda p: ctx.icp_symm_dev(ds.data_ptr(), n, dsn.data_ptr(), dt.data_ptr(), n, dtn.data_ptr(), p)}
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
    R_true, t_true = Rb.T, -Rb.T @ tb
    for k, run in runs.items():
        r, dt_s = timed(lambda: run(ctx.icp_params(max_iterations=100)))
        T = r.matrix()
        print("%s PCL mode: %d iterations, state %d, converged %d, fitness %.3e, |R - R_true| %.2e, |t - t_true| %.2e, %.2f ms"
              % (k, r.iterations, r.state, r.converged, r.fitness, np.abs(T[:3, :3] - R_true).max(), np.abs(T[:3, 3] - t_true).max(),
                 dt_s * 1e3), flush=True)
ctx.close()
