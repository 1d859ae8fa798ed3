#!/usr/bin/env python3
"""Point-to-plane ICP (kss_icp_p2l_dev) against point-to-point (kss_icp_dev) on one 100k x 100k pair with the target's
computed normals: ms per pass in fixed-iteration mode (difference of a 50- and a 100-pass run, so setup and the first
pass drop out), then iterations to convergence and |T - T_true| in PCL mode.  Runs the C2 pair (sphere, R_z 10 deg)
and the same size on the bumpy surface of synth.py.  Under rocprofv3 --kernel-trace --stats the per-kernel times
come from the trace.
usage: python tools/p2l_time.py [n=100000] [passes=50]"""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g
import torch
pkg = g.load_package(); S = pkg.synth
n = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
passes = int(sys.argv[2]) if len(sys.argv) > 2 else 50
ctx = pkg.Context(0)


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, time.perf_counter() - t0


Rz = S.rot_axis_angle([0, 0, 1], np.deg2rad(10.0))
Rb = S.rot_axis_angle([0.3, -0.5, 1.0], np.deg2rad(10.0))
for name, (src, tgt), R, t in (("C2 sphere", S.config_c2(n), Rz, np.zeros(3)),
                              ("bumpy", S.make_pair(0, n, R=Rb, t=(0.02, -0.01, 0.03), shape="bumpy"), Rb, np.array([0.02, -0.01, 0.03]))):
    nrm = ctx.normals(tgt.astype(np.float64), 20).astype(np.float32)
    ds, dt, dn = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (src, tgt, nrm))
    print("== %s, %d x %d, non-finite normals: %d" % (name, n, n, int((~np.isfinite(nrm).all(1)).sum())), flush=True)
    runs = {"p2p": lambda p: ctx.icp_dev(ds.data_ptr(), n, dt.data_ptr(), n, p),
            "p2l": lambda p: ctx.icp_p2l_dev(ds.data_ptr(), n, dt.data_ptr(), n, dn.data_ptr(), p)}
    for k, run in runs.items():
        ts = []
        for it in (passes, 2 * passes):
            p = ctx.icp_params(max_iterations=it, fixed_iterations=1, compute_fitness=0)
            run(p)   # warm-up (allocations, cell list sizes)
            ts.append(timed(lambda: run(p))[1])
        print("%s: %d passes %.3f ms, %d passes %.3f ms -> %.1f us per pass" % (k, passes, ts[0] * 1e3, 2 * passes, ts[1] * 1e3,
                                                                             (ts[1] - ts[0]) / passes * 1e6), flush=True)
    R_true, t_true = R.T, -R.T @ t
    for k, run in runs.items():
        r, dt_s = timed(lambda: run(ctx.icp_params()))
        T = r.matrix()
        print("%s PCL mode: %d iterations, state %d, converged %d, fitness %.3e, |R - R_true| %.2e, |t - t_true| %.2e, %.2f ms"
              % (k, r.iterations, r.state, r.converged, r.fitness, np.abs(T[:3, :3] - R_true).max(), np.abs(T[:3, 3] - t_true).max(),
                 dt_s * 1e3), flush=True)
ctx.close()
