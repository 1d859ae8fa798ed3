#!/usr/bin/env python3
"""The recorded bits of the pair metrics (tests/golden/pair_metric_bits.npz, read by tests/test_gpu_pair_bits.py).

records(pkg, ctx, inputs(pkg)) computes, from synth, seeded numpy and the public Context methods alone, one float64 array per
case and returns {name: its uint64 bit pattern}:

  sums records   (the *_dev entry points) p2l_sums, robust_sums (point and plane, fixed and automatic scale), gicp_sums, symm_sums and symm_robust_sums
                 (fixed and automatic scale) at n in SUMS_N: one lane, a workgroup's two edges, several workgroups, and
                 2048 * 256 + 300 sources -- the first count at which the rows kernels' grid-stride loop wraps.  Every case
                 runs against one 1000-point target with its computed normals (a few made non-finite), seeded random source
                 points, source normals (a few non-finite) and correspondences (a few outside the target, which contribute
                 nothing).  The record is the sums followed by the info record where the call returns one.
  ICP results    icp_p2l, icp_trimmed and icp_robust (both metrics; the robust ones with the automatic scale), icp_gicp,
                 icp_symm and icp_symm_robust on one 2000 x 2500 pair, six passes at most, under every nn_mode: the
                 transform, the iteration count, the state, the last pass's info record where the call returns one, and
                 every pass's traced sums.

Run on the GPU on a build of the commit whose bits are the yardstick: python tests/golden/make_pair_metric_bits.py
The test recomputes records() on the build under test from the stored small clouds and asserts equality bit for bit."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "pair_metric_bits.npz")
SUMS_N = (1, 255, 257, 1000, 2048 * 256 + 300)
NT = 1000
MAX_D2 = 1.5
F32, F64 = np.float32, np.float64


def _bits(*parts):
    """float64 bit patterns of the parts laid end to end (a float32 widens exactly)."""
    return np.concatenate([np.asarray(p, F64).reshape(-1) for p in parts]).view(np.uint64)


def _unit(rng, n):
    """Seeded directions from IEEE +, *, / and sqrt alone: the same bits on every host."""
    v = rng.uniform(-1.0, 1.0, size=(n, 3))
    r = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
    return (v / r[:, None]).astype(F32)


def inputs(pkg):
    """The small clouds, made with synth (whose sin / cos may round differently from host to host: they are stored with the
    records and the test reads them back)."""
    S = pkg.synth
    src, tgt = S.make_pair(5, 2500, R=S.rot_axis_angle([0.2, 0.1, 1.0], np.deg2rad(7.0)), t=(0.02, -0.01, 0.03), shape="bumpy", n_src=2000)
    return {"input/sums_tgt": S.bumpy(41, NT).astype(F32), "input/icp_src": src, "input/icp_tgt": tgt,
            "input/Rn": S.rot_axis_angle([0.3, -0.5, 0.8], 0.7).astype(F32)}


def sums_target(ctx, inp):
    tgt = inp["input/sums_tgt"]
    tn = ctx.normals(tgt.astype(F64), 20).astype(F32)
    rng = np.random.default_rng(4100)
    tn[rng.random(NT) < 0.03] = np.nan
    tn[rng.random(NT) < 0.02, 1] = np.inf
    return tgt, tn


def sums_sources(n):
    rng = np.random.default_rng(1000003 + n)
    src = rng.uniform(-1.2, 1.2, size=(n, 3)).astype(F32)
    sn = _unit(rng, n)
    sn[rng.random(n) < 0.03] = np.nan
    sn[rng.random(n) < 0.02, 2] = -np.inf
    idx = rng.integers(0, NT, size=n).astype(np.int32)
    out = rng.random(n) < 0.02                       # outside the target on either side
    idx[out] = np.where(rng.random(int(out.sum())) < 0.5, -1 - rng.integers(0, 5, size=int(out.sum())),
                        NT + rng.integers(0, 5, size=int(out.sum()))).astype(np.int32)
    return src, sn, idx


def sums_records(pkg, ctx, inp, out):
    """Through the device-pointer entry points: the host ones reject a correspondence outside the target before the kernel sees it."""
    import torch
    tgt, tn = sums_target(ctx, inp)
    Rn = inp["input/Rn"]
    POINT, PLANE = pkg.METRIC_POINT, pkg.METRIC_PLANE
    dt, dtn = torch.from_numpy(tgt).cuda(), torch.from_numpy(tn).cuda()
    T, TN = dt.data_ptr(), dtn.data_ptr()
    for n in SUMS_N:
        src, sn, idx = sums_sources(n)
        ds, dsn, di = torch.from_numpy(src).cuda(), torch.from_numpy(sn).cuda(), torch.from_numpy(idx).cuda()
        torch.cuda.synchronize()
        s_, sn_, i_ = ds.data_ptr(), dsn.data_ptr(), di.data_ptr()
        out["p2l_sums/n%d" % n] = _bits(ctx.p2l_sums_dev(s_, T, TN, i_, n, NT, MAX_D2))
        for metric, mname in ((POINT, "point"), (PLANE, "plane")):
            for scale, sname in ((0.05, "fixed"), (0.0, "auto")):
                rp = pkg.robust_params(pkg.LOSS_TUKEY, metric, scale=scale)
                s, info = ctx.robust_sums_dev(s_, T, TN if metric == PLANE else None, i_, n, NT, MAX_D2, rp=rp)
                out["robust_sums/%s/%s/n%d" % (mname, sname, n)] = _bits(s, info)
        out["gicp_sums/n%d" % n] = _bits(ctx.gicp_sums_dev(s_, sn_, T, TN, i_, n, NT, MAX_D2, Rn=Rn))
        out["symm_sums/n%d" % n] = _bits(ctx.symm_sums_dev(s_, sn_, T, TN, i_, n, NT, MAX_D2, Rn=Rn))
        for scale, sname in ((0.05, "fixed"), (0.0, "auto")):
            rp = pkg.robust_params(pkg.LOSS_HUBER, PLANE, scale=scale)
            s, info = ctx.symm_robust_sums_dev(s_, sn_, T, TN, i_, n, NT, MAX_D2, Rn=Rn, rp=rp)
            out["symm_robust_sums/%s/n%d" % (sname, n)] = _bits(s, info)


def icp_records(pkg, ctx, inp, out):
    src, tgt = inp["input/icp_src"], inp["input/icp_tgt"]
    sn = ctx.normals(src.astype(F64), 20).astype(F32)
    tn = ctx.normals(tgt.astype(F64), 20).astype(F32)
    POINT, PLANE = pkg.METRIC_POINT, pkg.METRIC_PLANE

    def rp(loss, metric):
        return pkg.robust_params(loss, metric, scale=0.0)

    calls = {
        "icp_p2l": lambda p: ctx.icp_p2l(src, tgt, tn, params=p, trace_cap=6),
        "icp_trimmed/point": lambda p: ctx.icp_trimmed(src, tgt, None, 0.7, POINT, params=p, trace_cap=6),
        "icp_trimmed/plane": lambda p: ctx.icp_trimmed(src, tgt, tn, 0.7, PLANE, params=p, trace_cap=6),
        "icp_robust/point": lambda p: ctx.icp_robust(src, tgt, None, rp=rp(pkg.LOSS_TUKEY, POINT), params=p, trace_cap=6),
        "icp_robust/plane": lambda p: ctx.icp_robust(src, tgt, tn, rp=rp(pkg.LOSS_CAUCHY, PLANE), params=p, trace_cap=6),
        "icp_gicp": lambda p: ctx.icp_gicp(src, tgt, sn, tn, params=p, trace_cap=6),
        "icp_symm": lambda p: ctx.icp_symm(src, tgt, sn, tn, params=p, trace_cap=6),
        "icp_symm_robust": lambda p: ctx.icp_symm_robust(src, tgt, sn, tn, rp=rp(pkg.LOSS_HUBER, PLANE), params=p, trace_cap=6),
    }
    for mode, mname in ((pkg.NN_AUTO, "auto"), (pkg.NN_BRUTE, "brute"), (pkg.NN_GRID, "grid")):
        for name, call in calls.items():
            r = call(ctx.icp_params(max_iterations=6, nn_mode=mode))
            info = r.get("trim_info", r.get("robust_info", np.zeros(0)))
            out["%s/%s" % (name, mname)] = _bits(r["T"], [r["iterations"], r["state"]], info, r["trace_sums"])


def records(pkg, ctx, inp):
    out = {}
    sums_records(pkg, ctx, inp, out)
    icp_records(pkg, ctx, inp, out)
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import __graft_entry__ as graft
    pkg = graft.load_package()
    ctx = pkg.Context(0)
    inp = inputs(pkg)
    rec = records(pkg, ctx, inp)
    ctx.close()
    dst = sys.argv[1] if len(sys.argv) > 1 else PATH
    np.savez_compressed(dst, **inp, **rec)
    print("%d records, %d words -> %s" % (len(rec), sum(len(v) for v in rec.values()), dst))
