"""Independent numpy restatement of trimmed ICP (include/kssicp.h at kss_icp_trimmed).

Test infrastructure only; it shares no code with the library.  Candidates, the rank k, the cut tau by numpy.sort and the
kept mask are restated here; the point sums are numpy sums solved by the oracle's rigid_from_sums; the plane sums, their
solve and PCL's criteria come from tests/p2l_ref.py; the exact NN, transformCloud and the Matrix4f product from the oracle."""
import math

import numpy as np

import p2l_ref as PR

F32, F64 = np.float32, np.float64
NINFO = 4
POINT, PLANE = 0, 1


def rank(m, overlap):
    """k: the Python expression of kss_trim_rank (float * float is one IEEE multiplication)."""
    return 0 if m == 0 else max(1, int(math.ceil(float(overlap) * float(m))))


def threshold(d2, max_d2, overlap):
    """(candidate mask, m, k, tau as float32, mask of the candidates <= tau)."""
    d2 = np.asarray(d2, F32).reshape(-1)
    with np.errstate(invalid="ignore"):
        d = d2.astype(F64)
        cand = (d >= 0.0) & (d <= max_d2)
    m = int(cand.sum())
    k = rank(m, overlap)
    if m == 0:
        return cand, 0, 0, F32(0.0), np.zeros(len(d2), bool)
    tau = np.sort(np.abs(d2[cand]))[k - 1]      # (abs: -0.0 counts as +0.0; the candidates are >= 0)
    with np.errstate(invalid="ignore"):
        kept = cand & (d2 <= tau)
    return cand, m, k, F32(tau), kept


def point_sums(cur, tgt, idx, kept, d2):
    """The KSS_NSUMS record over the kept correspondences (slots 17..19 stay 0)."""
    s = cur[kept].astype(F64)
    q = tgt[idx[kept]].astype(F64)
    out = np.zeros(20, F64)
    out[0] = kept.sum()
    out[1:4] = s.sum(0)
    out[4:7] = q.sum(0)
    out[7:16] = (s[:, :, None] * q[:, None, :]).sum(0).reshape(9)
    out[16] = d2[kept].astype(F64).sum()
    return out


def icp_trimmed(O, src, tgt, nrm, overlap, metric, **kw):
    """PCL align() with the trimmed step on the oracle's exact NN.  Returns the dictionary of Context.icp_trimmed."""
    p = dict(PR.DEFAULTS, **kw)
    src, tgt = np.asarray(src, F32), np.asarray(tgt, F32)
    max_d2 = p["max_corr_dist"] * p["max_corr_dist"]
    cur = src.copy()
    fin = np.eye(4, dtype=F32)
    crit = {"prev_mse": np.finfo(F64).max}
    iters, state, converged, last_mse = 0, 0, False, 0.0
    trace_Tk, trace_sums, trace_trim = [], [], []
    info = np.zeros(NINFO, F64)
    while p["max_iterations"] > 0:
        idx, d2 = O.nn_brute(cur, tgt)
        _, m, k, tau, kept = threshold(d2, max_d2, overlap)
        if metric == PLANE:
            # the cut is taken on d2 alone; p2l_ref.sums then drops the correspondences without a finite normal
            s, _ = PR.sums(cur[kept], tgt, nrm, idx[kept], np.inf, d2=d2[kept])
            s[29] = d2.astype(F64).sum()      # slot 29 runs over all sources
        else:
            s = point_sums(cur, tgt, idx, kept, d2)
        info = np.array([m, k, float(tau), s[0]], F64)
        if int(s[0]) < p["min_correspondences"]:
            state = PR.STATE_NO_CORRESPONDENCES
            break
        if metric == PLANE:
            Tk, degenerate = PR.rigid(s)
            if degenerate:
                state = PR.STATE_DEGENERATE
                break
            mse = s[28] / s[0]
        else:
            Tk = O.rigid_from_sums(s)
            mse = s[16] / s[0]
        fin = O.mat4_mul(Tk, fin)
        iters += 1
        last_mse = mse
        trace_Tk.append(Tk); trace_sums.append(s); trace_trim.append(info)
        state = PR.has_converged(crit, iters, Tk, mse, p)
        if state:
            converged = True
            break
        cur = O.transform_points_f32(Tk, cur)
    _, d2 = O.nn_brute(O.transform_points_f32(fin, src), tgt)
    ncol = PR.NSUMS if metric == PLANE else 20
    return {"T": fin, "iterations": iters, "converged": converged, "state": state, "last_mse": last_mse,
            "fitness": d2.astype(F64).sum() / len(src), "trace_Tk": np.array(trace_Tk).reshape(-1, 4, 4),
            "trace_sums": np.array(trace_sums).reshape(-1, ncol), "trace_trim": np.array(trace_trim).reshape(-1, NINFO),
            "trim_info": info}
