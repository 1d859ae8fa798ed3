"""Independent numpy restatement of one-to-one ICP (include/kssicp.h at kss_icp_o2o).

Test infrastructure only; it shares no code with the library.  The filter is a lexsort -- by target, then by the masked float bits
of d2, then by source index -- whose first row per target is the winner; the loop is tests/trim_ref.py's trimmed loop with the
filter in front of the selection: the selection, the sums, the solves and PCL's criteria are the ones that file uses."""
import numpy as np

import p2l_ref as PR
import trim_ref as TR

F32, F64 = np.float32, np.float64
NINFO = 5
POINT, PLANE = TR.POINT, TR.PLANE
QNAN = np.uint32(0x7FC00000)


def candidates(idx, d2, nt, max_d2):
    idx = np.asarray(idx, np.int32).reshape(-1)
    d2 = np.asarray(d2, F32).reshape(-1)
    with np.errstate(invalid="ignore"):
        d = d2.astype(F64)
        return (idx >= 0) & (idx.astype(np.int64) < nt) & (d >= 0.0) & (d <= max_d2)


def filter(idx, d2, nt, max_d2):
    """(idx_f int32, d2_f float32, m, u): of the candidates that chose one target the one with the smallest d2 (-0.0f as +0.0f),
    ties to the lowest source index, keeps idx and d2; the others get -1 and the quiet NaN; non-candidates pass through."""
    idx = np.asarray(idx, np.int32).reshape(-1)
    d2 = np.asarray(d2, F32).reshape(-1)
    cand = candidates(idx, d2, nt, max_d2)
    ci = np.nonzero(cand)[0]
    bits = d2.view(np.uint32)[ci] & np.uint32(0x7FFFFFFF)
    order = np.lexsort((ci, bits, idx[ci]))          # the last key is the primary one
    ci = ci[order]
    tj = idx[ci]
    first = np.ones(len(ci), bool)
    first[1:] = tj[1:] != tj[:-1]
    winners = ci[first]
    lose = cand.copy()
    lose[winners] = False
    idx_f, d2_f = idx.copy(), d2.copy()
    idx_f[lose] = -1
    d2_f.view(np.uint32)[lose] = QNAN
    return idx_f, d2_f, int(cand.sum()), int(len(winners))


def icp_o2o(O, src, tgt, nrm, overlap, metric, **kw):
    """PCL align() with the one-to-one trimmed step on the oracle's exact NN.  Returns the dictionary of Context.icp_o2o."""
    p = dict(PR.DEFAULTS, **kw)
    src, tgt = np.asarray(src, F32), np.asarray(tgt, F32)
    nt = len(tgt)
    max_d2 = p["max_corr_dist"] * p["max_corr_dist"]
    cur = src.copy()
    fin = np.eye(4, dtype=F32)
    crit = {"prev_mse": np.finfo(F64).max}
    iters, state, converged, last_mse = 0, 0, False, 0.0
    trace_Tk, trace_sums, trace_o2o = [], [], []
    info = np.zeros(NINFO, F64)
    while p["max_iterations"] > 0:
        idx, d2 = O.nn_brute(cur, tgt)
        idx_f, d2_f, m, u = filter(idx, d2, nt, max_d2)
        _, mu, k, tau, kept = TR.threshold(d2_f, max_d2, overlap)
        assert mu == u
        if metric == PLANE:
            s, _ = PR.sums(cur[kept], tgt, nrm, idx_f[kept], np.inf, d2=d2_f[kept])
            valid = (idx_f >= 0) & (idx_f < nt)
            s[29] = d2_f[valid].astype(F64).sum()      # slot 29 runs over the sources whose idx_f is valid
        else:
            s = TR.point_sums(cur, tgt, idx_f, kept, d2_f)
        info = np.array([u, k, float(tau), s[0], m], F64)
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
        trace_Tk.append(Tk); trace_sums.append(s); trace_o2o.append(info)
        state = PR.has_converged(crit, iters, Tk, mse, p)
        if state:
            converged = True
            break
        cur = O.transform_points_f32(Tk, cur)
    _, d2 = O.nn_brute(O.transform_points_f32(fin, src), tgt)
    ncol = PR.NSUMS if metric == PLANE else 20
    return {"T": fin, "iterations": iters, "converged": converged, "state": state, "last_mse": last_mse,
            "fitness": d2.astype(F64).sum() / len(src), "trace_Tk": np.array(trace_Tk).reshape(-1, 4, 4),
            "trace_sums": np.array(trace_sums).reshape(-1, ncol), "trace_o2o": np.array(trace_o2o).reshape(-1, NINFO),
            "o2o_info": info}
