"""Independent numpy restatement of reciprocal ICP (include/kssicp.h at kss_icp_recip).

Test infrastructure only; it shares no code with the library.  Two forms of the filter:
  filter_nn      on the oracle's exact NN map: mutual = candidate AND rev[idx[i]] == i with rev, rd2 = nn_brute(targets, sources)
                 (exact, ties to the lowest index).  It asserts bits(d2[i]) == bits(rd2[idx[i]]) on every mutual row: dist2 without fma
                 is symmetric in its operands bit for bit, which is what makes this form equal to the definition.
  filter_direct  for ANY d2: the existence statement itself -- a winner (tests/o2o_ref.py's) is mutual iff no source k has
                 rkey(k, j) < key(i) -- evaluated in float32 numpy arithmetic over all sources, in chunks of winners.
The loop is tests/o2o_ref.py's loop with filter_nn in front of the selection."""
import numpy as np

import o2o_ref as OR
import p2l_ref as PR
import trim_ref as TR

F32, F64 = np.float32, np.float64
NINFO = 6
POINT, PLANE = TR.POINT, TR.PLANE
QNAN = np.uint32(0x7FC00000)
MASK = np.uint32(0x7FFFFFFF)


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _finish(idx, d2, cand, mutual):
    idx_f, d2_f = idx.copy(), d2.copy()
    lose = cand & ~mutual
    idx_f[lose] = -1
    d2_f.view(np.uint32)[lose] = QNAN
    return idx_f, d2_f


def dist2(p, q):
    """The NN engines' float32 squared distance without fma, (dx*dx + dy*dy) + dz*dz, of the rows of p to the rows of q (broadcast),
    source first.  Every numpy float32 operation is one IEEE single operation."""
    d = p.astype(F32) - q.astype(F32)
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def filter_nn(O, cur, tgt, idx, d2, max_d2):
    """(idx_f, d2_f, m, u, r) on an exact NN map idx / d2 = nn_brute(cur, tgt)."""
    cur, tgt = np.asarray(cur, F32), np.asarray(tgt, F32)
    idx = np.asarray(idx, np.int32).reshape(-1)
    d2 = np.asarray(d2, F32).reshape(-1)
    nt = len(tgt)
    cand = OR.candidates(idx, d2, nt, max_d2)
    _, _, m, u = OR.filter(idx, d2, nt, max_d2)
    rev, rd2 = O.nn_brute(tgt, cur)
    j = np.clip(idx, 0, nt - 1)
    mutual = cand & (rev[j] == np.arange(len(idx)))
    assert np.array_equal(_bits(d2[mutual]), _bits(rd2[j[mutual]]))
    idx_f, d2_f = _finish(idx, d2, cand, mutual)
    return idx_f, d2_f, m, u, int(mutual.sum())


def filter_direct(cur, tgt, idx, d2, max_d2, chunk=128):
    """(idx_f, d2_f, m, u, r) for any idx / d2: the existence statement over all sources."""
    cur, tgt = np.asarray(cur, F32), np.asarray(tgt, F32)
    idx = np.asarray(idx, np.int32).reshape(-1)
    d2 = np.asarray(d2, F32).reshape(-1)
    n, nt = len(idx), len(tgt)
    cand = OR.candidates(idx, d2, nt, max_d2)
    o_idx, _, m, u = OR.filter(idx, d2, nt, max_d2)
    win = np.nonzero(cand & (o_idx >= 0))[0]
    key = ((_bits(d2) & MASK).astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    k_all = np.arange(n, dtype=np.uint64)[None, :]
    mutual = np.zeros(n, bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(0, len(win), chunk):
            w = win[b:b + chunk]
            d = dist2(cur[None, :, :], tgt[idx[w]][:, None, :])                       # [winners, sources]
            rkey = ((_bits(d).reshape(d.shape) & MASK).astype(np.uint64) << np.uint64(32)) | k_all
            mutual[w] = ~(rkey < key[w][:, None]).any(1)
    idx_f, d2_f = _finish(idx, d2, cand, mutual)
    return idx_f, d2_f, m, u, int(mutual.sum())


def icp_recip(O, src, tgt, nrm, overlap, metric, **kw):
    """PCL align() with the reciprocal trimmed step on the oracle's exact NN.  Returns the dictionary of Context.icp_recip."""
    p = dict(PR.DEFAULTS, **kw)
    src, tgt = np.asarray(src, F32), np.asarray(tgt, F32)
    nt = len(tgt)
    max_d2 = p["max_corr_dist"] * p["max_corr_dist"]
    cur = src.copy()
    fin = np.eye(4, dtype=F32)
    crit = {"prev_mse": np.finfo(F64).max}
    iters, state, converged, last_mse = 0, 0, False, 0.0
    trace_Tk, trace_sums, trace_recip = [], [], []
    info = np.zeros(NINFO, F64)
    while p["max_iterations"] > 0:
        idx, d2 = O.nn_brute(cur, tgt)
        idx_f, d2_f, m, u, r = filter_nn(O, cur, tgt, idx, d2, max_d2)
        _, mr, k, tau, kept = TR.threshold(d2_f, max_d2, overlap)
        assert mr == r
        if metric == PLANE:
            s, _ = PR.sums(cur[kept], tgt, nrm, idx_f[kept], np.inf, d2=d2_f[kept])
            valid = (idx_f >= 0) & (idx_f < nt)
            s[29] = d2_f[valid].astype(F64).sum()      # slot 29 runs over the sources whose idx_f is valid
        else:
            s = TR.point_sums(cur, tgt, idx_f, kept, d2_f)
        info = np.array([r, k, float(tau), s[0], m, u], F64)
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
        trace_Tk.append(Tk); trace_sums.append(s); trace_recip.append(info)
        state = PR.has_converged(crit, iters, Tk, mse, p)
        if state:
            converged = True
            break
        cur = O.transform_points_f32(Tk, cur)
    _, d2 = O.nn_brute(O.transform_points_f32(fin, src), tgt)
    ncol = PR.NSUMS if metric == PLANE else 20
    return {"T": fin, "iterations": iters, "converged": converged, "state": state, "last_mse": last_mse,
            "fitness": d2.astype(F64).sum() / len(src), "trace_Tk": np.array(trace_Tk).reshape(-1, 4, 4),
            "trace_sums": np.array(trace_sums).reshape(-1, ncol), "trace_recip": np.array(trace_recip).reshape(-1, NINFO),
            "recip_info": info}
