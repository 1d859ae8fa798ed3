"""Independent numpy restatement of generalized ICP (include/kssicp.h at kss_icp_gicp), written from the
header text.

Test infrastructure only.  Every per-correspondence term is an f64 numpy operation on the widened floats (numpy never fuses a
multiply into an add) in the order the header writes down, the sums are f64 numpy sums (any order: the tests compare them with
a tolerance), the 6 x 6 solve and the transform come from tests/p2l_ref.py, and the exact NN, transformCloud and the Matrix4f
product come from the oracle.  metric_py is the metric of ONE correspondence in Python floats, for the bit-for-bit test of
kss_gicp_metric."""
import math

import numpy as np

import p2l_ref as P

F32, F64 = np.float32, np.float64
NSUMS = 32
STATE_NO_CORRESPONDENCES, STATE_DEGENERATE = 5, 6


def metric_py(nq, m, eps):
    """(M00, M01, M02, M11, M12, M22) in Python floats, or None when dropped."""
    nq = [float(x) for x in nq]
    m = [float(x) for x in m]
    if not all(math.isfinite(x) for x in nq + m):
        return None
    e = 1.0 - eps

    def g(a, b):
        return nq[a] * nq[b] + m[a] * m[b]

    c00 = 2.0 - e * g(0, 0)
    c01 = -(e * g(0, 1))
    c02 = -(e * g(0, 2))
    c11 = 2.0 - e * g(1, 1)
    c12 = -(e * g(1, 2))
    c22 = 2.0 - e * g(2, 2)
    a00 = c11 * c22 - c12 * c12
    a01 = c02 * c12 - c01 * c22
    a02 = c01 * c12 - c02 * c11
    a11 = c00 * c22 - c02 * c02
    a12 = c01 * c02 - c00 * c12
    a22 = c00 * c11 - c01 * c01
    det = (c00 * a00 + c01 * a01) + c02 * a02
    if not math.isfinite(det) or not det > 0.0:
        return None
    return [a00 / det, a01 / det, a02 / det, a11 / det, a12 / det, a22 / det]


def metric(nq, m, eps):
    """Vectorised: (ok [n], M [n, 6]) for f64 nq, m of shape [n, 3] (rows that are not ok hold anything)."""
    e = 1.0 - eps
    with np.errstate(all="ignore"):
        def g(a, b):
            return nq[:, a] * nq[:, b] + m[:, a] * m[:, b]
        c00 = 2.0 - e * g(0, 0)
        c01 = -(e * g(0, 1))
        c02 = -(e * g(0, 2))
        c11 = 2.0 - e * g(1, 1)
        c12 = -(e * g(1, 2))
        c22 = 2.0 - e * g(2, 2)
        a00 = c11 * c22 - c12 * c12
        a01 = c02 * c12 - c01 * c22
        a02 = c01 * c12 - c02 * c11
        a11 = c00 * c22 - c02 * c02
        a12 = c01 * c02 - c00 * c12
        a22 = c00 * c11 - c01 * c01
        det = (c00 * a00 + c01 * a01) + c02 * a02
        ok = np.isfinite(det) & (det > 0.0)
        M = np.stack([a00, a01, a02, a11, a12, a22], axis=1) / det[:, None]
    return ok, M


def terms(src, sn, tgt, tn, idx, d2, max_d2, Rn, eps):
    """(kept [n], T [n, 32] f64): the 32 per-source terms of the record (slot 29 for every source, the others where kept)."""
    idx = np.asarray(idx, np.int64)
    p = np.asarray(src, F32).reshape(-1, 3).astype(F64)
    q = np.asarray(tgt, F32).reshape(-1, 3)[idx].astype(F64)
    nq32 = np.asarray(tn, F32).reshape(-1, 3)[idx]
    ns32 = np.asarray(sn, F32).reshape(-1, 3)
    nq, ns = nq32.astype(F64), ns32.astype(F64)
    R = (np.eye(3, dtype=F32) if Rn is None else np.asarray(Rn, F32).reshape(3, 3)).astype(F64)
    d2 = np.asarray(d2, F32).astype(F64)
    n = len(p)
    with np.errstate(all="ignore"):
        m = np.stack([(R[k, 0] * ns[:, 0] + R[k, 1] * ns[:, 1]) + R[k, 2] * ns[:, 2] for k in range(3)], axis=1)
        cand = ~(d2 > max_d2) & np.isfinite(nq32).all(1) & np.isfinite(ns32).all(1)
        ok, M6 = metric(nq, m, eps)
        kept = cand & ok
        M = np.empty((n, 3, 3), F64)
        for (a, b), k in zip([(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)], range(6)):
            M[:, a, b] = M6[:, k]
            M[:, b, a] = M6[:, k]
        px, py, pz = p[:, 0], p[:, 1], p[:, 2]
        d = q - p
        u = np.stack([(M[:, a, 0] * d[:, 0] + M[:, a, 1] * d[:, 1]) + M[:, a, 2] * d[:, 2] for a in range(3)], axis=1)
        B = np.empty((n, 3, 3), F64)
        for b in range(3):
            B[:, 0, b] = py * M[:, 2, b] - pz * M[:, 1, b]
            B[:, 1, b] = pz * M[:, 0, b] - px * M[:, 2, b]
            B[:, 2, b] = px * M[:, 1, b] - py * M[:, 0, b]
        UL = np.empty((n, 3, 3), F64)
        for a in range(3):
            UL[:, a, 0] = B[:, a, 2] * py - B[:, a, 1] * pz
            UL[:, a, 1] = B[:, a, 0] * pz - B[:, a, 2] * px
            UL[:, a, 2] = B[:, a, 1] * px - B[:, a, 0] * py
        T = np.zeros((n, NSUMS), F64)
        T[:, 0] = 1.0
        cols = [UL[:, 0, 0], UL[:, 0, 1], UL[:, 0, 2], B[:, 0, 0], B[:, 0, 1], B[:, 0, 2],
                UL[:, 1, 1], UL[:, 1, 2], B[:, 1, 0], B[:, 1, 1], B[:, 1, 2],
                UL[:, 2, 2], B[:, 2, 0], B[:, 2, 1], B[:, 2, 2],
                M[:, 0, 0], M[:, 0, 1], M[:, 0, 2], M[:, 1, 1], M[:, 1, 2], M[:, 2, 2],
                py * u[:, 2] - pz * u[:, 1], pz * u[:, 0] - px * u[:, 2], px * u[:, 1] - py * u[:, 0],
                u[:, 0], u[:, 1], u[:, 2]]
        for k, c in enumerate(cols):
            T[:, 1 + k] = c
        T[:, 28] = d2
        T[:, 30] = (d[:, 0] * u[:, 0] + d[:, 1] * u[:, 1]) + d[:, 2] * u[:, 2]
    T[~kept] = 0.0
    T[:, 29] = d2
    return kept, T


def sums(src, sn, tgt, tn, idx, max_d2, Rn=None, eps=1e-3, d2=None, reverse=False):
    """(the 32-slot record, the matching sums of |term| per slot).  reverse: the terms added last source first."""
    idx = np.asarray(idx, np.int64)
    if d2 is None:
        d2 = P.dist2(src, tgt, idx)
    _, T = terms(src, sn, tgt, tn, idx, d2, max_d2, Rn, eps)
    if reverse:
        T = T[::-1]
    return T.sum(0), np.abs(T).sum(0)


def icp_gicp(O, src, sn, tgt, tn, eps=1e-3, reverse=False, **kw):
    """PCL align() with the generalized-ICP step, on the oracle's exact NN.  Returns the dictionary of Context.icp_gicp."""
    p = dict(P.DEFAULTS, **kw)
    src, tgt = np.asarray(src, F32), np.asarray(tgt, F32)
    max_d2 = p["max_corr_dist"] * p["max_corr_dist"]
    cur = src.copy()
    fin = np.eye(4, dtype=F32)
    crit = {"prev_mse": np.finfo(F64).max}
    iters, state, converged, last_mse = 0, 0, False, 0.0
    trace_Tk, trace_sums = [], []
    while p["max_iterations"] > 0:
        idx, d2 = O.nn_brute(cur, tgt)
        s, _ = sums(cur, sn, tgt, tn, idx, max_d2, Rn=fin[:3, :3], eps=eps, d2=d2, reverse=reverse)
        if int(s[0]) < p["min_correspondences"]:
            state = STATE_NO_CORRESPONDENCES
            break
        Tk, degenerate = P.rigid(s)
        if degenerate:
            state = STATE_DEGENERATE
            break
        fin = O.mat4_mul(Tk, fin)
        iters += 1
        mse = s[28] / s[0]
        last_mse = mse
        trace_Tk.append(Tk); trace_sums.append(s)
        state = P.has_converged(crit, iters, Tk, mse, p)
        if state:
            converged = True
            break
        cur = O.transform_points_f32(Tk, cur)
    _, d2 = O.nn_brute(O.transform_points_f32(fin, src), tgt)
    return {"T": fin, "iterations": iters, "converged": converged, "state": state, "last_mse": last_mse,
            "fitness": d2.astype(F64).sum() / len(src), "trace_Tk": np.array(trace_Tk).reshape(-1, 4, 4),
            "trace_sums": np.array(trace_sums).reshape(-1, NSUMS)}


def halves_pair(S, seed, n, deg, axis=None, n_src=None, t=(0.02, -0.01, 0.03)):
    """Two independent samplings of one surface: S.bumpy(seed, 2n) permuted, the first n points the target, the rest -- the first
    n_src of them -- turned by deg degrees about axis (default S.sphere(7000 + seed, 1)[0]) and moved by t the source.  No point
    of the source is a point of the target.  Returns (source, target) float32 and the true (R, t) of T: source -> target."""
    M = S.bumpy(seed, 2 * n)[S.permutation(3000 + seed, 2 * n)]
    if axis is None:
        axis = S.sphere(7000 + seed, 1)[0]
    Rt = S.rot_axis_angle(axis, np.deg2rad(deg))
    t = np.asarray(t, F64)
    src = M[n:][:n_src if n_src is not None else n] @ Rt.T + t
    return src.astype(F32), M[:n].astype(F32), Rt.T, -Rt.T @ t


def errors(T, R_true, t_true):
    return np.abs(T[:3, :3] - R_true).max(), np.abs(T[:3, 3] - t_true).max()
