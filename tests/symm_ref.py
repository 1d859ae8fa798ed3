"""Independent numpy restatement of symmetric ICP (include/kssicp.h at kss_icp_symm), written from the header
text.

Test infrastructure only.  Every per-correspondence term is an f64 numpy operation on the widened floats (numpy never fuses a
multiply into an add) in the order the header writes down, the sums are f64 numpy sums (any order: the tests compare them with
a tolerance), the 6 x 6 solve, the criteria and the defaults come from tests/p2l_ref.py, and the exact NN, transformCloud and the
Matrix4f product come from the oracle.  construct is the step in Python floats with math.sqrt, for the bit-for-bit test of
kss_rigid_from_symm_sums."""
import math

import numpy as np

import p2l_ref as P
from gicp_ref import halves_pair, errors   # noqa: F401 -- the tests' pairs and the error against the true motion, shared

F32, F64 = np.float32, np.float64
NSUMS = 32
STATE_NO_CORRESPONDENCES, STATE_DEGENERATE = 5, 6


def terms(src, sn, tgt, tn, idx, d2, max_d2, Rn, align=1):
    """(kept [n], v [n, 6], r [n], d2 [n]) in f64 for the correspondences source i -> target idx[i] (rows not kept hold anything)."""
    idx = np.asarray(idx, np.int64)
    p = np.asarray(src, F32).reshape(-1, 3).astype(F64)
    q = np.asarray(tgt, F32).reshape(-1, 3)[idx].astype(F64)
    nq32 = np.asarray(tn, F32).reshape(-1, 3)[idx]
    ns32 = np.asarray(sn, F32).reshape(-1, 3)
    nq, ns = nq32.astype(F64), ns32.astype(F64)
    R = (np.eye(3, dtype=F32) if Rn is None else np.asarray(Rn, F32).reshape(3, 3)).astype(F64)
    d2 = np.asarray(d2, F32).astype(F64)
    with np.errstate(all="ignore"):
        kept = ~(d2 > max_d2) & np.isfinite(nq32).all(1) & np.isfinite(ns32).all(1)
        m = np.stack([(R[k, 0] * ns[:, 0] + R[k, 1] * ns[:, 1]) + R[k, 2] * ns[:, 2] for k in range(3)], axis=1)
        dot = (m[:, 0] * nq[:, 0] + m[:, 1] * nq[:, 1]) + m[:, 2] * nq[:, 2]
        flip = (dot < 0.0) if align else np.zeros(len(p), bool)
        n = np.where(flip[:, None], nq - m, nq + m)
        w = p + q
        d = q - p
        c0 = w[:, 1] * n[:, 2] - w[:, 2] * n[:, 1]
        c1 = w[:, 2] * n[:, 0] - w[:, 0] * n[:, 2]
        c2 = w[:, 0] * n[:, 1] - w[:, 1] * n[:, 0]
        v = np.stack([c0, c1, c2, n[:, 0], n[:, 1], n[:, 2]], axis=1)
        r = (d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1]) + d[:, 2] * n[:, 2]
    return kept, v, r, d2


def sums(src, sn, tgt, tn, idx, max_d2, Rn=None, align=1, d2=None, reverse=False):
    """(the 32-slot record, the matching sums of |term| per slot).  reverse: the terms added last source first."""
    idx = np.asarray(idx, np.int64)
    if d2 is None:
        d2 = P.dist2(src, tgt, idx)
    kept, v, r, d2 = terms(src, sn, tgt, tn, idx, d2, max_d2, Rn, align)
    if reverse:
        kept, v, r, d2 = kept[::-1], v[::-1], r[::-1], d2[::-1]
    vk, rk = v[kept], r[kept]
    cols, absc = [float(kept.sum())], [float(kept.sum())]
    for a in range(6):
        for b in range(a, 6):
            t = vk[:, a] * vk[:, b]
            cols.append(t.sum()); absc.append(np.abs(t).sum())
    for a in range(6):
        t = vk[:, a] * rk
        cols.append(t.sum()); absc.append(np.abs(t).sum())
    tail = [d2[kept].sum(), d2.sum(), (rk * rk).sum(), 0.0]
    return np.array(cols + tail, F64), np.array(absc + tail, F64)


def construct(x):
    """The step from x = (a0, a1, a2, t0, t1, t2) in Python floats: two half rotations, rounded to float."""
    a = [float(x[0]), float(x[1]), float(x[2])]
    t = [float(x[3]), float(x[4]), float(x[5])]
    s2 = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]
    c = 1.0 / math.sqrt(1.0 + s2)
    k = (c * c) / (1.0 + c)
    K = [[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]]
    H = [[c * ((1.0 if i == j else 0.0) + K[i][j]) + k * (a[i] * a[j]) for j in range(3)] for i in range(3)]
    ct = [c * t[0], c * t[1], c * t[2]]
    T = np.zeros((4, 4), F32)
    for i in range(3):
        for j in range(3):
            T[i, j] = (H[i][0] * H[0][j] + H[i][1] * H[1][j]) + H[i][2] * H[2][j]
        T[i, 3] = (H[i][0] * ct[0] + H[i][1] * ct[1]) + H[i][2] * ct[2]
    T[3, 3] = 1.0
    return T


def half(x):
    """H, c in f64 numpy (for the orthogonality checks)."""
    a = np.asarray(x[:3], F64)
    c = 1.0 / math.sqrt(1.0 + float(a @ a))
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return c * (np.eye(3) + K) + (c * c) / (1.0 + c) * np.outer(a, a), c


def rigid(s):
    """(T, degenerate): the restatement of kss_rigid_from_symm_sums (identity when degenerate)."""
    x = P.solve(s)
    if x is None:
        return np.eye(4, dtype=F32), True
    return construct(x), False


def icp_symm(O, src, sn, tgt, tn, align=1, reverse=False, **kw):
    """PCL align() with the symmetric step, on the oracle's exact NN.  Returns the dictionary of Context.icp_symm."""
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
        s, _ = sums(cur, sn, tgt, tn, idx, max_d2, Rn=fin[:3, :3], align=align, d2=d2, reverse=reverse)
        if int(s[0]) < p["min_correspondences"]:
            state = STATE_NO_CORRESPONDENCES
            break
        Tk, degenerate = rigid(s)
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
