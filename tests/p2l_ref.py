"""Independent numpy restatement of point-to-plane ICP (include/kssicp.h at KSS_P2L_NSUMS).

Test infrastructure only.  The per-correspondence terms are float32 numpy operations (numpy never fuses a multiply
into an add), the sums are f64 numpy sums (any order: the tests compare them with a tolerance), and the 6x6 solve and
PCL's constructTransformationMatrix are restated with Python floats and math.sin / math.cos -- the same libm the
library calls, so the transform compares bit for bit.  The exact NN, transformCloud and the Matrix4f product come
from the oracle."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
NSUMS = 32
STATE_NO_CORRESPONDENCES, STATE_DEGENERATE = 5, 6


def terms(src, tgt, nrm, idx, d2, max_d2):
    """Per-source (kept mask, v [n, 6] f64, r f64, d2 f64) of the correspondences source i -> target idx[i]."""
    s = np.asarray(src, F32).reshape(-1, 3)
    q = np.asarray(tgt, F32).reshape(-1, 3)[idx]
    n = np.asarray(nrm, F32).reshape(-1, 3)[idx]
    sx, sy, sz = s[:, 0], s[:, 1], s[:, 2]
    qx, qy, qz = q[:, 0], q[:, 1], q[:, 2]
    nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        a = nz * sy - ny * sz
        b = nx * sz - nz * sx
        c = ny * sx - nx * sy
        r = ((nx * qx + ny * qy) + nz * qz) - nx * sx - ny * sy - nz * sz
    d2 = np.asarray(d2, F32).astype(F64)
    kept = ~(d2 > max_d2) & np.isfinite(nx) & np.isfinite(ny) & np.isfinite(nz)
    v = np.stack([a, b, c, nx, ny, nz], axis=1).astype(F64)
    return kept, v, r.astype(F64), d2


def dist2(src, tgt, idx):
    """FLANN L2_Simple in float: (dx*dx + dy*dy) + dz*dz."""
    s = np.asarray(src, F32).reshape(-1, 3)
    q = np.asarray(tgt, F32).reshape(-1, 3)[idx]
    d = s - q
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def sums(src, tgt, nrm, idx, max_d2, d2=None):
    """(the 32-slot record, the matching sums of |term| per slot)."""
    idx = np.asarray(idx, np.int64)
    if d2 is None:
        d2 = dist2(src, tgt, idx)
    kept, v, r, d2 = terms(src, tgt, nrm, idx, d2, max_d2)
    vk, rk = v[kept], r[kept]
    cols, absc = [float(kept.sum())], [float(kept.sum())]
    for p in range(6):
        for q in range(p, 6):
            t = vk[:, p] * vk[:, q]
            cols.append(t.sum()); absc.append(np.abs(t).sum())
    for p in range(6):
        t = vk[:, p] * rk
        cols.append(t.sum()); absc.append(np.abs(t).sum())
    cols += [d2[kept].sum(), d2.sum(), (rk * rk).sum(), 0.0]
    absc += [d2[kept].sum(), d2.sum(), (rk * rk).sum(), 0.0]
    return np.array(cols, F64), np.array(absc, F64)


def solve(s):
    """Cholesky of ATA in the textbook column order, forward and back substitution: x, or None when degenerate."""
    s = [float(x) for x in s]
    A = [[0.0] * 6 for _ in range(6)]
    k = 1
    for i in range(6):
        for j in range(i, 6):
            A[i][j] = A[j][i] = s[k]
            k += 1
    b = s[22:28]
    dmax = 0.0
    for i in range(6):
        if A[i][i] > dmax:
            dmax = A[i][i]
    tol = 1e-12 * dmax
    L = [[0.0] * 6 for _ in range(6)]
    for j in range(6):
        t = A[j][j]
        for k in range(j):
            t = t - L[j][k] * L[j][k]
        if not math.isfinite(t) or t <= tol:
            return None
        L[j][j] = math.sqrt(t)
        for i in range(j + 1, 6):
            t = A[i][j]
            for k in range(j):
                t = t - L[i][k] * L[j][k]
            L[i][j] = t / L[j][j]
    y = [0.0] * 6
    for i in range(6):
        t = b[i]
        for k in range(i):
            t = t - L[i][k] * y[k]
        y[i] = t / L[i][i]
    x = [0.0] * 6
    for i in range(5, -1, -1):
        t = y[i]
        for k in range(i + 1, 6):
            t = t - L[k][i] * x[k]
        x[i] = t / L[i][i]
    return x


def construct(x):
    """PCL's constructTransformationMatrix(alpha, beta, gamma, tx, ty, tz) in double, rounded to float."""
    al, be, ga, tx, ty, tz = x
    T = np.zeros((4, 4), F32)
    T[0, 0] = math.cos(ga) * math.cos(be)
    T[0, 1] = -math.sin(ga) * math.cos(al) + math.cos(ga) * math.sin(be) * math.sin(al)
    T[0, 2] = math.sin(ga) * math.sin(al) + math.cos(ga) * math.sin(be) * math.cos(al)
    T[1, 0] = math.sin(ga) * math.cos(be)
    T[1, 1] = math.cos(ga) * math.cos(al) + math.sin(ga) * math.sin(be) * math.sin(al)
    T[1, 2] = -math.cos(ga) * math.sin(al) + math.sin(ga) * math.sin(be) * math.cos(al)
    T[2, 0] = -math.sin(be)
    T[2, 1] = math.cos(be) * math.sin(al)
    T[2, 2] = math.cos(be) * math.cos(al)
    T[0, 3], T[1, 3], T[2, 3] = tx, ty, tz
    T[3, 3] = 1.0
    return T


def rigid(s):
    """(T, degenerate): the restatement of kss_rigid_from_p2l_sums (identity when degenerate)."""
    x = solve(s)
    if x is None:
        return np.eye(4, dtype=F32), True
    return construct(x), False


def has_converged(state, iters, Tk, mse, p):
    """pcl DefaultConvergenceCriteria<float>::hasConverged (kss_host_math.hpp Convergence); state = dict(prev_mse)."""
    if iters >= p["max_iterations"]:
        return 1
    if p["fixed_iterations"]:
        return 0
    tr = F32(F32(F32(Tk[0, 0] + Tk[1, 1]) + Tk[2, 2]) - F32(1.0))
    cos_angle = 0.5 * float(tr)
    tsq = F32(F32(Tk[0, 3] * Tk[0, 3]) + F32(Tk[1, 3] * Tk[1, 3]))
    tsq = F32(tsq + F32(Tk[2, 3] * Tk[2, 3]))
    if cos_angle >= 1.0 - p["transformation_epsilon"] and float(tsq) <= p["transformation_epsilon"]:
        return 2
    prev = state["prev_mse"]
    if abs(mse - prev) < p["abs_mse_epsilon"]:
        return 3
    if abs(mse - prev) / prev < p["euclidean_fitness_epsilon"]:
        return 4
    state["prev_mse"] = mse
    return 0


DEFAULTS = dict(max_iterations=1000, max_corr_dist=1.0, transformation_epsilon=1e-10, euclidean_fitness_epsilon=1e-3,
                abs_mse_epsilon=1e-12, min_correspondences=3, fixed_iterations=0)


def icp_p2l(O, src, tgt, nrm, **kw):
    """PCL align() with the point-to-plane step, on the oracle's exact NN.  Returns the dictionary of Context.icp_p2l."""
    p = dict(DEFAULTS, **kw)
    src, tgt = np.asarray(src, F32), np.asarray(tgt, F32)
    max_d2 = p["max_corr_dist"] * p["max_corr_dist"]
    cur = src.copy()
    fin = np.eye(4, dtype=F32)
    crit = {"prev_mse": np.finfo(F64).max}
    iters, state, converged, last_mse = 0, 0, False, 0.0
    trace_Tk, trace_sums = [], []
    while p["max_iterations"] > 0:
        idx, d2 = O.nn_brute(cur, tgt)
        s, _ = sums(cur, tgt, nrm, idx, max_d2, d2=d2)
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
        state = has_converged(crit, iters, Tk, mse, p)
        if state:
            converged = True
            break
        cur = O.transform_points_f32(Tk, cur)
    _, d2 = O.nn_brute(O.transform_points_f32(fin, src), tgt)
    return {"T": fin, "iterations": iters, "converged": converged, "state": state, "last_mse": last_mse,
            "fitness": d2.astype(F64).sum() / len(src), "trace_Tk": np.array(trace_Tk).reshape(-1, 4, 4),
            "trace_sums": np.array(trace_sums).reshape(-1, NSUMS)}
