"""Independent numpy restatement of robust symmetric ICP (include/kssicp.h at kss_icp_symm_robust), written from
the header text.

Test infrastructure only; it shares no code with the library.  v and r come from tests/symm_ref.py (terms), the weight and the
scale from tests/robust_ref.py, the rank from tests/trim_ref.py, the 6 x 6 solve, the criteria and the defaults from
tests/p2l_ref.py, the step from symm_ref.rigid, and the exact NN, transformCloud and the Matrix4f product from the oracle.  The sums
are f64 numpy sums (any order: the tests compare them with a tolerance)."""
import numpy as np

import p2l_ref as P
import robust_ref as RR
import symm_ref as S
import trim_ref as TR
from gicp_ref import halves_pair, errors   # noqa: F401 -- shared with the tests

F32, F64 = np.float32, np.float64
NSUMS, NINFO = 32, 4
L2, HUBER, TUKEY, CAUCHY = RR.L2, RR.HUBER, RR.TUKEY, RR.CAUCHY
LOSSES = RR.LOSSES
AXIS = [0.3, -0.5, 1.0]


def one_pass(cur, sn, tgt, tn, idx, d2, max_d2, loss, Rn=None, align=1, scale=0.0, tune=None, min_scale=0.0):
    """(sums, sums of |term| per slot, info = {m, c2, sum of weights, cnt}, keys) of one pass over the correspondences idx / d2."""
    cur, tgt = np.asarray(cur, F32).reshape(-1, 3), np.asarray(tgt, F32).reshape(-1, 3)
    idx = np.asarray(idx, np.int64)
    d2f = np.asarray(d2, F32)
    inr = (idx >= 0) & (idx < len(tgt))
    ic = np.where(inr, idx, 0)
    fin, v, r, d = S.terms(cur, sn, tgt, tn, ic, d2f, np.inf, Rn, align)   # fin: all six normal components finite (no bound on d2)
    with np.errstate(invalid="ignore"):
        cand = inr & (d >= 0.0) & (d <= max_d2) & fin
        x = r * r
        key = np.abs(r).astype(F32)
    key[~cand] = np.nan
    m = int(cand.sum())
    if scale > 0.0:
        c2 = F64(scale) * F64(scale)
    elif m == 0:
        c2 = F64(0.0)
    else:
        k = TR.rank(m, 0.5)
        med = np.sort(key[cand])[k - 1]
        c2 = RR.scale2(RR.PLANE, RR.TUNE[loss] if tune is None else tune, med, min_scale)
    with np.errstate(invalid="ignore"):
        w = RR.weight(loss, x, c2)
        kept = cand & np.isfinite(w) & (w > 0.0)
    wk, dk, vk, rk = w[kept], d[kept], v[kept], r[kept]
    cnt = int(kept.sum())
    wv = wk[:, None] * vk
    terms = [wk]
    for p in range(6):
        for q in range(p, 6):
            terms.append(wv[:, p] * vk[:, q])
    for p in range(6):
        terms.append(wv[:, p] * rk)
    terms += [wk * dk, None, (wk * rk) * rk, None]
    s = np.array([0.0 if t is None else t.sum() for t in terms], F64)
    a = np.array([0.0 if t is None else np.abs(t).sum() for t in terms], F64)
    s[29] = a[29] = float(m)
    s[31] = a[31] = float(cnt)
    return s, a, np.array([m, c2, s[0], cnt], F64), key


def icp_symm_robust(O, src, sn, tgt, tn, loss, align=1, scale=0.0, tune=None, min_scale=0.0, **kw):
    """PCL align() with the robust symmetric step on the oracle's exact NN.  Returns the dictionary of Context.icp_symm_robust."""
    p = dict(P.DEFAULTS, **kw)
    src, tgt = np.asarray(src, F32), np.asarray(tgt, F32)
    max_d2 = p["max_corr_dist"] * p["max_corr_dist"]
    cur = src.copy()
    fin = np.eye(4, dtype=F32)
    crit = {"prev_mse": np.finfo(F64).max}
    iters, state, converged, last_mse = 0, 0, False, 0.0
    trace_Tk, trace_sums, trace_robust = [], [], []
    info = np.zeros(NINFO, F64)
    while p["max_iterations"] > 0:
        idx, d2 = O.nn_brute(cur, tgt)
        s, _, info, _ = one_pass(cur, sn, tgt, tn, idx, d2, max_d2, loss, fin[:3, :3], align, scale, tune, min_scale)
        if int(info[3]) < p["min_correspondences"]:
            state = S.STATE_NO_CORRESPONDENCES
            break
        Tk, degenerate = S.rigid(s)
        if degenerate:
            state = S.STATE_DEGENERATE
            break
        fin = O.mat4_mul(Tk, fin)
        iters += 1
        mse = s[28] / s[0]
        last_mse = mse
        trace_Tk.append(Tk); trace_sums.append(s); trace_robust.append(info)
        state = P.has_converged(crit, iters, Tk, mse, p)
        if state:
            converged = True
            break
        cur = O.transform_points_f32(Tk, cur)
    _, d2 = O.nn_brute(O.transform_points_f32(fin, src), tgt)
    return {"T": fin, "iterations": iters, "converged": converged, "state": state, "last_mse": last_mse,
            "fitness": d2.astype(F64).sum() / len(src), "trace_Tk": np.array(trace_Tk).reshape(-1, 4, 4),
            "trace_sums": np.array(trace_sums).reshape(-1, NSUMS), "trace_robust": np.array(trace_robust).reshape(-1, NINFO),
            "robust_info": info}


# ---- the two headline scenes (65 degrees about AXIS), built from synth only ----
def outliers(synth, src, seed, share, amp=0.3):
    """src with its first k = int(share * n) points pushed off the surface, as synth.make_outlier_pair does it: (u - 0.5) * 2 * amp
    is added in f64, u[:, j] = u01(9000 + seed, k, j * k), then rounded to float."""
    out = np.asarray(src, F32).astype(F64)
    k = int(share * len(out))
    u = np.stack([synth.u01(9000 + seed, k, j * k) for j in range(3)], axis=1)
    out[:k] += (u - 0.5) * 2.0 * amp
    return out.astype(F32)


def scene_a(synth, seed=8, share=0.2):
    """halves_pair(synth, seed, 2000, 65 degrees, AXIS) with the first share of the source pushed off the surface.
    Returns (source, target, R_true, t_true)."""
    src, tgt, R_true, t_true = halves_pair(synth, seed, 2000, 65.0, axis=AXIS)
    return outliers(synth, src, seed, share), tgt, R_true, t_true


def scene_b(synth, seed=8):
    """Two partial views of one surface: M = bumpy(seed, 6000) permuted; the target is the rows of M[:3000] with x > -0.5, the
    source the rows of M[3000:] with x < 0.5, turned 65 degrees about AXIS and moved by (0.02, -0.01, 0.03).
    Returns (source, target, R_true, t_true)."""
    M = synth.bumpy(seed, 6000)[synth.permutation(3000 + seed, 6000)]
    A, B = M[:3000], M[3000:]
    tgt = A[A[:, 0] > -0.5]
    part = B[B[:, 0] < 0.5]
    Rt = synth.rot_axis_angle(AXIS, np.deg2rad(65.0))
    t = np.array([0.02, -0.01, 0.03], F64)
    src = part @ Rt.T + t
    return src.astype(F32), tgt.astype(F32), Rt.T, -Rt.T @ t


_CACHE = {}


def scene(pkg, O, name):
    """(src, tgt, sn, tn, R_true, t_true) of scene 'A' or 'B' with the library's normals definition: the oracle's PCL normals at
    k = 20 on the clouds as given, rounded to float.  Computed once per session, never modified."""
    if name not in _CACHE:
        src, tgt, R_true, t_true = (scene_a if name == "A" else scene_b)(pkg.synth)
        sn = O.normals_pcl(src.astype(F64), 20).astype(F32)
        tn = O.normals_pcl(tgt.astype(F64), 20).astype(F32)
        _CACHE[name] = (src, tgt, sn, tn, R_true, t_true)
    return _CACHE[name]
