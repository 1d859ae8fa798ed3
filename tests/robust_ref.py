"""Independent numpy restatement of robust ICP (include/kssicp.h at kss_icp_robust).

Test infrastructure only; it shares no code with the library.  The weights, the scale from the median key (numpy.sort), the
candidate and kept masks and the weighted sums are restated here with numpy's IEEE f64 +, -, *, / and sqrt; the plane metric's
float terms, its solve and PCL's criteria come from tests/p2l_ref.py, the rank from tests/trim_ref.py; the exact NN,
rigid_from_sums, transformCloud and the Matrix4f product from the oracle."""
import numpy as np

import p2l_ref as PR
import trim_ref as TR

F32, F64 = np.float32, np.float64
NINFO = 4
POINT, PLANE = 0, 1
L2, HUBER, TUKEY, CAUCHY = 0, 1, 2, 3
LOSSES = [L2, HUBER, TUKEY, CAUCHY]
TUNE = {L2: 1.0, HUBER: 1.345, TUKEY: 4.685, CAUCHY: 2.385}


def weight(loss, x, c2):
    """w of the squared residuals x (f64 array or scalar) under `loss` with the squared scale c2."""
    x = np.asarray(x, F64)
    c2 = F64(c2)
    if loss == L2:
        return np.ones_like(x)
    if c2 == 0.0:
        return np.where(x == 0.0, 1.0, 0.0)
    with np.errstate(all="ignore"):
        u2 = x / c2
        if loss == HUBER:
            return np.where(x <= c2, 1.0, np.sqrt(c2 / x))
        if loss == TUKEY:
            return np.where(x < c2, (1.0 - u2) * (1.0 - u2), 0.0)
        return 1.0 / (1.0 + u2)


def scale2(metric, tune, med_key, min_scale):
    """c2 of the automatic form from the median key (float32; -0.0 counts as +0.0)."""
    med = F64(np.abs(F32(med_key)))
    with np.errstate(all="ignore"):
        medx = med * med if metric == PLANE else med
        K = (F64(tune) * F64(1.4826)) * (F64(tune) * F64(1.4826))
        c2 = K * medx
        floor = F64(min_scale) * F64(min_scale)
    return floor if c2 < floor else c2


def one_pass(cur, tgt, nrm, idx, d2, max_d2, loss, metric, scale=0.0, tune=None, min_scale=0.0):
    """(sums, sums of |term| per slot, info = {m, c2, sum of weights, cnt}) of one pass over the correspondences idx / d2."""
    cur, tgt = np.asarray(cur, F32).reshape(-1, 3), np.asarray(tgt, F32).reshape(-1, 3)
    idx = np.asarray(idx, np.int64)
    d2f = np.asarray(d2, F32)
    inr = (idx >= 0) & (idx < len(tgt))
    ic = np.where(inr, idx, 0)
    with np.errstate(invalid="ignore"):
        d = d2f.astype(F64)
        cand = inr & (d >= 0.0) & (d <= max_d2)
    if metric == PLANE:
        fin, v, rd, _ = PR.terms(cur, tgt, nrm, ic, d2f, np.inf)      # fin: the normal is finite (no bound on d2 here)
        cand &= fin
        x = rd * rd
        with np.errstate(invalid="ignore"):
            key = np.abs(rd.astype(F32))
    else:
        x = d
        key = d2f
    m = int(cand.sum())
    if scale > 0.0:
        c2 = F64(scale) * F64(scale)
    elif m == 0:
        c2 = F64(0.0)
    else:
        k = TR.rank(m, 0.5)
        med = np.sort(np.abs(key[cand]))[k - 1]
        c2 = scale2(metric, TUNE[loss] if tune is None else tune, med, min_scale)
    w = weight(loss, x, c2)
    with np.errstate(invalid="ignore"):
        kept = cand & np.isfinite(w) & (w > 0.0)
    wk, dk = w[kept], d[kept]
    cnt = int(kept.sum())
    if metric == PLANE:
        vk, rk = v[kept], rd[kept]
        wv = wk[:, None] * vk
        terms = [wk]
        for p in range(6):
            for q in range(p, 6):
                terms.append(wv[:, p] * vk[:, q])
        for p in range(6):
            terms.append(wv[:, p] * rk)
        terms += [wk * dk, None, (wk * rk) * rk, None]
        fixed = {29: m, 31: cnt}
    else:
        p, q = cur[kept].astype(F64), tgt[ic[kept]].astype(F64)
        ws = wk[:, None] * p
        terms = [wk] + [ws[:, k] for k in range(3)] + [wk * q[:, k] for k in range(3)]
        terms += [ws[:, k] * q[:, l] for k in range(3) for l in range(3)]
        terms += [wk * dk, None, None, None]
        fixed = {17: m, 18: 0, 19: cnt}
    s = np.array([0.0 if t is None else t.sum() for t in terms], F64)
    a = np.array([0.0 if t is None else np.abs(t).sum() for t in terms], F64)
    for slot, val in fixed.items():
        s[slot] = a[slot] = float(val)
    return s, a, np.array([m, c2, s[0], cnt], F64)


def icp_robust(O, src, tgt, nrm, loss, metric, scale=0.0, tune=None, min_scale=0.0, **kw):
    """PCL align() with the robust step on the oracle's exact NN.  Returns the dictionary of Context.icp_robust."""
    p = dict(PR.DEFAULTS, **kw)
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
        s, _, info = one_pass(cur, tgt, nrm, idx, d2, max_d2, loss, metric, scale, tune, min_scale)
        if int(info[3]) < p["min_correspondences"]:
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
        trace_Tk.append(Tk); trace_sums.append(s); trace_robust.append(info)
        state = PR.has_converged(crit, iters, Tk, mse, p)
        if state:
            converged = True
            break
        cur = O.transform_points_f32(Tk, cur)
    _, d2 = O.nn_brute(O.transform_points_f32(fin, src), tgt)
    ncol = PR.NSUMS if metric == PLANE else 20
    return {"T": fin, "iterations": iters, "converged": converged, "state": state, "last_mse": last_mse,
            "fitness": d2.astype(F64).sum() / len(src), "trace_Tk": np.array(trace_Tk).reshape(-1, 4, 4),
            "trace_sums": np.array(trace_sums).reshape(-1, ncol), "trace_robust": np.array(trace_robust).reshape(-1, NINFO),
            "robust_info": info}


# ---- the two outlier pairs of the issue, and their references computed once per session ----
PAIRS = [(2, 4000, 10.0, 0.3), (3, 3000, 5.0, 0.4)]
_CACHE = {}


def pair(pkg, O, spec):
    """(src, tgt, normals float32 by the oracle's PCL normals, R_true, t_true) with (R_true, t_true) the inverse of the
    generating transform: what a registration of the source onto the target should find."""
    key = ("pair",) + tuple(spec)
    if key not in _CACHE:
        src, tgt, R, t = pkg.synth.make_outlier_pair(*spec)
        nrm = O.normals_pcl(tgt.astype(F64), 20).astype(F32)
        _CACHE[key] = (src, tgt, nrm, R.T, -R.T @ t)
    return _CACHE[key]


def reference(pkg, O, spec, loss, metric):
    """icp_robust of the restatement on the pair, max_iterations = 200, default tuning: computed once, never modified."""
    key = ("ref",) + tuple(spec) + (loss, metric)
    if key not in _CACHE:
        src, tgt, nrm, _, _ = pair(pkg, O, spec)
        _CACHE[key] = icp_robust(O, src, tgt, nrm if metric == PLANE else None, loss, metric, max_iterations=200)
    return _CACHE[key]
