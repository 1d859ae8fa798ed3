"""Independent numpy restatement of similarity ICP (include/kssicp.h at kss_icp_sim).

Test infrastructure only; it shares no code with the library.  The selection comes from tests/trim_ref.py, the record's slots
[0..16] from its point_sums and slot [17] is a numpy sum; the solve is numpy's own SVD with Umeyama's scale and the clamp; the
criteria are p2l_ref.has_converged plus the scale condition; the exact NN, transformCloud and the Matrix4f product come from the
oracle."""
import numpy as np

import p2l_ref as PR
import trim_ref as TR

F32, F64 = np.float32, np.float64
NINFO = 6


def point_sums(cur, tgt, idx, kept, d2):
    """The KSS_NSUMS record of a similarity pass over the kept correspondences."""
    out = TR.point_sums(cur, tgt, idx, kept, d2)
    p = cur[kept].astype(F64)
    out[17] = ((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]).sum()
    return out


def sums_for(src, tgt, idx, max_d2):
    """kss_sim_sums: the untrimmed record for given correspondences (d2 recomputed in float, idx outside the target: no candidate)."""
    src, tgt = np.asarray(src, F32).reshape(-1, 3), np.asarray(tgt, F32).reshape(-1, 3)
    idx = np.asarray(idx, np.int64)
    inside = (idx >= 0) & (idx < len(tgt))
    j = np.where(inside, idx, 0)
    d2 = PR.dist2(src, tgt, j)
    with np.errstate(invalid="ignore"):
        kept = inside & (d2.astype(F64) >= 0.0) & (d2.astype(F64) <= max_d2)
    return point_sums(src, tgt, j, kept, d2)


def solve(s, lo, hi):
    """(T float32 4x4, C float32 4x4 = the step without its scale, s_k, degenerate): Umeyama with scaling by numpy's SVD."""
    s = np.asarray(s, F64)
    n = s[0]
    with np.errstate(all="ignore"):
        mu_s, mu_d = s[1:4] / n, s[4:7] / n
        var = s[17] / n - mu_s @ mu_s
        sigma = s[7:16].reshape(3, 3).T / n - np.outer(mu_d, mu_s)      # [7 + 3k + l] = sum p_k q_l; sigma_ij = E[q_i p_j] - ...
    eye = np.eye(4, dtype=F32)
    if not (var > 0.0) or not np.isfinite(sigma).all():
        return eye, eye.copy(), 1.0, True
    U, sv, Vt = np.linalg.svd(sigma)
    d = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        d[2] = -1.0
    R = U @ np.diag(d) @ Vt
    sc = (sv * d).sum() / var
    if not np.isfinite(sc) or not sc > 0.0:
        return eye, eye.copy(), 1.0, True
    sk = min(max(sc, lo), hi)
    t = mu_d - sk * (R @ mu_s)
    T, Cm = np.eye(4, dtype=F32), np.eye(4, dtype=F32)
    T[:3, :3] = (sk * R).astype(F32)
    Cm[:3, :3] = R.astype(F32)
    T[:3, 3] = t.astype(F32)
    Cm[:3, 3] = t.astype(F32)
    return T, Cm, float(sk), False


def converged(crit, iters, Cm, sk, mse, p):
    """PCL's criteria on the step without its scale; the transformation test also asks for (s_k - 1)^2 <= transformation_epsilon."""
    saved = dict(crit)
    st = PR.has_converged(crit, iters, Cm, mse, p)
    if st == 2 and not (sk - 1.0) * (sk - 1.0) <= p["transformation_epsilon"]:
        # the transformation test fails on the scale: the MSE tests that follow it, read on a step that fails it outright
        crit.clear(); crit.update(saved)
        far = Cm.copy()
        far[:3, 3] = F32(1.0) + F32(np.sqrt(abs(p["transformation_epsilon"])))
        st = PR.has_converged(crit, iters, far, mse, p)
    return st


def icp_sim(O, src, tgt, overlap=1.0, scale_min=0.5, scale_max=2.0, **kw):
    """PCL align() with the similarity step on the oracle's exact NN.  Returns the dictionary of Context.icp_sim."""
    p = dict(PR.DEFAULTS, **kw)
    src, tgt = np.asarray(src, F32), np.asarray(tgt, F32)
    max_d2 = p["max_corr_dist"] * p["max_corr_dist"]
    cur = src.copy()
    fin = np.eye(4, dtype=F32)
    crit = {"prev_mse": np.finfo(F64).max}
    iters, state, conv, last_mse = 0, 0, False, 0.0
    s_acc = 1.0
    trace_Tk, trace_sums, trace_sim = [], [], []
    info = np.zeros(NINFO, F64)
    while p["max_iterations"] > 0:
        idx, d2 = O.nn_brute(cur, tgt)
        _, m, k, tau, kept = TR.threshold(d2, max_d2, overlap)
        s = point_sums(cur, tgt, idx, kept, d2)
        info = np.array([m, k, float(tau), s[0], 0.0, s_acc], F64)
        if int(s[0]) < p["min_correspondences"]:
            state = PR.STATE_NO_CORRESPONDENCES
            break
        Tk, Cm, sk, degenerate = solve(s, scale_min / s_acc, scale_max / s_acc)
        if degenerate:
            state = PR.STATE_DEGENERATE
            break
        s_acc = min(max(s_acc * sk, scale_min), scale_max)
        info[4], info[5] = sk, s_acc
        fin = O.mat4_mul(Tk, fin)
        iters += 1
        mse = s[16] / s[0]
        last_mse = mse
        trace_Tk.append(Tk); trace_sums.append(s); trace_sim.append(info)
        state = converged(crit, iters, Cm, sk, mse, p)
        if state:
            conv = True
            break
        cur = O.transform_points_f32(Tk, cur)
    _, d2 = O.nn_brute(O.transform_points_f32(fin, src), tgt)
    return {"T": fin, "iterations": iters, "converged": conv, "state": state, "last_mse": last_mse,
            "fitness": d2.astype(F64).sum() / len(src), "trace_Tk": np.array(trace_Tk).reshape(-1, 4, 4),
            "trace_sums": np.array(trace_sums).reshape(-1, 20), "trace_sim": np.array(trace_sim).reshape(-1, NINFO),
            "sim_info": info, "scale": s_acc}


# ---- the scenes of the tests and their truth ----
def full_scene(pkg, scale):
    """make_pair(1, 3000, 8 degrees about (1, 2, 3), scale, t = (0.02, -0.01, 0.03), bumpy) and the true inverse [sR | t]."""
    R = pkg.synth.rot_axis_angle([1.0, 2.0, 3.0], np.deg2rad(8.0))
    t = np.array([0.02, -0.01, 0.03])
    src, tgt = pkg.synth.make_pair(1, 3000, R=R, scale=scale, t=t, shape="bumpy")
    A = R.T / scale
    return src, tgt, np.concatenate([A, (-A @ t)[:, None]], 1), 1.0


def partial_scene(pkg, f):
    """make_partial_pair(1, 6000, 10.0, -0.35, 0.5) with the source scaled about its centroid by f; (src, tgt, true inverse
    [sR | t], overlap to run at = 0.8 x the true overlap)."""
    src, tgt, R, t, ov = pkg.synth.make_partial_pair(1, 6000, 10.0, -0.35, 0.5)
    c = src.astype(F64).mean(0)
    src2 = (c + f * (src.astype(F64) - c)).astype(F32)
    A = R.T / f
    b = R.T @ (c - c / f - t)
    return src2, tgt, np.concatenate([A, b[:, None]], 1), 0.8 * ov
