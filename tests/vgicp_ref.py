"""Independent numpy restatement of voxelized generalized ICP (include/kssicp.h at kss_vmap and kss_icp_vgicp),
written from the header text.

Test infrastructure only.  The map: float32 numpy arithmetic for the cell of a point (a subtraction, then a multiplication, each
rounded to float; numpy never fuses), and np.bincount with f64 weights for the voxel sums -- bincount adds its weights one by one
in index order, which IS the definition's order, so the map is compared bit for bit.  The pass: every per-source term is an f64
numpy operation on the widened floats in the order the header writes down, the sums are f64 numpy sums (any order: the tests
compare them with a tolerance), the 6 x 6 solve and the criteria come from tests/p2l_ref.py, transformCloud and the Matrix4f
product from the oracle."""
import numpy as np

import p2l_ref as P
from gicp_ref import errors, halves_pair  # noqa: F401  (the scenes and the error measure are generalized ICP's)

F32, F64 = np.float32, np.float64
NSUMS = 32
MAX_CELLS = 1 << 26
STATE_NO_CORRESPONDENCES, STATE_DEGENERATE = 5, 6


class VoxelMap:
    """lo [3] f32, inv f32, dims [3] int64, lin [nvox] int64 ascending, stats [nvox, 10] f64, mapped, leaf."""

    def info(self):
        return np.array([self.mapped, len(self.lin), self.dims[0], self.dims[1], self.dims[2], self.leaf,
                         self.lo[0], self.lo[1], self.lo[2], self.inv], F64)


def cells(pts, lo, inv):
    """f [n, 3] float32 = floorf((x - lo) * inv): float subtraction, float multiplication, floor."""
    with np.errstate(all="ignore"):
        return np.floor((np.asarray(pts, F32).reshape(-1, 3) - lo) * inv)


def build(tgt, nrm, leaf):
    """The map of the definition, or None where kss_vmap_create returns KSS_ERR_ARG."""
    tgt = np.asarray(tgt, F32).reshape(-1, 3)
    nrm = np.asarray(nrm, F32).reshape(-1, 3)
    if not (np.isfinite(leaf) and leaf > 0.0) or len(tgt) == 0:
        return None
    mapped = np.isfinite(tgt).all(1) & np.isfinite(nrm).all(1)
    if not mapped.any():
        return None
    q, n = tgt[mapped], nrm[mapped]
    lo = q.min(0) + F32(0.0)                         # a zero minimum is +0
    with np.errstate(all="ignore"):
        inv = F32(1.0) / F32(leaf)
    f = cells(q, lo, inv)
    fmax = f.max(0)
    if not ((fmax >= 0) & (fmax < MAX_CELLS)).all():  # (a NaN fails)
        return None
    dims = 1 + fmax.astype(np.int64)
    if int(dims[0]) * int(dims[1]) * int(dims[2]) > MAX_CELLS:
        return None
    c = f.astype(np.int64)
    lin = (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0]
    ulin, v = np.unique(lin, return_inverse=True)
    q64, n64 = q.astype(F64), n.astype(F64)
    N = np.bincount(v).astype(F64)
    stats = np.empty((len(ulin), 10), F64)
    stats[:, 0] = N
    for a in range(3):
        stats[:, 1 + a] = np.bincount(v, weights=q64[:, a]) / N
    for k, (a, b) in enumerate([(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]):
        stats[:, 4 + k] = np.bincount(v, weights=n64[:, a] * n64[:, b]) / N
    m = VoxelMap()
    m.lo, m.inv, m.dims, m.lin, m.stats, m.mapped, m.leaf = lo, inv, dims, ulin, stats, int(mapped.sum()), float(leaf)
    return m


def lookup(vm, pts):
    """(has [n] bool, voxel [n] int64: the row of vm.stats where has)."""
    f = cells(pts, vm.lo, vm.inv)
    with np.errstate(all="ignore"):
        inside = ((f >= 0) & (f < vm.dims.astype(F32))).all(1)   # compared in float: a NaN is outside
    c = np.where(inside[:, None], f, 0).astype(np.int64)
    lin = (c[:, 2] * vm.dims[1] + c[:, 1]) * vm.dims[0] + c[:, 0]
    v = np.minimum(np.searchsorted(vm.lin, lin), len(vm.lin) - 1)
    has = inside & (vm.lin[v] == lin)
    return has, v


def metric_g(S6, m, eps):
    """(ok [n], M [n, 6]): kss_icp_gicp's C and M = adj(C) / det(C) with g(a,b) = S_ab + m[a]*m[b]."""
    e = 1.0 - eps
    idx = {(0, 0): 0, (0, 1): 1, (0, 2): 2, (1, 1): 3, (1, 2): 4, (2, 2): 5}
    with np.errstate(all="ignore"):
        def g(a, b):
            return S6[:, idx[(a, b)]] + m[:, a] * m[:, b]
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


def terms(src, sn, vm, max_d2, Rn, eps):
    """(kept [n], T [n, 32] f64): the 32 per-source terms of the record, zero rows where the source is not kept."""
    p32 = np.asarray(src, F32).reshape(-1, 3)
    ns32 = np.asarray(sn, F32).reshape(-1, 3)
    p, ns = p32.astype(F64), ns32.astype(F64)
    R = (np.eye(3, dtype=F32) if Rn is None else np.asarray(Rn, F32).reshape(3, 3)).astype(F64)
    n = len(p)
    has, v = lookup(vm, p32)
    mean, S6 = vm.stats[v, 1:4], vm.stats[v, 4:10]
    with np.errstate(all="ignore"):
        d = mean - p
        dd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        cand = has & np.isfinite(ns32).all(1) & ~(dd > max_d2)
        m = np.stack([(R[k, 0] * ns[:, 0] + R[k, 1] * ns[:, 1]) + R[k, 2] * ns[:, 2] for k in range(3)], axis=1)
        ok, M6 = metric_g(S6, m, eps)
        kept = cand & ok
        M = np.empty((n, 3, 3), F64)
        for (a, b), k in zip([(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)], range(6)):
            M[:, a, b] = M6[:, k]
            M[:, b, a] = M6[:, k]
        px, py, pz = p[:, 0], p[:, 1], p[:, 2]
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
        T[:, 28] = dd
        T[:, 30] = (d[:, 0] * u[:, 0] + d[:, 1] * u[:, 1]) + d[:, 2] * u[:, 2]
    T[~kept] = 0.0
    return kept, T


def sums(src, sn, vm, max_d2, Rn=None, eps=1e-3):
    """(the 32-slot record, the matching sums of |term| per slot)."""
    _, T = terms(src, sn, vm, max_d2, Rn, eps)
    return T.sum(0), np.abs(T).sum(0)


def icp_vgicp(O, src, sn, vm, eps=1e-3, **kw):
    """kss_icp_gicp's loop without an NN pass.  Returns the dictionary of Context.icp_vgicp."""
    p = dict(P.DEFAULTS, **kw)
    src = np.asarray(src, F32).reshape(-1, 3)
    max_d2 = p["max_corr_dist"] * p["max_corr_dist"]
    cur = src.copy()
    fin = np.eye(4, dtype=F32)
    crit = {"prev_mse": np.finfo(F64).max}
    iters, state, converged, last_mse = 0, 0, False, 0.0
    trace_Tk, trace_sums = [], []
    info = np.array([0.0, len(src), 0.0, len(vm.lin)], F64)
    while p["max_iterations"] > 0:
        s, _ = sums(cur, sn, vm, max_d2, Rn=fin[:3, :3], eps=eps)
        info[0], info[2] = s[0], s[30]
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
    s, _ = sums(O.transform_points_f32(fin, src), sn, vm, max_d2, Rn=fin[:3, :3], eps=eps)
    with np.errstate(all="ignore"):
        fitness = s[28] / s[0]
    return {"T": fin, "iterations": iters, "converged": converged, "state": state, "last_mse": last_mse,
            "fitness": fitness, "trace_Tk": np.array(trace_Tk).reshape(-1, 4, 4),
            "trace_sums": np.array(trace_sums).reshape(-1, NSUMS), "info": info}
