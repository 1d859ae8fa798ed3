"""Independent numpy restatement of the voxel-map pyramid (include/kssicp.h at kss_vmap_coarsen, kss_icp_vgicp_from and
kss_icp_vgicp_c2f), written from the header text.

Test infrastructure only.  coarsen() works on vmap_shift_ref's SlideMap: every voxel's lin is decoded into its local cell, the
base added, the lattice cell floor-divided by k (numpy's // rounds towards minus infinity, the definition's rule), and np.bincount
-- which adds its weights one by one in index order, here the fine voxels in their stored order, ascending fine lin -- gives N',
s' and P' from the children's kept sums: the definition's order, so a coarse map is compared bit for bit.  icp_vgicp_from() is
vgicp_ref.icp_vgicp's loop with the accumulated F started at T0 and the sources moved by T0 in float first; the pass, the solve
and the criteria are vgicp_ref's and p2l_ref's own code through vmap_shift_ref's based look-up."""
import numpy as np

import p2l_ref as P
import vgicp_ref as V
import vmap_shift_ref as Sh

F32, F64, I64 = np.float32, np.float64, np.int64
K_MIN, K_MAX, MAX_LEVELS = 2, 8, 8


def header(vm, k):
    """(leaf', inv', base', dims') of kss_vmap_coarsen(vm, k)."""
    k = int(k)
    leaf = float(k) * float(vm.leaf)
    inv = F32(1.0) / F32(leaf)
    base = Sh._base(vm) // k                           # floor division: towards minus infinity
    dims = (np.asarray(vm.dims, I64) + k - 2) // k + 1
    return leaf, inv, base.astype(I64), dims.astype(I64)


def parents(vm, k):
    """[nvox, 3] int64: the LOCAL cell C of every fine voxel's parent in the coarse window."""
    _, _, base, _ = header(vm, k)
    a = Sh.local_cells(vm) + Sh._base(vm)              # lattice cells
    return a // int(k) - base


def coarsen(vm, k):
    """kss_vmap_coarsen: a new SlideMap, or None where it returns KSS_ERR_ARG.  vm is not changed."""
    k = int(k)
    if vm is None or not K_MIN <= k <= K_MAX:
        return None
    leaf, inv, base, dims = header(vm, k)
    out = Sh.SlideMap(np.array(vm.lo, F32), inv, dims, leaf)
    out.base = base
    out.mapped = vm.mapped
    C = parents(vm, k)
    assert ((C >= 0) & (C < dims)).all()
    lin = (C[:, 2] * dims[1] + C[:, 1]) * dims[0] + C[:, 0]
    ulin, v = np.unique(lin, return_inverse=True)
    n = len(ulin)
    out.lin = ulin.astype(I64)
    out.N = np.bincount(v, weights=vm.N, minlength=n).astype(F64)
    out.s = np.stack([np.bincount(v, weights=vm.s[:, a], minlength=n) for a in range(3)], axis=1).reshape(n, 3)
    out.P = np.stack([np.bincount(v, weights=vm.P[:, a], minlength=n) for a in range(6)], axis=1).reshape(n, 6)
    return out


def same_shape(dst, vm, k):
    """kss_vmap_coarsen_into's test of dst against kss_vmap_coarsen(vm, k)'s header: lo, leaf, inv and dims bit for bit."""
    leaf, inv, _, dims = header(vm, k)
    return (np.array(dst.lo, F32).tobytes() == np.array(vm.lo, F32).tobytes() and F64(dst.leaf).tobytes() == F64(leaf).tobytes()
            and F32(dst.inv).tobytes() == F32(inv).tobytes() and (np.asarray(dst.dims, I64) == dims).all())


def coarsen_into(vm, k, dst):
    """kss_vmap_coarsen_into on dst in place: True, or False where it returns KSS_ERR_ARG (both maps untouched)."""
    if vm is None or dst is None or dst is vm or not K_MIN <= int(k) <= K_MAX or not same_shape(dst, vm, k):
        return False
    c = coarsen(vm, k)
    dst.base, dst.mapped, dst.lin, dst.N, dst.s, dst.P = c.base, c.mapped, c.lin, c.N, c.s, c.P
    return True


def icp_vgicp_from(O, src, sn, vm, T0=None, eps=1e-3, fitness=True, **kw):
    """kss_icp_vgicp_from: vgicp_ref.icp_vgicp with F started at T0.  T0 None: vmap_shift_ref.icp_vgicp itself.  Returns
    Context.icp_vgicp's dictionary, or None where T0 is refused.  fitness False: as with compute_fitness = 0."""
    if T0 is None:
        r = Sh.icp_vgicp(O, src, sn, vm, eps, **kw)
        if not fitness:
            r["fitness"] = 0.0
        return r
    T0 = np.asarray(T0, F32).reshape(4, 4)
    if not np.isfinite(T0).all():
        return None
    p = dict(P.DEFAULTS, **kw)
    src = np.asarray(src, F32).reshape(-1, 3)
    max_d2 = p["max_corr_dist"] * p["max_corr_dist"]
    fin = T0.copy()
    cur = O.transform_points_f32(T0, src)              # pass 0 works on T0 * src, the loop's float move
    crit = {"prev_mse": np.finfo(F64).max}
    iters, state, converged, last_mse = 0, 0, False, 0.0
    trace_Tk, trace_sums = [], []
    info = np.array([0.0, len(src), 0.0, len(vm.lin)], F64)
    while p["max_iterations"] > 0:
        s, _ = Sh.sums(cur, sn, vm, max_d2, Rn=fin[:3, :3], eps=eps)   # the normals: R_F on the ORIGINAL float normals, in f64
        info[0], info[2] = s[0], s[30]
        if int(s[0]) < p["min_correspondences"]:
            state = V.STATE_NO_CORRESPONDENCES
            break
        Tk, degenerate = P.rigid(s)
        if degenerate:
            state = V.STATE_DEGENERATE
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
    fit = 0.0
    if fitness:
        s, _ = Sh.sums(O.transform_points_f32(fin, src), sn, vm, max_d2, Rn=fin[:3, :3], eps=eps)
        with np.errstate(all="ignore"):
            fit = s[28] / s[0]
    return {"T": fin, "iterations": iters, "converged": converged, "state": state, "last_mse": last_mse,
            "fitness": fit, "trace_Tk": np.array(trace_Tk).reshape(-1, 4, 4),
            "trace_sums": np.array(trace_sums).reshape(-1, V.NSUMS), "info": info}


def icp_vgicp_c2f(O, src, sn, vms, T0=None, eps=1e-3, **kw):
    """kss_icp_vgicp_c2f: the chain of icp_vgicp_from calls, coarsest map first; the fitness for the last level only.  Returns the
    list of the levels' dictionaries, or None where the call is refused."""
    if not 1 <= len(vms) <= MAX_LEVELS or any(vm is None for vm in vms):
        return None
    out, A = [], T0
    for l, vm in enumerate(vms):
        r = icp_vgicp_from(O, src, sn, vm, A, eps, fitness=l == len(vms) - 1, **kw)
        if r is None:
            return None
        out.append(r)
        A = r["T"]
    return out


def ladder(vm, ks):
    """[coarsen(vm, k) for k in ks] + [vm]: the maps of a ladder such as 8, 4, 2, 1."""
    return [coarsen(vm, k) for k in ks] + [vm]
