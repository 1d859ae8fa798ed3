"""Independent numpy restatement of the 7- and 27-voxel neighbourhoods of voxelized generalized ICP (include/kssicp.h at
kss_vmap_set_neighbourhood), written from the header text on top of vgicp_ref.

Test infrastructure only.  The lattice cell of a source is an INTEGER here: f by vgicp_ref.cells, |f| <= 2^24 tested in float,
then int64; a neighbour is that cell plus an offset, and the window test is integer arithmetic on base and dims (a map without a
base has base 0).  What a correspondence adds is not restated again: terms_of() runs vgicp_ref.terms with the one function that
holds the lookup -- vgicp_ref.lookup -- replaced by the neighbour's for the length of the call (vgicp_ref is not edited), so at
setting 1 it gives vgicp_ref.terms in every bit wherever both define a voxel.  The record is the f64 sum over the
correspondences; the loop is vmap_pyramid_ref's, F started at T0."""
import contextlib

import numpy as np

import p2l_ref as P
import vgicp_ref as V

F32, F64, I64 = np.float32, np.float64, np.int64
NB_1, NB_7, NB_27 = 1, 7, 27
LIM = 1 << 24


def offsets(nb):
    """[nb, 3] int64 (o_x, o_y, o_z): the centre first, then the others in ascending (o_z, o_y, o_x)."""
    if nb not in (NB_1, NB_7, NB_27):
        raise ValueError("nb must be 1, 7 or 27")
    out = [(0, 0, 0)]
    if nb == NB_1:
        return np.array(out, I64)
    for oz in (-1, 0, 1):
        for oy in (-1, 0, 1):
            for ox in (-1, 0, 1):
                nz = (ox != 0) + (oy != 0) + (oz != 0)
                if nz == 0 or (nb == NB_7 and nz != 1):
                    continue
                out.append((ox, oy, oz))
    return np.array(out, I64)


def lattice(vm, pts):
    """(has [n] bool, a [n, 3] int64, 0 where not has): the lattice cell of every point."""
    f = V.cells(pts, vm.lo, vm.inv)
    with np.errstate(all="ignore"):
        has = (np.abs(f) <= F32(LIM)).all(1)           # compared in float: a NaN has none
    return has, np.where(has[:, None], f, F32(0)).astype(I64)


def lookup_at(vm, pts, o):
    """vgicp_ref.lookup's pair for the neighbour at offset o: (in the window and occupied [n], its row of vm.stats)."""
    has, a = lattice(vm, pts)
    base = np.asarray(getattr(vm, "base", np.zeros(3, I64)), I64)
    dims = np.asarray(vm.dims, I64)
    c = a + np.asarray(o, I64) - base
    inside = has & ((c >= 0) & (c < dims)).all(1)
    if len(vm.lin) == 0:
        return np.zeros(len(c), bool), np.zeros(len(c), I64)
    c = np.where(inside[:, None], c, 0)
    lin = (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0]
    v = np.minimum(np.searchsorted(vm.lin, lin), len(vm.lin) - 1)
    return inside & (vm.lin[v] == lin), v


@contextlib.contextmanager
def _neighbour(o):
    old = V.lookup
    V.lookup = lambda vm, pts: lookup_at(vm, pts, o)
    try:
        yield
    finally:
        V.lookup = old


def terms_of(src, sn, vm, max_d2, Rn, eps, o):
    """(kept [n], T [n, 32]) of the correspondences with the neighbour at offset o: vgicp_ref.terms on that voxel's record."""
    n = len(np.asarray(src).reshape(-1, 3))
    if len(vm.lin) == 0:
        return np.zeros(n, bool), np.zeros((n, V.NSUMS), F64)
    with _neighbour(o):
        return V.terms(src, sn, vm, max_d2, Rn, eps)


def terms(src, sn, vm, max_d2, Rn, eps, nb):
    """(kept [nb, n], T [nb, n, 32]): per neighbour in the definition's order, per source."""
    both = [terms_of(src, sn, vm, max_d2, Rn, eps, o) for o in offsets(nb)]
    return np.stack([k for k, _ in both]), np.stack([t for _, t in both])


def sums(src, sn, vm, max_d2, Rn=None, eps=1e-3, nb=NB_1):
    """(the 32-slot record, the matching sums of |term| per slot)."""
    _, T = terms(src, sn, vm, max_d2, Rn, eps, nb)
    T = T.reshape(-1, V.NSUMS)
    return T.sum(0), np.abs(T).sum(0)


def icp_vgicp(O, src, sn, vm, nb=NB_1, T0=None, eps=1e-3, fitness=True, **kw):
    """kss_icp_vgicp[_from] on a map at setting nb: vmap_pyramid_ref.icp_vgicp_from's loop over sums() above."""
    p = dict(P.DEFAULTS, **kw)
    src = np.asarray(src, F32).reshape(-1, 3)
    max_d2 = p["max_corr_dist"] * p["max_corr_dist"]
    fin = np.eye(4, dtype=F32) if T0 is None else np.asarray(T0, F32).reshape(4, 4).copy()
    cur = src.copy() if T0 is None else O.transform_points_f32(fin, src)
    crit = {"prev_mse": np.finfo(F64).max}
    iters, state, converged, last_mse = 0, 0, False, 0.0
    trace_Tk, trace_sums = [], []
    info = np.array([0.0, len(src), 0.0, len(vm.lin)], F64)
    while p["max_iterations"] > 0:
        s, _ = sums(cur, sn, vm, max_d2, Rn=fin[:3, :3], eps=eps, nb=nb)
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
        s, _ = sums(O.transform_points_f32(fin, src), sn, vm, max_d2, Rn=fin[:3, :3], eps=eps, nb=nb)
        with np.errstate(all="ignore"):
            fit = s[28] / s[0]
    return {"T": fin, "iterations": iters, "converged": converged, "state": state, "last_mse": last_mse,
            "fitness": fit, "trace_Tk": np.array(trace_Tk).reshape(-1, 4, 4),
            "trace_sums": np.array(trace_sums).reshape(-1, V.NSUMS), "info": info}
