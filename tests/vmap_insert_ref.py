"""Independent numpy restatement of a voxel map that grows (include/kssicp.h at kss_vmap_create_box and kss_vmap_insert, DESIGN.md
2.34), written from the header text.

Test infrastructure only.  The map keeps, per voxel in ascending lin, N, s [3] and P [6] in f64 and an insert CONTINUES them: the
old sums are carried to the new numbering and np.bincount -- which adds its weights one by one in index order, the definition's
order -- is seeded with them: every voxel's first weight is its old sum (0 + s = s exactly; a sum is never -0), the new points
follow in call order.  Nothing is rebuilt from kept points: no point is kept.  The position is moved
in float32 numpy arithmetic (never fused), the normal is turned in f64 on the widened floats.  tests/vgicp_ref.py's build() is
independent of all this, and its lookup(), sums() and icp_vgicp() take a map of this class as they take one of their own."""
import numpy as np

import vgicp_ref as V

F32, F64 = np.float32, np.float64
PAIRS = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
NINSERT = 4


class GrowMap:
    """lo [3] f32, inv f32, dims [3] int64, leaf, mapped; lin [nvox] int64 ascending, N [nvox], s [nvox, 3], P [nvox, 6] f64."""

    def __init__(self, lo, inv, dims, leaf):
        self.lo, self.inv, self.dims, self.leaf = lo, inv, dims, float(leaf)
        self.mapped = 0
        self.lin = np.zeros(0, np.int64)
        self.N, self.s, self.P = np.zeros(0, F64), np.zeros((0, 3), F64), np.zeros((0, 6), F64)

    @property
    def stats(self):
        out = np.empty((len(self.lin), 10), F64)
        out[:, 0] = self.N
        out[:, 1:4] = self.s / self.N[:, None]
        out[:, 4:10] = self.P / self.N[:, None]
        return out

    def info(self):
        return np.array([self.mapped, len(self.lin), self.dims[0], self.dims[1], self.dims[2], self.leaf,
                         self.lo[0], self.lo[1], self.lo[2], self.inv], F64)

    def copy(self):
        m = GrowMap(self.lo, self.inv, self.dims, self.leaf)
        m.mapped, m.lin, m.N, m.s, m.P = self.mapped, self.lin.copy(), self.N.copy(), self.s.copy(), self.P.copy()
        return m


def _grid(lo, hi, leaf):
    """(lo with +0, inv, dims) of kss_vmap_create_box, or None where it returns KSS_ERR_ARG."""
    lo, hi = np.asarray(lo, F32).reshape(3), np.asarray(hi, F32).reshape(3)
    if not (np.isfinite(leaf) and leaf > 0.0) or not (np.isfinite(lo).all() and np.isfinite(hi).all()) or (hi < lo).any():
        return None
    lo = lo + F32(0.0)                                # a zero is +0
    with np.errstate(all="ignore"):
        inv = F32(1.0) / F32(leaf)
        f = np.floor((hi - lo) * inv)
    assert f.dtype == F32
    if not ((f >= 0) & (f < V.MAX_CELLS)).all():      # (a NaN and an infinity fail)
        return None
    dims = 1 + f.astype(np.int64)
    if int(dims[0]) * int(dims[1]) * int(dims[2]) > V.MAX_CELLS:
        return None
    return lo, inv, dims


def box(lo, hi, leaf):
    g = _grid(lo, hi, leaf)
    return None if g is None else GrowMap(g[0], g[1], g[2], leaf)


def moved(pts, nrm, T):
    """(p' [n, 3] f32, m [n, 3] f64) of the definition; T None: p' = p, m = (double)n."""
    p = np.asarray(pts, F32).reshape(-1, 3)
    n64 = np.asarray(nrm, F32).reshape(-1, 3).astype(F64)
    if T is None:
        return p, n64
    T = np.asarray(T, F32).reshape(4, 4)
    R = T[:3, :3].astype(F64)
    with np.errstate(all="ignore"):
        q = np.stack([((T[k, 0] * p[:, 0] + T[k, 1] * p[:, 1]) + T[k, 2] * p[:, 2]) + T[k, 3] for k in range(3)], axis=1)
        m = np.stack([(R[k, 0] * n64[:, 0] + R[k, 1] * n64[:, 1]) + R[k, 2] * n64[:, 2] for k in range(3)], axis=1)
    assert q.dtype == F32 and m.dtype == F64
    return q, m


def select(vm, pts, nrm, T=None):
    """(sel [n] bool: mapped and inside, mapped [n] bool, p', m, lin [n] of the selected rows)."""
    q, m = moved(pts, nrm, T)
    mapped = np.isfinite(q).all(1) & np.isfinite(np.asarray(nrm, F32).reshape(-1, 3)).all(1)
    f = V.cells(q, vm.lo, vm.inv)
    with np.errstate(all="ignore"):
        inside = ((f >= 0) & (f < vm.dims.astype(F32))).all(1)     # compared in float: the lookup's rule
    sel = mapped & inside
    c = f[sel].astype(np.int64)
    lin = (c[:, 2] * vm.dims[1] + c[:, 1]) * vm.dims[0] + c[:, 0]
    return sel, mapped, q, m, lin


def insert(vm, pts, nrm, T=None):
    """kss_vmap_insert on vm in place; returns the NINSERT doubles."""
    sel, mapped, q, m, lin = select(vm, pts, nrm, T)
    info = np.array([sel.sum(), (~mapped).sum(), (mapped & ~sel).sum(), 0], F64)
    if not sel.any():
        return info
    new_lin = np.union1d(vm.lin, lin)
    at = np.searchsorted(new_lin, vm.lin)              # the old voxels in the new numbering
    v = np.concatenate([at, np.searchsorted(new_lin, lin)])   # every old voxel's sum first, then the new points in call order

    def go_on(old, new):
        return np.bincount(v, weights=np.concatenate([old, new]), minlength=len(new_lin))

    q64, m64 = q[sel].astype(F64), m[sel]
    N = go_on(vm.N, np.ones(len(lin), F64))
    s = np.stack([go_on(vm.s[:, a], q64[:, a]) for a in range(3)], axis=1)
    P = np.stack([go_on(vm.P[:, k], m64[:, a] * m64[:, b]) for k, (a, b) in enumerate(PAIRS)], axis=1)
    info[3] = len(new_lin) - len(vm.lin)
    vm.lin, vm.N, vm.s, vm.P = new_lin, N, s, P
    vm.mapped += int(sel.sum())
    return info


def create(tgt, nrm, leaf):
    """kss_vmap_create as bounds + insert into empty (None where it returns KSS_ERR_ARG); V.build is the independent check."""
    tgt = np.asarray(tgt, F32).reshape(-1, 3)
    nrm = np.asarray(nrm, F32).reshape(-1, 3)
    mapped = np.isfinite(tgt).all(1) & np.isfinite(nrm).all(1)
    if not mapped.any():
        return None
    vm = box(tgt[mapped].min(0), tgt[mapped].max(0), leaf)
    if vm is not None:
        insert(vm, tgt, nrm)
    return vm


# ---- the sequence scene: eight partial views walking round one surface ----
AXIS = [0.3, -0.5, 1.0]
BOX_LO, BOX_HI, LEAF = [-1.6] * 3, [1.6] * 3, 0.1
NSCANS = 8


def sequence_scene(S, O, seed):
    """[(scan_k float32, its normals float32, R_k, t_k)]: M = S.bumpy(1000 + seed, 48000); scan k takes the rows whose azimuth is
    within 50 degrees of 20 k and whose index is k modulo 8 -- no point is shared -- seen from the pose R_k = 3 k degrees about AXIS,
    t_k = k * (0.02, -0.01, 0.03): scan_k = (M[sel] - t_k) @ R_k, so that R_k scan_k + t_k is the surface."""
    M = S.bumpy(1000 + seed, 48000)
    phi = np.degrees(np.arctan2(M[:, 1], M[:, 0]))
    idx = np.arange(len(M))
    out = []
    for k in range(NSCANS):
        w = (phi - 20.0 * k + 180.0) % 360.0 - 180.0
        sel = (np.abs(w) < 50.0) & (idx % 8 == k)
        R = S.rot_axis_angle(AXIS, np.deg2rad(3.0 * k))
        t = k * np.array([0.02, -0.01, 0.03])
        scan = ((M[sel] - t) @ R).astype(F32)
        out.append((scan, O.normals_pcl(scan.astype(F64), 20).astype(F32), R, t))
    return out


def start_at(O, T, scan, sn):
    """The scan and its normals at the start pose T (a float 4 x 4): the caller's to apply before kss_icp_vgicp."""
    R = np.asarray(T, F32)[:3, :3].astype(F64)
    return O.transform_points_f32(T, scan), (sn.astype(F64) @ R.T).astype(F32)


def run_sequence(O, scene, register, insert_scan, grow, max_iterations=50):
    """The scan-to-map loop.  register(k, pts, normals) -> icp_vgicp's dictionary against the map as it stands;
    insert_scan(k, scan, normals, T) adds scan k at the float pose T (None: scan 0 as it is).  grow False: only scan 0 is mapped.
    Returns [(k, result, eR, et, T)] for k = 1 ..: every scan starts from the previous scan's accumulated pose."""
    scan0, sn0, _, _ = scene[0]
    insert_scan(0, scan0, sn0, None)
    T = np.eye(4, dtype=F32)
    out = []
    for k in range(1, len(scene)):
        scan, sn, R, t = scene[k]
        p0, n0 = start_at(O, T, scan, sn)
        r = register(k, p0, n0)
        T = O.mat4_mul(r["T"], T)
        eR, et = V.errors(T, R, t)
        out.append((k, r, eR, et, T.copy()))
        if grow:
            insert_scan(k, scan, sn, T)
    return out
