"""Independent numpy restatement of a voxel map whose box slides over its lattice (include/kssicp.h at kss_vmap_shift and
kss_vmap_recentre), written from the header text.

Test infrastructure only.  A SlideMap is vmap_insert_ref's GrowMap with a window base: lo, inv, leaf and dims never change, a
point is inside iff (float)base <= f < (float)(base + dims) and its local cell is f - base.  shift() decodes every voxel's lin
into its local cell, keeps the voxels whose cell minus k is still in the window and subtracts delta from their lin; N, s and P of
a survivor are the same array rows, so they are the same bits.  The insert's continued sums and the whole VGICP pass are NOT
restated again: insert(), sums() and icp_vgicp() run vmap_insert_ref's and vgicp_ref's own code with the two functions that hold
the inside test -- vmap_insert_ref.select and vgicp_ref.lookup -- replaced by the based ones below for the length of the call
(neither file is edited; a map without a base is looked up as before, in every bit)."""
import contextlib

import numpy as np

import vgicp_ref as V
import vmap_insert_ref as R

F32, F64, I64 = np.float32, np.float64, np.int64
NSHIFT = 4
LIM = 1 << 24            # beyond it f is not an exact integer in float


class SlideMap(R.GrowMap):
    """GrowMap and base [3] int64, the window's first cell per axis."""

    def __init__(self, lo, inv, dims, leaf):
        super().__init__(lo, inv, dims, leaf)
        self.base = np.zeros(3, I64)

    def window(self):
        return self.base.copy()

    def copy(self):
        m = SlideMap(self.lo, self.inv, self.dims, self.leaf)
        m.mapped, m.lin, m.N, m.s, m.P = self.mapped, self.lin.copy(), self.N.copy(), self.s.copy(), self.P.copy()
        m.base = self.base.copy()
        return m


def slide(gm):
    """A GrowMap (from vmap_insert_ref.box / create) as a SlideMap with base 0; None stays None."""
    if gm is None:
        return None
    m = SlideMap(gm.lo, gm.inv, gm.dims, gm.leaf)
    m.mapped, m.lin, m.N, m.s, m.P = gm.mapped, gm.lin.copy(), gm.N.copy(), gm.s.copy(), gm.P.copy()
    return m


def box(lo, hi, leaf):
    return slide(R.box(lo, hi, leaf))


def create(tgt, nrm, leaf):
    return slide(R.create(tgt, nrm, leaf))


def _base(vm):
    return getattr(vm, "base", np.zeros(3, I64))


def inside_local(vm, f):
    """(inside [n] bool, c [n, 3] int64 local cells, 0 where outside) of float cells f: compared in float, a NaN is outside."""
    b = _base(vm)
    with np.errstate(all="ignore"):
        inside = ((f >= b.astype(F32)) & (f < (b + vm.dims).astype(F32))).all(1)
    c = np.where(inside[:, None], f, b.astype(F32)).astype(I64) - b
    return inside, c


def cells_of(vm, pts):
    """The lattice cells (int64, not window-local) of finite points: what the tests filter clouds with."""
    return V.cells(pts, vm.lo, vm.inv).astype(I64)


def select(vm, pts, nrm, T=None):
    """vmap_insert_ref.select with the based inside test and local lin."""
    q, m = R.moved(pts, nrm, T)
    mapped = np.isfinite(q).all(1) & np.isfinite(np.asarray(nrm, F32).reshape(-1, 3)).all(1)
    inside, c = inside_local(vm, V.cells(q, vm.lo, vm.inv))
    sel = mapped & inside
    c = c[sel]
    lin = (c[:, 2] * vm.dims[1] + c[:, 1]) * vm.dims[0] + c[:, 0]
    return sel, mapped, q, m, lin


def lookup(vm, pts):
    """vgicp_ref.lookup with the based inside test and local lin; a map without a voxel has none for anybody."""
    inside, c = inside_local(vm, V.cells(pts, vm.lo, vm.inv))
    if len(vm.lin) == 0:
        return np.zeros(len(c), bool), np.zeros(len(c), I64)
    lin = (c[:, 2] * vm.dims[1] + c[:, 1]) * vm.dims[0] + c[:, 0]
    v = np.minimum(np.searchsorted(vm.lin, lin), len(vm.lin) - 1)
    return inside & (vm.lin[v] == lin), v


@contextlib.contextmanager
def _based():
    old = R.select, V.lookup
    R.select, V.lookup = select, lookup
    try:
        yield
    finally:
        R.select, V.lookup = old


def insert(vm, pts, nrm, T=None):
    with _based():
        return R.insert(vm, pts, nrm, T)


def sums(src, sn, vm, max_d2, Rn=None, eps=1e-3):
    if len(vm.lin) == 0:
        return np.zeros(V.NSUMS, F64), np.zeros(V.NSUMS, F64)
    with _based():
        return V.sums(src, sn, vm, max_d2, Rn, eps)


def icp_vgicp(O, src, sn, vm, eps=1e-3, **kw):
    with _based():
        return V.icp_vgicp(O, src, sn, vm, eps, **kw)


def local_cells(vm):
    """[nvox, 3] int64: every voxel's local cell, decoded from its lin."""
    dx, dy = int(vm.dims[0]), int(vm.dims[1])
    return np.stack([vm.lin % dx, vm.lin // dx % dy, vm.lin // (dx * dy)], axis=1)


def delta_of(vm, k):
    return (int(k[2]) * int(vm.dims[1]) + int(k[1])) * int(vm.dims[0]) + int(k[0])


def shift(vm, k):
    """kss_vmap_shift on vm in place; the NSHIFT doubles, or None where it returns KSS_ERR_ARG (vm untouched)."""
    k = np.array([int(x) for x in np.asarray(k).reshape(3)], dtype=object)
    nb = [int(vm.base[a]) + k[a] for a in range(3)]
    if any(nb[a] < -LIM or nb[a] + int(vm.dims[a]) > LIM for a in range(3)):
        return None
    k = k.astype(I64)
    delta = delta_of(vm, k)
    if not k.any():
        return np.array([len(vm.lin), 0, 0, 0], F64)
    c = local_cells(vm) - k
    keep = ((c >= 0) & (c < vm.dims)).all(1)
    dropped = int(vm.N[~keep].sum())
    info = np.array([keep.sum(), (~keep).sum(), dropped, delta], F64)
    vm.lin, vm.N, vm.s, vm.P = vm.lin[keep] - delta, vm.N[keep], vm.s[keep], vm.P[keep]
    vm.mapped -= dropped
    vm.base = vm.base + k
    return info


def recentre_k(vm, centre, slack):
    """k of kss_vmap_recentre, or None where the centre or the slack is refused."""
    c = np.asarray(centre, F32).reshape(3)
    if not np.isfinite(c).all() or slack < 0:
        return None
    f = V.cells(c, vm.lo, vm.inv)[0]
    if not (np.abs(f) <= LIM).all():
        return None
    d = (f.astype(I64) - vm.dims // 2) - vm.base
    return np.where(np.abs(d) > slack, d, 0).astype(I64)


def recentre(vm, centre, slack=0):
    """(k, info), or None where kss_vmap_recentre returns KSS_ERR_ARG."""
    k = recentre_k(vm, centre, slack)
    if k is None:
        return None
    info = shift(vm, k)
    return None if info is None else (k, info)


def in_window(vm, cells, base=None):
    """[n] bool: lattice cells (int64) inside the window at `base` (default: vm's own)."""
    b = _base(vm) if base is None else np.asarray(base, I64)
    return ((cells >= b) & (cells < b + vm.dims)).all(1)


def as_seen_from(vm, other):
    """vm's voxels as (lin in `other`'s base and dims, row index into vm) for the voxels whose cell lies in other's window: the
    big-box anchor's re-expression.  Both maps share lo and inv."""
    g = local_cells(vm) + _base(vm)                   # lattice cells
    ok = in_window(other, g)
    c = g[ok] - _base(other)
    lin = (c[:, 2] * other.dims[1] + c[:, 1]) * other.dims[0] + c[:, 0]
    order = np.argsort(lin, kind="stable")
    return lin[order], np.flatnonzero(ok)[order]


# ---- the strip scene: a sensor that travels 3.15 along a strip 8 long, 64 scans ----
STRIP_SCANS, STRIP_STEP = 64, 0.05
W_LO, W_HI = [-1.6] * 3, [1.6] * 3
G_LO, G_HI = [-1.6] * 3, [6.6, 1.6, 1.6]
STRIP_LEAF, STRIP_SLACK = 0.1, 2


def strip_scene(S, O, seed, nscans=STRIP_SCANS, step=STRIP_STEP):
    """[(scan_k float32, its normals float32, R_k, t_k)] as vmap_insert_ref.sequence_scene lays it out.  The surface: 64 000 points,
    x uniform in [-1, 7), y uniform in [-0.8, 0.8) (all x drawn first), z the sum of three sines.  Scan k: the rows with
    |x - step k| < 1 whose index is k modulo 8, seen from R_k = 0.4 k degrees about AXIS and t_k = k (step, 0.002, -0.0015)."""
    rng = np.random.default_rng(2000 + seed)
    n = 64000
    x = rng.uniform(-1.0, 7.0, n)
    y = rng.uniform(-0.8, 0.8, n)
    z = 0.25 * np.sin(1.3 * x + 0.7 * seed) * np.cos(2.1 * y) + 0.15 * np.sin(2.9 * x - 1.1 * y) + 0.08 * np.sin(5.3 * y + 0.4 * x)
    M = np.stack([x, y, z], axis=1)
    idx = np.arange(n)
    out = []
    for k in range(nscans):
        sel = (np.abs(x - step * k) < 1.0) & (idx % 8 == k % 8)
        Rk = S.rot_axis_angle(R.AXIS, np.deg2rad(0.4 * k))
        t = k * np.array([step, 0.002, -0.0015])
        scan = ((M[sel] - t) @ Rk).astype(F32)
        out.append((scan, O.normals_pcl(scan.astype(F64), 20).astype(F32), Rk, t))
    return out


def run_strip(O, scene, register, insert_scan, recentre_at=None):
    """vmap_insert_ref.run_sequence with every scan inserted at its found pose; recentre_at(t) follows every insert (arm W) with
    the translation just found (zero for scan 0)."""
    def put(k, scan, sn, T):
        insert_scan(k, scan, sn, T)
        if recentre_at is not None:
            recentre_at(np.zeros(3, F32) if T is None else np.asarray(T, F32)[:3, 3])
    return R.run_sequence(O, scene, register, put, True)
