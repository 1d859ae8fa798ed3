"""Independent numpy restatement of the reference's arithmetic where it narrows to float and widens back.

Test code only: nothing here imports the oracle or the package, so a mistake that the oracle and a kernel share
(both are restatements of the same reference lines) still shows up against these functions.  Every function cites
the reference lines it restates.  The reference includes <math.h> under `using namespace std`, so `sqrt` of a
`float` resolves to `float sqrt(float)`: an f32 square root, widened afterwards.

numpy float32 ufuncs round every operation to f32 and never fuse a multiply-add, which is what the reference's
float arithmetic does; cos/sin come from `math` (the C library), as in the reference.
"""
import math

import numpy as np

F32 = np.float32
F64 = np.float64


def _min_d2(q32, t32, chunk=256):
    """Squared distance from each f32 query to its nearest f32 target, d2 = (dx*dx + dy*dy) + dz*dz in f32
    (pcl::KdTreeFLANN on PointXYZ: only the smallest value is used, so any exact search gives the same one)."""
    out = np.empty(len(q32), F32)
    for a in range(0, len(q32), chunk):
        out[a:a + chunk] = _d2_block(q32[a:a + chunk], t32).min(axis=1)
    return out


def _d2_block(q32, t32):
    dx = q32[:, None, 0] - t32[None, :, 0]
    dy = q32[:, None, 1] - t32[None, :, 1]
    dz = q32[:, None, 2] - t32[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def _serial_sum(x):
    """distanceSum = distanceSum + d_i, in f64, in index order (np.add.accumulate is strictly sequential)."""
    x = np.asarray(x, F64)
    return float(np.add.accumulate(x)[-1]) if len(x) else 0.0


def error_ave(src, tgt):
    """initRegistration_Error_Ave, initRegistrationKSS.hpp:430-450.

    searchPoint.x = pointS[i][0] narrows the query to f32 (:440-442); the kd-tree holds the f32 target (:224-234);
    distance_i = sqrt(pointNKNSquaredDistance[0]) takes the f32 sqrt of an f32 d2 and widens it (:444); the distances
    are summed serially in f64 and divided by the point count (:445-448)."""
    q = np.asarray(src, F64).reshape(-1, 3).astype(F32)
    t = np.asarray(tgt, F64).reshape(-1, 3).astype(F32)
    dist = np.sqrt(_min_d2(q, t)).astype(F64)
    return _serial_sum(dist) / len(q)


def grid_angles(step):
    """for (double i = 0; i < 6.3; i = i + 6.3 / step), initRegistrationKSS.hpp:245: accumulated in f64."""
    out, a = [], 0.0
    while a < 6.3:
        out.append(a)
        a = a + 6.3 / step
    return out


def _rotate(cord, angle, p):
    """initRegistration_Transfer, initRegistrationKSS.hpp:365-404: one axis, f64, the reference's expression order."""
    c, s = math.cos(angle), math.sin(angle)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    if cord == 1:
        return np.stack([x, y * c - z * s, y * s + z * c], axis=1)
    if cord == 2:
        return np.stack([z * s + x * c, y, z * c - x * s], axis=1)
    return np.stack([x * c - y * s, x * s + y * c, z], axis=1)


def error_volume(src_preshaped, tgt, step):
    """initRegistration_Rotation, initRegistrationKSS.hpp:222-260: value[i][j][k] = Error_Ave of the source rotated
    about x by angle i, then about y by j, then about z by k (each step in f64 on the previous step's output)."""
    S = np.asarray(src_preshaped, F64).reshape(-1, 3)
    ang = grid_angles(step)
    g = len(ang)
    vol = np.empty((g, g, g), F64)
    for a, ia in enumerate(ang):
        px = _rotate(1, ia, S)
        for b, jb in enumerate(ang):
            pxy = _rotate(2, jb, px)
            for c, kc in enumerate(ang):
                vol[a, b, c] = error_ave(_rotate(3, kc, pxy), tgt)
    return vol


def octree_kn(n):
    """PCL_Octree_Resolution, Method_Octree.hpp:151-165: kn = 2 below regularPoint = 80000 points, else
    7 * (n / 80000) (integer division), capped at 35 from a multiple of 5 on."""
    if n < 80000:
        return 2
    m = n // 80000
    return 35 if m >= 5 else 7 * m


def octree_resolution(xyz):
    """PCL_Octree_Estimate_Radius + PCL_Octree_Resolution, Method_Octree.hpp:110-165.

    The cloud is narrowed to f32 PointXYZ (:119-127); each of the first 1000 points asks for its kn nearest points,
    itself included (:130-140); radius_i = sqrt(pointNKNSquaredDistance[kn - 1]) is the f32 sqrt of the f32 d2,
    widened (:141); the radii are summed serially in f64 and divided by 1000 (:142-144); `float resolution` narrows
    the mean (:150-163).  Returned as the f64 value of that float."""
    p = np.asarray(xyz, F64).reshape(-1, 3).astype(F32)
    kn = octree_kn(len(p))
    kth = np.empty(1000, F32)
    for a in range(0, 1000, 50):
        d2 = _d2_block(p[a:a + 50], p)
        kth[a:a + 50] = np.partition(d2, kn - 1, axis=1)[:, kn - 1]
    radius = np.sqrt(kth).astype(F64)
    return float(F32(_serial_sum(radius) / 1000))


def _f32_ulps_around_one(k):
    up, down = [F32(1.0)], []
    for _ in range(k):
        up.append(np.nextafter(up[-1], F32(2.0)))
        down.append(np.nextafter(down[-1] if down else F32(1.0), F32(0.0)))
    return np.array(down[::-1] + up, F32)


def check_renormalised(normals, ulps=32):
    """normalCompute.hpp:342-348 (and :387-392): dis_i = sqrt(nx*nx + ny*ny + nz*nz) over the float fields of
    pcl::Normal, so the products and sums are f32, the sqrt is f32, and only then normal_x / dis_i divides in f64.

    A property check, independent of the eigen-solver that produced the float normal v: n passes iff for some f32 s
    within `ulps` ulps of 1, v = fl32(n * s) satisfies sqrtf(fl32((vx*vx + vy*vy) + vz*vz)) == s and v / s == n in f64
    bit for bit.  Returns the rows of `normals` that fail."""
    n = np.asarray(normals, F64).reshape(-1, 3)
    s32 = _f32_ulps_around_one(ulps)
    v = (n[:, None, :] * s32.astype(F64)[None, :, None]).astype(F32)
    back = np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
    exact = (v.astype(F64) / s32.astype(F64)[None, :, None] == n[:, None, :]).all(axis=-1)
    ok = ((back == s32[None, :]) & exact).any(axis=1)
    return n[~ok]


# ---- constructed cases: inputs on which the f32 and the f64 reading of those sqrt calls give different answers ----
def origin_case(seed, min_ulp=0.4):
    """A target point (x, y, 0) whose f32 squared distance d2 from the origin has sqrt((double)d2) and
    (double)sqrtf(d2) at least `min_ulp` f32 ulps apart."""
    rng = np.random.default_rng(seed)
    for _ in range(1000):
        x, y = rng.uniform(0.2, 1.5, size=2).astype(F32)
        d2 = (x * x + y * y) + F32(0) * F32(0)
        f = F64(np.sqrt(d2))
        wide = np.sqrt(F64(d2))
        if abs(wide - f) >= min_ulp * float(np.spacing(np.sqrt(d2))):
            return x, y, d2
    raise AssertionError("no origin case found")


def paired_octree_cloud(seed, n_far=600):
    """First 1000 points: 500 isolated pairs on an integer lattice, half of them offset by (a1, b1, 0), half by
    (a2, b2, 0), with a, b multiples of 2^-20 (so the offsets are exact in f32 and every pair has the same f32 d2);
    then `n_far` points well away.  The offsets are searched so that the mean of widened sqrtf(d2) and the mean of
    sqrt((double)d2) narrow to different floats."""
    rng = np.random.default_rng(seed)
    lat = np.stack(np.meshgrid(np.arange(10), np.arange(10), np.arange(5), indexing="ij"), -1).reshape(-1, 3)
    far = rng.uniform(0.0, 6.0, size=(n_far, 3)) + np.array([30.0, 0.0, 0.0])
    for _ in range(400):
        off = np.zeros((2, 3))
        off[:, :2] = rng.integers(10000, 30000, size=(2, 2)) * 2.0 ** -20
        P = np.empty((1000, 3))
        P[0::2] = lat
        P[1::2] = lat + off[np.arange(500) % 2]
        o32 = off.astype(F32)
        d2 = (o32[:, 0] * o32[:, 0] + o32[:, 1] * o32[:, 1]) + o32[:, 2] * o32[:, 2]
        per = np.tile(np.repeat(d2, 2), 250)                           # the nearest other point of each of the 1000
        new = F32(np.add.accumulate(np.sqrt(per).astype(F64))[-1] / 1000)
        old = F32(np.add.accumulate(np.sqrt(per.astype(F64)))[-1] / 1000)
        if new != old:
            return np.concatenate([P, far]), float(new), float(old)
    raise AssertionError("no pair of offsets found")
