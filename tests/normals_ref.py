"""Independent numpy reference for the surface normals (kss_normals, normals_kernel in kss_knn.hip).

Test infrastructure only; it does not import the package.  cov32 restates PCL's computeMeanAndCovarianceMatrix in float32 numpy
operations (one operation per rounding, neighbours in k-NN order) with no closed form in it; truth takes the smallest
eigenvector of that matrix from numpy.linalg.eigh in float64 and states, per point, how far PCL's closed form may be from it:

    sin(angle(n, v0)) <= C * B,    B = eps / g^2 + fb * |l0| / g,    g = l1 - l0,  eps = 2^-23

fb = 1 where pcl::computeRoots falls back to computeRoots2, which forces the smallest root to 0 (the error is |l0| itself).
A point is judged when g > 0 and B < 4e-3.  check() returns the rows of a set of normals that break one of four rules; fallback_differs() is a fifth, bit for bit against
the oracle where the normal does not depend on the trigonometric roots."""
import numpy as np

F32, F64 = np.float32, np.float64
EPS = 2.0 ** -23                      # FLT_EPSILON
FLT_MIN = 1.17549435e-38
B_MAX = 4e-3

# Twice the largest sin / B the oracle's closed form (O.normals_pcl) shows over cases(), rounded up.  Measured: 3.501, set by
# bumpy(4, 6000) at k = 64 (test_normals_host.py prints it per input and asserts C_REF <= C / 2).  The factor of two is for the
# device's atan2f, cosf and sinf, which may differ from glibc's in the last ulps: a root then moves by a few eps, the size of
# the first term of B.  Never measured against the kernel.
C = 8.0


def knn_numpy(q, t, k):
    """Exact k-NN in ascending (d2, index) order; d2 = (dx * dx + dy * dy) + dz * dz in float32."""
    q, t = np.asarray(q, F32).reshape(-1, 3), np.asarray(t, F32).reshape(-1, 3)
    idx = np.empty((len(q), k), np.int32)
    d2 = np.empty((len(q), k), F32)
    for b in range(0, len(q), 512):
        d = q[b:b + 512, None, :] - t[None, :, :]
        dd = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        o = np.argsort(dd, axis=1, kind="stable")[:, :k]
        idx[b:b + 512] = o
        d2[b:b + 512] = np.take_along_axis(dd, o, axis=1)
    return idx, d2


def cov32(P, k, knn=None):
    """(m [n, 3, 3] float32, k used): computeMeanAndCovarianceMatrix of every point's k nearest neighbours (itself included),
    k clamped to n.  knn(q, t, k) -> (idx, d2) is the exact search (default knn_numpy; the tests pass the oracle's brute force)."""
    p = np.asarray(P, F64).reshape(-1, 3).astype(F32)
    n = len(p)
    k = min(int(k), n)
    idx, _ = (knn or knn_numpy)(p, p, k)
    a = np.zeros((9, n), F32)
    for c in range(k):
        q = p[idx[:, c]]
        x, y, z = q[:, 0], q[:, 1], q[:, 2]
        a[0] = a[0] + x * x; a[1] = a[1] + x * y; a[2] = a[2] + x * z
        a[3] = a[3] + y * y; a[4] = a[4] + y * z; a[5] = a[5] + z * z
        a[6] = a[6] + x; a[7] = a[7] + y; a[8] = a[8] + z
    a = a / F32(k)
    m = np.empty((n, 3, 3), F32)
    m[:, 0, 0] = a[0] - a[6] * a[6]
    m[:, 0, 1] = m[:, 1, 0] = a[1] - a[6] * a[7]
    m[:, 0, 2] = m[:, 2, 0] = a[2] - a[6] * a[8]
    m[:, 1, 1] = a[3] - a[7] * a[7]
    m[:, 1, 2] = m[:, 2, 1] = a[4] - a[7] * a[8]
    m[:, 2, 2] = a[5] - a[8] * a[8]
    return m, k


def truth(P, k, knn=None):
    """Per point: v0 [n, 3] (eigenvector of the smallest eigenvalue of the scaled float covariance sm, float64 eigh),
    lam [n, 3] ascending, g, fb, B and the judged mask."""
    m, _ = cov32(P, k, knn)
    n = len(m)
    scale = np.abs(m).reshape(n, 9).max(axis=1)
    scale = np.where(scale <= F32(FLT_MIN), F32(1.0), scale).astype(F32)
    sm = m / scale[:, None, None]
    assert sm.dtype == F32
    m00, m01, m02, m11, m12, m22 = sm[:, 0, 0], sm[:, 0, 1], sm[:, 0, 2], sm[:, 1, 1], sm[:, 1, 2], sm[:, 2, 2]
    # pcl::computeRoots' c0, float, left to right
    c0 = m00 * m11 * m22 + F32(2.0) * m01 * m02 * m12 - m00 * m12 * m12 - m11 * m02 * m02 - m22 * m01 * m01
    lam, vec = np.linalg.eigh(sm.astype(F64))
    v0 = vec[:, :, 0]
    l0 = lam[:, 0]
    g = lam[:, 1] - l0
    fb = (np.abs(c0) < F32(EPS)) | (l0 < 16.0 * EPS)
    with np.errstate(divide="ignore", invalid="ignore"):
        B = EPS / (g * g) + np.where(fb, np.abs(l0) / g, 0.0)
    judged = (g > 0) & (B < B_MAX)
    # Rows whose normal is no function of the trigonometric roots: |c0| < eps takes computeRoots2 before any of them, and a float
    # covariance with l0 < -16 eps (cancellation made it indefinite) has a computed smallest root <= 0 whatever the last ulps
    # of atan2f, cosf and sinf (they move a root by a few eps), so computeRoots2 replaces it.  Either way the root used is
    # exactly 0 and the rest is float products, sums, one sqrtf and divisions, all correctly rounded: device and oracle agree
    # bit for bit there.  (Measured on the oracle with the second fallback taken out: of this set it changes 4147 rows of
    # bumpy + 100, 1188 of bumpy + 10 and 84 at k = 8.)
    sure = (np.abs(c0) < F32(EPS)) | (l0 < -16.0 * EPS)
    return dict(v0=v0, lam=lam, g=g, fb=fb, B=B, judged=judged, scale=scale, c0=c0, sure=sure)


def sin_to_v0(normals, tr):
    """|n x v0| per row (float64; NaN where the row is not finite)."""
    return np.linalg.norm(np.cross(np.asarray(normals, F64).reshape(-1, 3), tr["v0"]), axis=1)


def rules(P, k, normals, C, knn=None, tr=None):
    """{rule: indices of the rows that break it} for the rules (a) .. (d) of check()."""
    p = np.asarray(P, F64).reshape(-1, 3).astype(F32).astype(F64)
    nr = np.asarray(normals, F64).reshape(-1, 3)
    tr = tr if tr is not None else truth(P, k, knn)
    fin = np.isfinite(nr)
    finite, none = fin.all(axis=1), ~fin.any(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        length = np.linalg.norm(np.where(fin, nr, 0.0), axis=1)
        a = ~((finite & (np.abs(length - 1.0) < 2.0 ** -20)) | none)
        J, bound = tr["judged"], C * tr["B"]
        b = J & ~(finite & (sin_to_v0(nr, tr) <= bound))
        pn = np.linalg.norm(p, axis=1)
        c = finite & ~(-(p * nr).sum(axis=1) >= -1e-6 * pn)
        pv = (p * tr["v0"]).sum(axis=1)
        nv = (nr * tr["v0"]).sum(axis=1)
        d = J & (np.abs(pv) > 2.0 * bound * pn) & ~(nv * -pv > 0)
    return {"a": np.flatnonzero(a), "b": np.flatnonzero(b), "c": np.flatnonzero(c), "d": np.flatnonzero(d)}


def check(P, k, normals, C, knn=None, tr=None, only="abcd"):
    """Indices of the rows of `normals` that break a rule:
    (a) a row is all finite with | |n| - 1 | < 2^-20, or has no finite component;
    (b) a judged row is finite and |n x v0| <= C * B;
    (c) a finite row has -(p_f32 . n) >= -1e-6 |p| (the view-point flip is neither missing nor inverted);
    (d) a judged row's sign is that of -(p . v0) wherever |p . v0| > 2 C B |p|."""
    r = rules(P, k, normals, C, knn, tr)
    return np.unique(np.concatenate([r[x] for x in only]))


def apart(P, k, n_a, n_b, C, knn=None, tr=None):
    """Indices of the rows judged and finite in both sets whose normals are farther apart than 2 C B."""
    a, b = np.asarray(n_a, F64).reshape(-1, 3), np.asarray(n_b, F64).reshape(-1, 3)
    tr = tr if tr is not None else truth(P, k, knn)
    both = tr["judged"] & np.isfinite(a).all(axis=1) & np.isfinite(b).all(axis=1)
    with np.errstate(invalid="ignore"):
        far = np.linalg.norm(a - b, axis=1) > 2.0 * C * tr["B"]
    return np.flatnonzero(both & far)


def fallback_differs(n_a, n_b, tr):
    """Indices of the rows of truth()'s `sure` set on which two sets of normals do not have the same bits (rule (e); a NaN
    matches a NaN)."""
    a, b = np.ascontiguousarray(n_a, F64).reshape(-1, 3), np.ascontiguousarray(n_b, F64).reshape(-1, 3)
    same = ((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all(axis=1)
    return np.flatnonzero(tr["sure"] & ~same)


# ---- the inputs of tests/test_normals_host.py (oracle) and tests/test_gpu_normals.py (device) -----------------------------------
class Case:
    """name, cloud (float64), k; share: the least judged share (None: no condition); only: the rules that apply."""

    def __init__(self, name, P, k, share=None, only="abcd", group=""):
        self.name, self.P, self.k, self.share, self.only, self.group = name, np.ascontiguousarray(P, F64), k, share, only, group

    def __repr__(self):
        return self.name


K_SWEEP = (3, 4, 5, 8, 9, 16, 17, 20, 32, 33, 64)
SIZES = (4, 20, 21, 255, 256, 257, 300)
# truth()'s judged share of the inputs the 0.99 condition does not cover, as measured (it depends on the cloud alone, not on any
# normals); the tests require the share to be at least this minus 0.01
SHARE = {"k3": 0.768, "k4": 0.969, "k5": 0.996, "plus10": 0.897}


def plane(n=3000, noise=0.0):
    rng = np.random.default_rng(21)
    P = np.empty((n, 3))
    P[:, :2] = rng.uniform(-1, 1, size=(n, 2))
    P[:, 2] = 0.25
    if noise:
        P[:, 2] += noise * rng.normal(size=n)
    return P


def lattice():
    g = np.linspace(-1, 1, 40)
    xy = np.stack(np.meshgrid(g, g), -1).reshape(-1, 2)
    return np.concatenate([xy, np.ones((len(xy), 1))], axis=1)


def collinear(n=500):
    t = np.random.default_rng(22).uniform(-1, 1, size=n)
    return np.array([0.2, -0.1, 0.4]) + t[:, None] * np.array([0.6, 0.3, -0.74])


def coincident(n=30):
    return np.tile(np.array([0.3, -0.2, 0.9]), (n, 1))


def cases(S):
    """Every input, S the package's synth module.  Built once per test session by the callers."""
    out = []
    b4 = S.bumpy(4, 6000)
    for k in K_SWEEP:
        out.append(Case("bumpy4_k%d" % k, b4, k, share=0.99 if k >= 8 else SHARE["k%d" % k] - 0.01, group="k"))
    for n in SIZES:                                     # n = 4: k is clamped to 4, which the 0.99 condition does not cover
        out.append(Case("bumpy3_n%d" % n, S.bumpy(3, n), 20, share=0.99 if n >= 8 else None, group="size"))
    out.append(Case("bumpy4_plus1", b4 + 1.0, 20, share=0.99, group="pos"))
    out.append(Case("bumpy4_plus10", b4 + 10.0, 20, share=SHARE["plus10"] - 0.01, group="pos"))
    out.append(Case("bumpy4_milli", b4 * 1e-3, 20, share=0.99, group="pos"))
    out.append(Case("bumpy4_kilo", b4 * 1e3, 20, share=0.99, group="pos"))
    out.append(Case("bumpy11_aniso_plus5", S.bumpy(11, 3000) * np.array([1.0, 0.31, 2.7]) + 5.0, 20, group="pos"))
    out.append(Case("sphere8_k8", S.sphere(8, 3000), 8, share=0.99, group="pos"))
    out.append(Case("sphere8_k20", S.sphere(8, 3000), 20, share=0.99, group="pos"))
    out.append(Case("bumpy4_plus100", b4 + 100.0, 20, only="ab", group="pos"))
    out.append(Case("plane_exact", plane(), 20, share=0.99, group="fallback"))
    out.append(Case("plane_noisy", plane(noise=1e-3), 20, share=0.99, group="fallback"))
    out.append(Case("lattice", lattice(), 20, share=0.99, group="fallback"))
    out.append(Case("collinear", collinear(), 20, only="a", group="degenerate"))
    out.append(Case("coincident", coincident(), 20, only="a", group="degenerate"))
    out.append(Case("one_point", np.array([[0.5, 0.25, -1.0]]), 20, only="a", group="degenerate"))
    out.append(Case("two_points", np.array([[0.5, 0.25, -1.0], [0.1, 0.2, 0.3]]), 20, only="a", group="degenerate"))
    origin = S.bumpy(5, 1000).copy()
    origin[0] = 0.0
    out.append(Case("origin_point", origin, 20, group="degenerate"))
    assert tuple(c.name for c in out) == NAMES
    return out


NAMES = (tuple("bumpy4_k%d" % k for k in K_SWEEP) + tuple("bumpy3_n%d" % n for n in SIZES) +
         ("bumpy4_plus1", "bumpy4_plus10", "bumpy4_milli", "bumpy4_kilo", "bumpy11_aniso_plus5", "sphere8_k8", "sphere8_k20",
          "bumpy4_plus100", "plane_exact", "plane_noisy", "lattice", "collinear", "coincident", "one_point", "two_points",
          "origin_point"))
_REFERENCE = {}


def reference(S, O):
    """{name: (case, truth(case), the oracle's normals)}, computed once per process and shared by both test modules; nobody
    writes to it.  O: the oracle module (its brute-force k-NN and its copy of PCL's closed form)."""
    if not _REFERENCE:
        for c in cases(S):
            tr = truth(c.P, c.k, O.knn_brute)
            no = O.normals_pcl(c.P, min(c.k, len(c.P)))
            for a in list(tr.values()) + [no, c.P]:
                a.setflags(write=False)
            _REFERENCE[c.name] = (c, tr, no)
    return _REFERENCE
