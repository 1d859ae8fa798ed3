"""A voxel map whose box slides, the parts that need no GPU: the exported symbols and binding methods, the
restatement in tests/vmap_shift_ref.py on the consequences the header states -- against tests/vmap_insert_ref.py maps, which
know nothing of a base, as the big box G --, kss_vmap_recentre's arithmetic, the refusals, and the strip sequence on the
restatement alone: the check that the GPU test's scene is fair, and the source of its error bar.

The strip sequence, measured with the restatement (max over scans 1..63 of max|R - R_k|, max|t - t_k|):
    seed 3   W 2.888e-03  5.549e-03    G 2.888e-03  5.549e-03
    seed 8   W 2.190e-03  3.595e-03    G 2.190e-03  3.595e-03
W and G agree in every digit: a scan only ever reads voxels inside the window, and the window drops none of those.  Arm F, the
fixed small box, does NOT end in KSS_STATE_NO_CORRESPONDENCES in the chained loop, whatever k: a scan is a cloud around the
sensor, and from the previous pose -- which F stops advancing -- it lands inside the box again and "converges" on a wrong pose
(errors up to 0.25 in R and 0.64 in t).  What the geometry does give is checked instead: see test_strip_sequence."""
import os
import re

import numpy as np
import pytest

import vgicp_ref as V
import vmap_insert_ref as R
import vmap_shift_ref as H
from conftest import ROOT

F32, F64, I64 = np.float32, np.float64, np.int64
NAMES = ["kss_vmap_window", "kss_vmap_shift", "kss_vmap_recentre"]
STRIP_CPU = {3: (2.888e-03, 5.549e-03), 8: (2.190e-03, 3.595e-03)}   # the figures above


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)


def _snapshot(m):
    return m.lin.copy(), m.stats.copy(), m.s.copy(), m.P.copy(), m.info().copy(), m.window()


def _same_snapshot(a, b):
    for x, y in zip(a, b):
        assert np.array_equal(_bits(x), _bits(y))


def test_symbols_exported_listed_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "kssicp.h")).read()
    declared = set(re.findall(r"\b(kss_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    exported = set(pkg.exported_symbols())
    for n in NAMES:
        assert n in declared and n in pkg.binding.SYMBOLS and n in exported, n
    L = pkg.load_library()
    assert len(L.kss_vmap_window.argtypes) == 2 and len(L.kss_vmap_shift.argtypes) == 4 and len(L.kss_vmap_recentre.argtypes) == 6
    for n in ("shift", "recentre", "window"):
        assert callable(getattr(pkg.VoxelMap, n)), n
    assert pkg.VMAP_NSHIFT == pkg.binding.VMAP_NSHIFT == 4 == H.NSHIFT
    assert re.search(r"#define\s+KSS_VMAP_NSHIFT\s+4\b", hdr)
    # a null context or map is refused before anything touches a device
    k = np.zeros(3, I64)
    assert L.kss_vmap_window(None, k.ctypes.data) == -1
    assert L.kss_vmap_shift(None, None, k.ctypes.data, None) == -1
    assert L.kss_vmap_recentre(None, None, None, 0, None, None) == -1


@pytest.fixture(scope="module")
def cloud(pkg):
    n = 5000
    return pkg.synth.bumpy(11, n).astype(F32), _unit(np.random.default_rng(11), n)


def _survive(m0, ks):
    """The voxels of m0 that are inside every window of the walk ks, from the definition: keep [nvox] bool."""
    c = H.local_cells(m0)
    keep = np.ones(len(c), bool)
    for k in np.cumsum(np.asarray(ks, I64).reshape(-1, 3), axis=0):
        keep &= ((c - k >= 0) & (c - k < m0.dims)).all(1)
    return keep


@pytest.mark.parametrize("k", [(1, 0, 0), (0, -1, 0), (0, 0, 1), (8, -5, 3), (-15, 2, 0), (0, 0, -16)])
def test_consequence_1_shift_and_back(cloud, k):
    A, an = cloud
    m = H.create(A, an, 0.1)
    m0 = m.copy()
    before = _snapshot(m)
    assert np.array_equal(H.shift(m, (0, 0, 0)), [len(m0.lin), 0, 0, 0])
    _same_snapshot(before, _snapshot(m))
    keep = _survive(m0, [k])
    info = H.shift(m, k)
    delta = (k[2] * int(m.dims[1]) + k[1]) * int(m.dims[0]) + k[0]
    assert np.array_equal(info, [keep.sum(), (~keep).sum(), m0.N[~keep].sum(), delta])
    assert 0 < keep.sum() < len(keep)
    assert np.array_equal(m.lin, m0.lin[keep] - delta) and (np.diff(m.lin) > 0).all()
    assert np.array_equal(m.window(), k) and m.mapped == m0.N[keep].sum()
    back = H.shift(m, [-x for x in k])
    assert np.array_equal(back, [keep.sum(), 0, 0, -delta])
    assert np.array_equal(m.lin, m0.lin[keep]) and np.array_equal(m.window(), [0, 0, 0])
    assert np.array_equal(_bits(m.stats), _bits(m0.stats[keep]))
    assert np.array_equal(_bits(m.s), _bits(m0.s[keep])) and np.array_equal(_bits(m.P), _bits(m0.P[keep]))
    assert np.array_equal(m.info()[[2, 3, 4, 5, 6, 7, 8, 9]], m0.info()[[2, 3, 4, 5, 6, 7, 8, 9]])


@pytest.mark.parametrize("k1,k2", [((3, 0, 0), (0, 4, 0)), ((5, -2, 1), (-9, 2, 3)), ((-4, -4, -4), (4, 4, 4)), ((20, 0, 0), (20, 0, 0))])
def test_consequence_2_two_shifts(cloud, k1, k2):
    A, an = cloud
    m = H.create(A, an, 0.1)
    m0 = m.copy()
    keep = _survive(m0, [k1, k2])
    H.shift(m, k1)
    H.shift(m, k2)
    d = H.delta_of(m0, k1) + H.delta_of(m0, k2)
    assert np.array_equal(m.lin, m0.lin[keep] - d)
    assert np.array_equal(_bits(m.stats), _bits(m0.stats[keep]))
    assert np.array_equal(m.window(), np.add(k1, k2)) and m.mapped == m0.N[keep].sum()
    if k1 == (20, 0, 0):
        assert len(m.lin) == 0 and m.mapped == 0                     # 40 >= dims_x: everything has left


def test_consequence_3_big_box_anchor(pkg):
    """W slides by (3, 0, 0) and (0, 4, 0) with inserts between; G is vmap_insert_ref's own box map -- no base anywhere in its
    code -- over the same lo with a hi that contains every window.  Both get the same clouds, filtered on the CPU to W's window
    at the time, so W counts nothing as outside.  The walk is monotone, so no cell of the final window was ever dropped."""
    leaf = 0.1
    W = H.box(H.W_LO, H.W_HI, leaf)
    G = R.box(H.W_LO, [2.6, 2.6, 1.6], leaf)
    assert np.array_equal(_bits(W.lo), _bits(G.lo)) and W.inv == G.inv and list(W.dims) == [33, 33, 33] and list(G.dims) == [43, 43, 33]
    rng = np.random.default_rng(21)
    total = 0
    for step, (k, off) in enumerate([((0, 0, 0), (0, 0, 0)), ((3, 0, 0), (0.3, 0.05, 0)), ((0, 4, 0), (0.35, 0.4, 0.02))]):
        assert H.shift(W, k) is not None
        P = (pkg.synth.bumpy(30 + step, 3000) * 1.4 + np.array(off)).astype(F32)
        nr = _unit(rng, len(P))
        ok = H.in_window(W, H.cells_of(W, P))
        assert 0.5 * len(P) < ok.sum() < len(P)                      # the filter bites, and leaves a cloud
        iw = H.insert(W, P[ok], nr[ok])
        ig = R.insert(G, P[ok], nr[ok])
        assert iw[2] == 0 and ig[2] == 0 and iw[0] == ig[0] == ok.sum()
        total += int(ok.sum())
    assert np.array_equal(W.window(), [3, 4, 0]) and 0 < W.mapped < total == G.mapped
    lin, rows = H.as_seen_from(G, W)
    assert np.array_equal(lin, W.lin) and 0 < len(rows) < len(G.lin)
    assert np.array_equal(_bits(G.stats[rows]), _bits(W.stats))
    # and the other way round: W's voxels at G's lin
    lin_g, rows_w = H.as_seen_from(W, G)
    assert np.array_equal(lin_g, G.lin[rows]) and np.array_equal(rows_w, np.arange(len(W.lin)))


def test_consequence_4_sums_against_the_big_box(pkg):
    """The restatement's own pass against W and against G, for sources inside W's final window: the same voxels, so the same bits."""
    W = H.box(H.W_LO, H.W_HI, 0.1)
    G = R.box(H.W_LO, [2.6, 2.6, 1.6], 0.1)
    rng = np.random.default_rng(22)
    A, an = (pkg.synth.bumpy(40, 3000) * 1.2).astype(F32), _unit(rng, 3000)
    ok = H.in_window(W, H.cells_of(W, A), base=[3, 0, 0]) & H.in_window(W, H.cells_of(W, A))
    H.insert(W, A[ok], an[ok])
    R.insert(G, A[ok], an[ok])
    assert H.shift(W, (3, 0, 0))[1] == 0                             # every voxel lies in both windows: none dropped
    src = (A[ok][::3] + F32(0.01)).astype(F32)
    sn = _unit(rng, len(src))
    inside = H.in_window(W, H.cells_of(W, src))
    src, sn = src[inside], sn[inside]
    a, _ = H.sums(src, sn, W, 0.01)
    b, _ = V.sums(src, sn, G, 0.01)
    assert a[0] > 100 and np.array_equal(_bits(a), _bits(b))


def test_recentre_arithmetic():
    """lo = 0, leaf 0.25 (inv = 4 exactly), hi = 8: dims 33, dims / 2 = 16.  want = (int64)f - 16."""
    m = H.box([0, 0, 0], [8, 8, 8], 0.25)
    assert list(m.dims) == [33, 33, 33] and m.inv == 4.0
    # the middle cell: nothing to do; a centre exactly on the boundary between cells 16 and 17 is in cell 17
    assert np.array_equal(H.recentre_k(m, [4.0, 4.1, 4.24], 0), [0, 0, 0])
    assert np.array_equal(H.recentre_k(m, [4.25, np.nextafter(F32(4.25), F32(0)), 4.5], 0), [1, 0, 2])
    assert np.array_equal(H.recentre_k(m, [4.25, 4.5, 4.75], 2), [0, 0, 3])     # |d| > slack, not >=
    assert np.array_equal(H.recentre_k(m, [3.99, 3.5, 3.25], 2), [0, 0, -3])
    # below lo: f = floorf(-0.4) = -1, not 0
    assert np.array_equal(H.recentre_k(m, [-0.1, -0.25, -0.26], 0), [-17, -17, -18])
    assert np.array_equal(H.recentre_k(m, [-0.1, 4.0, 4.0], 2), [-17, 0, 0])
    k, info = H.recentre(m, [-0.1, 4.0, 4.6], 0)
    assert np.array_equal(k, [-17, 0, 2]) and np.array_equal(m.window(), [-17, 0, 2]) and np.array_equal(info, [0, 0, 0, 2 * 33 * 33 - 17])
    # from the new base the same centre asks for nothing, and the old middle asks for the way back
    assert np.array_equal(H.recentre_k(m, [-0.1, 4.0, 4.6], 0), [0, 0, 0])
    assert np.array_equal(H.recentre_k(m, [4.0, 4.0, 4.0], 0), [17, 0, -2])
    assert np.array_equal(H.recentre_k(m, [4.0, 4.0, 4.0], 2), [17, 0, 0])


def test_refusals(cloud):
    A, an = cloud
    m = H.create(A, an, 0.1)
    dims = [int(d) for d in m.dims]
    before = _snapshot(m)
    lim = 1 << 24
    for k in ((-lim - 1, 0, 0), (0, lim - dims[1] + 1, 0), (0, 0, 1 << 40), (0, 0, -(1 << 62)), ((1 << 63) - 1, 0, 0)):
        assert H.shift(m, k) is None
    for centre, slack in (([np.nan, 0, 0], 0), ([0, np.inf, 0], 0), ([0, 0, -np.inf], 0), ([0, 0, 0], -1), ([3e6, 0, 0], 0), ([0, -3e6, 0], 0)):
        assert H.recentre(m, centre, slack) is None                  # 3e6 * 10 cells is beyond 2^24
    _same_snapshot(before, _snapshot(m))
    # the edges themselves are taken: the window at the last cells of the lattice, empty
    assert H.shift(m, (-lim, lim - dims[1], 0))[0] == 0 and np.array_equal(m.window(), [-lim, lim - dims[1], 0])
    assert H.shift(m, (-1, 0, 0)) is None and H.shift(m, (0, 1, 0)) is None
    assert H.shift(m, (1, -1, 0)) is not None


# ---- the strip sequence ----
@pytest.fixture(scope="module")
def strips(pkg, O):
    return {seed: H.strip_scene(pkg.synth, O, seed) for seed in (3, 8)}


def restated_strip(O, scene, lo, hi, slack=None):
    vm = H.box(lo, hi, H.STRIP_LEAF)
    outside = [0.0]

    def put(k, scan, sn, T):
        outside[0] += H.insert(vm, scan, sn, T)[2]
    out = H.run_strip(O, scene, lambda k, p, n: H.icp_vgicp(O, p, n, vm, max_iterations=50), put,
                      None if slack is None else lambda t: H.recentre(vm, t, slack))
    return vm, out, outside[0]


@pytest.mark.parametrize("seed", [3, 8])
def test_strip_sequence(O, strips, seed):
    """The three arms on the restatement; the figures are in the module's docstring and DESIGN.md 2.35.
    W and G: every scan converges, under the figures measured.  W's table has F's cells, not G's.
    F: the issue expected KSS_STATE_NO_CORRESPONDENCES for every scan with 0.05 k - 1 > 1.6, "a condition of the geometry".  It is
    not one (the module's docstring): the condition on the estimated pose fails in the restatement's own loop.  What IS geometry:
    the box's last cell ends at lo + 33 * 0.1 = 1.7, so from k = 54 on (0.05 k - 1 >= 1.7) no point of scan k AT ITS TRUE POSE is
    inside F -- a registration started there finds nothing -- and hence whatever F's chained loop reports for such a scan is
    either KSS_STATE_NO_CORRESPONDENCES or a pose that is wrong by more than W's whole error, while W stays right."""
    scene = strips[seed]
    sizes = [len(s[0]) for s in scene]
    assert len(scene) == 64 and 1800 < min(sizes) and max(sizes) < 2200
    W, w, w_out = restated_strip(O, scene, H.W_LO, H.W_HI, H.STRIP_SLACK)
    G, g, g_out = restated_strip(O, scene, H.G_LO, H.G_HI)
    F, f, f_out = restated_strip(O, scene, H.W_LO, H.W_HI)
    for name, out in (("W", w), ("G", g), ("F", f)):
        print("seed %d arm %s: worst |R| %.3e |t| %.3e, passes %s, states %s" % (
            seed, name, max(e[2] for e in out), max(e[3] for e in out), [e[1]["iterations"] for e in out], [e[1]["state"] for e in out]))
    assert list(W.dims) == list(F.dims) == [33, 33, 33] and list(G.dims) == [83, 33, 33]
    assert w_out == 0 and g_out == 0 and f_out > 0.4 * sum(sizes)
    assert W.window()[0] >= 28 and W.mapped < G.mapped == sum(sizes)
    for out in (w, g):
        assert all(r["converged"] for _, r, _, _, _ in out)
        assert all(r["info"][0] > 0.6 * sizes[k] for k, r, _, _, _ in out)
        assert max(e[2] for e in out) <= 1.001 * STRIP_CPU[seed][0] and max(e[3] for e in out) <= 1.001 * STRIP_CPU[seed][1]   # as measured
    lin, rows = H.as_seen_from(G, W)                                  # consequence 3 at the end of a real walk
    assert np.array_equal(lin, W.lin) and np.array_equal(_bits(G.stats[rows]), _bits(W.stats))
    bar = max(STRIP_CPU[seed])
    for k, r, eR, et, _ in f:
        if H.STRIP_STEP * k - 1.0 >= 1.7:
            scan, sn, Rk, tk = scene[k]
            Tk = np.eye(4)
            Tk[:3, :3], Tk[:3, 3] = Rk, tk
            p0, n0 = R.start_at(O, Tk.astype(F32), scan, sn)
            assert H.sums(p0, n0, F, 1.0)[0][0] == 0
            assert H.icp_vgicp(O, p0, n0, F, max_iterations=50)["state"] == V.STATE_NO_CORRESPONDENCES
            assert r["state"] == V.STATE_NO_CORRESPONDENCES or max(eR, et) > 10 * bar, (k, r["state"], eR, et)
    assert max(e[3] for e in f) > 10 * bar
