"""The voxel-map pyramid, the parts that need no GPU: the exported symbols and binding methods, the
restatement in tests/vmap_pyramid_ref.py against tests/vgicp_ref.py's build() -- which knows nothing of sums, bases or parents
-- at the coarse leaf, its bookkeeping, a shifted map, and the ladder scene on the restatement alone: the check that the GPU
test's scene is fair, and the source of its error bar.

The ladder scene (halves_pair(S, seed, 4000, 55 degrees, axis (0.3, -0.5, 1)), PCL normals at k = 20, fine leaf 0.05,
max_iterations 200), measured with the restatement, max|R - R_true| and max|t - t_true|, passes per level of the ladder 8 4 2 1:
    seed 8   fine map alone 6.17e-01  1.29e-02    ladder 7.06e-05  3.67e-05   (10, 2, 2, 2)
    seed 3   fine map alone 7.60e-01  5.68e-02    ladder 3.05e-05  5.06e-05   (3, 12, 2, 2)
    seed 5   fine map alone 7.06e-01  9.02e-02    ladder 4.75e-05  5.54e-05   (9, 3, 2, 2)"""
import os
import re

import numpy as np
import pytest

import vgicp_ref as V
import vmap_pyramid_ref as Y
import vmap_shift_ref as H
from conftest import ROOT

F32, F64, I64 = np.float32, np.float64, np.int64
NAMES = ["kss_vmap_coarsen", "kss_vmap_coarsen_into", "kss_icp_vgicp_from", "kss_icp_vgicp_from_dev", "kss_icp_vgicp_c2f",
         "kss_icp_vgicp_c2f_dev"]
AXIS = [0.3, -0.5, 1.0]
FINE_LEAF, LADDER = 0.05, (8, 4, 2)
LADDER_BAR, LOST_BAR = 2e-4, 1e-1


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)


def ladder_scene(S, O, seed, deg=55.0, n=4000):
    """(src, its normals, the fine restated map, R_true, t_true) of the ladder scene."""
    src, tgt, R_true, t_true = V.halves_pair(S, seed, n, deg, axis=AXIS)
    sn = O.normals_pcl(src.astype(F64), 20).astype(F32)
    tn = O.normals_pcl(tgt.astype(F64), 20).astype(F32)
    return src, sn, tgt, tn, R_true, t_true


def test_symbols_exported_listed_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "kssicp.h")).read()
    declared = set(re.findall(r"\b(kss_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    exported = set(pkg.exported_symbols())
    for n in NAMES:
        assert n in declared and n in pkg.binding.SYMBOLS and n in exported, n
    L = pkg.load_library()
    assert len(L.kss_vmap_coarsen.argtypes) == 4 and len(L.kss_vmap_coarsen_into.argtypes) == 4
    assert len(L.kss_icp_vgicp_from.argtypes) == len(L.kss_icp_vgicp_from_dev.argtypes) == 10
    assert len(L.kss_icp_vgicp_c2f.argtypes) == len(L.kss_icp_vgicp_c2f_dev.argtypes) == 11
    for n in ("coarsen", "coarsen_into"):
        assert callable(getattr(pkg.VoxelMap, n)), n
    for n in ("icp_vgicp_from", "icp_vgicp_from_dev", "icp_vgicp_c2f", "icp_vgicp_c2f_dev"):
        assert callable(getattr(pkg.Context, n)), n
    assert re.search(r"#define\s+KSS_VGICP_MAX_LEVELS\s+8\b", hdr) and Y.MAX_LEVELS == 8
    # a null context is refused before anything touches a device
    assert L.kss_vmap_coarsen(None, None, 2, None) == -1
    assert L.kss_vmap_coarsen_into(None, None, 2, None) == -1
    for n in ("kss_icp_vgicp_from", "kss_icp_vgicp_from_dev"):
        assert getattr(L, n)(None, None, 0, None, None, None, None, None, None, None) == -1
    for n in ("kss_icp_vgicp_c2f", "kss_icp_vgicp_c2f_dev"):
        assert getattr(L, n)(None, None, 0, None, None, 0, None, None, None, None, None) == -1


@pytest.fixture(scope="module")
def cloud(pkg):
    n = 5000
    return pkg.synth.bumpy(11, n).astype(F32), _unit(np.random.default_rng(11), n)


@pytest.fixture(scope="module")
def fine(cloud):
    return H.create(cloud[0], cloud[1], 2.0 ** -4)


def _decoded(lin, dims):
    dx, dy = int(dims[0]), int(dims[1])
    return np.stack([lin % dx, lin // dx % dy, lin // (dx * dy)], axis=1)


@pytest.mark.parametrize("k", [2, 4, 8])
def test_coarsen_against_independent_build(cloud, fine, k):
    """leaf and k are powers of two, so the point's own coarse cell is its fine voxel's parent: the coarsened map must hold the
    voxels of a map built at the coarse leaf -- the same cells and counts, and sums that differ by their order of addition alone."""
    A, an = cloud
    before = fine.copy()
    c = Y.coarsen(fine, k)
    ref = V.build(A, an, k * 2.0 ** -4)
    assert c.inv == F32(16 // k) and c.leaf == k * 2.0 ** -4 and np.array_equal(c.lo, ref.lo)
    assert np.array_equal(c.dims, (fine.dims + k - 2) // k + 1) and (c.dims >= ref.dims).all() and (c.dims <= fine.dims).all()
    assert np.array_equal(_decoded(c.lin, c.dims), _decoded(ref.lin, ref.dims))
    assert (np.diff(c.lin) > 0).all()
    assert np.array_equal(c.N, ref.stats[:, 0])
    err = np.abs(c.stats - ref.stats).max()
    print("k %d: %d -> %d voxels, inv' %g, max |stats - build| %.2e" % (k, len(fine.lin), len(c.lin), c.inv, err))
    assert err <= 1e-14
    for x, y in zip((fine.lin, fine.N, fine.s, fine.P, fine.info()), (before.lin, before.N, before.s, before.P, before.info())):
        assert np.array_equal(_bits(x), _bits(y))


@pytest.mark.parametrize("k", [2, 3, 4, 5, 8])
def test_bookkeeping(fine, k):
    c = Y.coarsen(fine, k)
    assert c.N.sum() == fine.N.sum() == fine.mapped == c.mapped
    C = Y.parents(fine, k)
    plin = (C[:, 2] * c.dims[1] + C[:, 1]) * c.dims[0] + C[:, 0]
    assert np.isin(plin, c.lin).all() and np.array_equal(np.unique(plin), c.lin)
    at = np.searchsorted(c.lin, plin)
    children = np.bincount(at, minlength=len(c.lin))
    one = np.flatnonzero(children == 1)
    assert len(one) > 0
    child = np.array([np.flatnonzero(at == v)[0] for v in one])
    assert np.array_equal(_bits(c.N[one]), _bits(fine.N[child]))
    assert np.array_equal(_bits(c.s[one]), _bits(fine.s[child])) and np.array_equal(_bits(c.P[one]), _bits(fine.P[child]))
    assert np.array_equal(_bits(c.stats[one]), _bits(fine.stats[child]))
    assert Y.coarsen(fine, 1) is None and Y.coarsen(fine, 9) is None


@pytest.mark.parametrize("k,base,nvox", [(2, (-2, 0, 2), 1003), (3, (-1, 0, 1), 507), (4, (-1, 0, 1), 308)])
def test_shifted_map(fine, k, base, nvox):
    m = fine.copy()
    H.shift(m, (-3, 1, 5))
    assert len(m.lin) == 2478
    c = Y.coarsen(m, k)
    assert np.array_equal(c.window(), base)
    C = Y.parents(m, k)
    assert ((C >= 0) & (C < c.dims)).all()
    assert c.N.sum() == m.N.sum() == m.mapped == c.mapped
    assert len(c.lin) == nvox
    # the parent of a fine voxel holds the fine voxel's lattice cell
    a = H.local_cells(m) + m.window()
    A = _decoded(c.lin, c.dims) + c.window()
    assert {tuple(x) for x in a // k} == {tuple(x) for x in A}


def test_coarsen_into_restated(cloud, fine):
    A, an = cloud
    c = Y.coarsen(fine, 2)
    dst = Y.coarsen(fine, 2)
    H.insert(dst, A[:100] + F32(0.3), an[:100])
    H.shift(dst, (1, 0, -2))
    m = fine.copy()
    H.shift(m, (4, -2, 0))
    assert Y.coarsen_into(m, 2, dst)
    want = Y.coarsen(m, 2)
    for x, y in zip((dst.lin, dst.N, dst.s, dst.P, dst.info(), dst.window()), (want.lin, want.N, want.s, want.P, want.info(), want.window())):
        assert np.array_equal(_bits(x), _bits(y))
    assert not Y.coarsen_into(m, 4, dst) and not Y.coarsen_into(m, 2, m) and not Y.coarsen_into(c, 2, dst)


@pytest.mark.parametrize("seed", [8, 3, 5])
def test_ladder_scene(pkg, O, seed):
    """From 55 degrees the fine map alone is lost and the ladder 8 4 2 1 ends where the fine map ends from a good start."""
    src, sn, tgt, tn, R_true, t_true = ladder_scene(pkg.synth, O, seed)
    vm = H.create(tgt, tn, FINE_LEAF)
    alone = H.icp_vgicp(O, src, sn, vm, max_iterations=200)
    eR0, et0 = V.errors(alone["T"], R_true, t_true)
    rs = Y.icp_vgicp_c2f(O, src, sn, Y.ladder(vm, LADDER), max_iterations=200)
    eR, et = V.errors(rs[-1]["T"], R_true, t_true)
    print("seed %d: fine map alone %.2e %.2e   ladder %.2e %.2e  passes %s states %s" % (
        seed, eR0, et0, eR, et, [r["iterations"] for r in rs], [r["state"] for r in rs]))
    assert eR0 >= LOST_BAR
    assert eR <= LADDER_BAR and et <= LADDER_BAR
    assert [r["fitness"] for r in rs[:-1]] == [0.0] * 3 and rs[-1]["fitness"] > 0.0


def test_from_identity_and_none(pkg, O):
    """T0 None is icp_vgicp; an identity T0 moves nothing and gives the same result."""
    src, sn, tgt, tn, _, _ = ladder_scene(pkg.synth, O, 8, deg=10.0, n=1000)
    vm = H.create(tgt, tn, 0.1)
    a = Y.icp_vgicp_from(O, src, sn, vm, None, max_iterations=30)
    b = Y.icp_vgicp_from(O, src, sn, vm, np.eye(4, dtype=F32), max_iterations=30)
    assert a["iterations"] == b["iterations"] >= 2 and np.array_equal(_bits(a["T"]), _bits(b["T"]))
    assert np.array_equal(_bits(a["trace_sums"]), _bits(b["trace_sums"]))
    bad = np.eye(4, dtype=F32)
    bad[1, 3] = np.nan
    assert Y.icp_vgicp_from(O, src, sn, vm, bad) is None
    assert Y.icp_vgicp_c2f(O, src, sn, []) is None and Y.icp_vgicp_c2f(O, src, sn, [vm] * 9) is None
