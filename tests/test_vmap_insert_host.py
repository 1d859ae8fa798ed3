"""A voxel map that grows, the parts that need no GPU: the exported symbols and binding methods, the restatement
in tests/vmap_insert_ref.py against the independent tests/vgicp_ref.build() on the three consequences the header states, and the
scan-to-map sequence on the restatement alone -- the growing map keeps every scan registered where the static map of the first
view runs out of correspondences: the check that the GPU test's scene is fair, and the source of its error bar."""
import os
import re

import numpy as np
import pytest

import vgicp_ref as V
import vmap_insert_ref as R
from conftest import ROOT

F32, F64 = np.float32, np.float64
NAMES = ["kss_vmap_create_box", "kss_vmap_insert", "kss_vmap_insert_dev"]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def _same(a, b):
    assert np.array_equal(a.lin, b.lin)
    assert np.array_equal(_bits(a.stats), _bits(b.stats))
    assert np.array_equal(_bits(a.info()), _bits(b.info()))


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)


def test_symbols_exported_listed_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "kssicp.h")).read()
    declared = set(re.findall(r"\b(kss_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    exported = set(pkg.exported_symbols())
    for n in NAMES:
        assert n in declared and n in pkg.binding.SYMBOLS and n in exported, n
    L = pkg.load_library()
    assert len(L.kss_vmap_create_box.argtypes) == 5
    assert len(L.kss_vmap_insert.argtypes) == 8 and len(L.kss_vmap_insert_dev.argtypes) == 8
    for n in ("insert", "insert_dev"):
        assert callable(getattr(pkg.VoxelMap, n)), n
    assert callable(pkg.Context.vmap_box)
    assert pkg.VMAP_NINSERT == 4 == R.NINSERT
    # a null context is refused before anything touches a device
    assert L.kss_vmap_create_box(None, None, None, None, None) == -1
    assert L.kss_vmap_insert(None, None, None, 1, None, None, 20, None) == -1
    assert L.kss_vmap_insert_dev(None, None, None, 1, None, None, 20, None) == -1


@pytest.mark.parametrize("leaf", [1e3, 0.1, 1e-2])
@pytest.mark.parametrize("n", [1, 257, 5000])
def test_restatement_create_then_insert_is_create_of_the_concatenation(pkg, n, leaf):
    """Consequence 1, and create() itself against build()."""
    A = pkg.synth.bumpy(n, n).astype(F32)
    B = (pkg.synth.bumpy(500 + n, n) * 1.05).astype(F32)          # some of B lies outside A's box
    rng = np.random.default_rng(n)
    an, bn = _unit(rng, n), _unit(rng, n)
    if n > 1:
        B[3, 1] = np.nan; bn[5] = np.inf
    m = R.create(A, an, leaf)
    _same(m, V.build(A, an, leaf))
    sel = R.select(m, B, bn)[0]
    info = R.insert(m, B, bn)
    _same(m, V.build(np.concatenate([A, B[sel]]), np.concatenate([an, bn[sel]]), leaf))
    assert info[0] == sel.sum() and info[:3].sum() == n and m.mapped == n + sel.sum()
    if n == 5000 and leaf == 0.1:
        assert 0 < info[2] < n and info[1] == 2 and info[3] > 0


def test_restatement_box_map_any_split(pkg):
    """Consequence 2 down to one point per call, against build() where the box's origin is the cloud's own minimum."""
    n = 257
    A = pkg.synth.bumpy(9, n).astype(F32)
    an = _unit(np.random.default_rng(9), n)
    lo, hi = A.min(0), A.max(0)
    whole = R.box(lo, hi, 0.1)
    R.insert(whole, A, an)
    _same(whole, V.build(A, an, 0.1))
    for chunk in (1, 7, 256):
        m = R.box(lo, hi, 0.1)
        for i in range(0, n, chunk):
            R.insert(m, A[i:i + chunk], an[i:i + chunk])
        _same(m, whole)


def test_restatement_pose(pkg):
    """Consequence 3: an identity T gives the bits of None; a real pose is the map of the moved cloud with the turned normals
    (build() takes float normals, so only the positions' part of the record is compared with it)."""
    n = 1000
    A = pkg.synth.bumpy(4, n).astype(F32)
    an = _unit(np.random.default_rng(4), n)
    A[7, 0] = -0.0
    a, b = R.box(R.BOX_LO, R.BOX_HI, 0.1), R.box(R.BOX_LO, R.BOX_HI, 0.1)
    R.insert(a, A, an)
    R.insert(b, A, an, np.eye(4, dtype=F32))
    _same(a, b)
    T = np.eye(4)
    T[:3, :3] = pkg.synth.rot_axis_angle(R.AXIS, np.deg2rad(17.0))
    T[:3, 3] = [0.05, -0.02, 0.04]
    c = R.box(R.BOX_LO, R.BOX_HI, 0.1)
    R.insert(c, A, an, T.astype(F32))
    q, m = R.moved(A, an, T.astype(F32))
    d = R.box(R.BOX_LO, R.BOX_HI, 0.1)
    R.insert(d, q, an)
    assert np.array_equal(c.lin, d.lin) and np.array_equal(_bits(c.stats[:, :4]), _bits(d.stats[:, :4]))
    assert np.abs(np.linalg.norm(m, axis=1) - 1.0).max() < 1e-6
    assert np.abs(c.stats[:, [4, 7, 9]].sum(1) - 1.0).max() < 1e-6     # trace of the average m m^T


def test_restatement_box_refusals():
    for lo, hi, leaf in (([0, 0, 0], [1, 1, np.nan], 0.1), ([0, 0, -np.inf], [1, 1, 1], 0.1), ([0, 0, 0], [1, -1, 1], 0.1),
                         ([0, 0, 0], [1, 1, 1], 0.0), ([0, 0, 0], [1, 1, 1], np.nan), ([0, 0, 0], [1, 1, 1], 1e-3),
                         ([0, 0, 0], [1, 1, 1], 1e-40)):
        assert R.box(lo, hi, leaf) is None
    m = R.box([-0.0, 0, 0], [0, 0, 0], 0.1)
    assert list(m.dims) == [1, 1, 1] and not np.signbit(m.lo).any() and len(m.lin) == 0 and m.stats.shape == (0, 10)


@pytest.fixture(scope="module")
def scenes(pkg, O):
    return {seed: R.sequence_scene(pkg.synth, O, seed) for seed in (8, 3)}


def restated_sequence(O, scene, grow):
    vm = R.box(R.BOX_LO, R.BOX_HI, R.LEAF)
    return R.run_sequence(O, scene, lambda k, p, n: V.icp_vgicp(O, p, n, vm, max_iterations=50),
                          lambda k, scan, sn, T: R.insert(vm, scan, sn, T), grow)


@pytest.mark.parametrize("seed", [8, 3])
def test_restated_sequence_growing_and_static(O, scenes, seed):
    """Measured with this restatement (sums continued, normals turned in f64): see the figures in DESIGN.md 2.34."""
    scene = scenes[seed]
    sizes = [len(s[0]) for s in scene]
    assert min(sizes) > 1000 and sum(sizes) < 48000
    grown = restated_sequence(O, scene, True)
    for k, r, eR, et, _ in grown:
        print("seed %d growing scan %d: %d passes, state %d, kept %d of %d, |R| %.2e |t| %.2e" % (
            seed, k, r["iterations"], r["state"], int(r["info"][0]), sizes[k], eR, et))
        assert r["converged"] and r["info"][0] > 0.6 * sizes[k]
    assert max(e[2] for e in grown) <= 5e-3 and max(e[3] for e in grown) <= 5e-3
    static = restated_sequence(O, scene, False)
    for k, r, eR, et, _ in static:
        print("seed %d static scan %d: %d passes, state %d, kept %d of %d, |R| %.2e |t| %.2e" % (
            seed, k, r["iterations"], r["state"], int(r["info"][0]), sizes[k], eR, et))
    assert [e[1]["state"] for e in static[5:]] == [V.STATE_NO_CORRESPONDENCES] * 2
    kept = [e[1]["info"][0] for e in static]
    assert kept[0] > 2 * kept[3] > 0                                  # the overlap with view 0 runs out scan by scan
