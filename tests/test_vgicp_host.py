"""Voxelized generalized ICP, the parts that need no GPU: the exported symbols and default parameters, and the restatement in
tests/vgicp_ref.py itself on the scenes the GPU tests use -- two independent samplings of one surface, where the voxel metric ends
where generalized ICP ends, far closer than point-to-point ICP: the check that the GPU tests' inputs are fair."""
import numpy as np
import pytest

import vgicp_ref as V

F32, F64 = np.float32, np.float64
NAMES = ["kss_vmap_default_params", "kss_vmap_create", "kss_vmap_create_dev", "kss_vmap_destroy", "kss_vmap_info", "kss_vmap_read",
         "kss_vgicp_sums", "kss_vgicp_sums_dev", "kss_icp_vgicp", "kss_icp_vgicp_dev"]


def test_symbols_exported_and_listed(pkg):
    exported = set(pkg.exported_symbols())
    for n in NAMES:
        assert n in pkg.binding.SYMBOLS and n in exported, n
    for n in ("vmap", "vmap_dev", "vgicp_sums", "vgicp_sums_dev", "icp_vgicp", "icp_vgicp_dev"):
        assert callable(getattr(pkg.Context, n)), n
    for n in ("info", "read", "close"):
        assert callable(getattr(pkg.VoxelMap, n)), n
    assert (pkg.VMAP_NINFO, pkg.VMAP_NSTAT, pkg.VGICP_NINFO) == (10, 10, 4)


def test_default_params(pkg):
    vp = pkg.vmap_params()
    assert vp.leaf == 0.0 and vp.normals_k == 20          # no default leaf: the caller sets it
    vp = pkg.vmap_params(leaf=0.25, normals_k=12)
    assert vp.leaf == 0.25 and vp.normals_k == 12
    with pytest.raises(AttributeError):
        pkg.vmap_params(epsilon=0.5)
    assert pkg.load_library().kss_vmap_default_params(None) == -1


def test_restatement_map_is_the_definition():
    """The bincount map against a plain Python loop over the targets in index order, bit for bit, on a small cloud with unmapped
    targets and several points per voxel."""
    rng = np.random.default_rng(3)
    tgt = rng.uniform(-1, 1, size=(300, 3)).astype(F32)
    nrm = rng.normal(size=(300, 3)).astype(F32)
    tgt[5, 1] = np.nan; tgt[17, 0] = np.inf; nrm[40, 2] = np.nan; nrm[41] = -np.inf
    vm = V.build(tgt, nrm, 0.5)
    assert vm.mapped == 296 and len(vm.lin) < 296
    acc = {}
    for i in range(300):
        if not (np.isfinite(tgt[i]).all() and np.isfinite(nrm[i]).all()):
            continue
        f = np.floor((tgt[i] - vm.lo) * vm.inv)
        assert f.dtype == F32
        lin = (int(f[2]) * int(vm.dims[1]) + int(f[1])) * int(vm.dims[0]) + int(f[0])
        a = acc.setdefault(lin, [0, [0.0] * 3, [0.0] * 6])
        a[0] += 1
        q, n = [float(x) for x in tgt[i]], [float(x) for x in nrm[i]]
        for k in range(3):
            a[1][k] += q[k]
        for k, (r, c) in enumerate([(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]):
            a[2][k] += n[r] * n[c]
    assert sorted(acc) == list(vm.lin)
    for row, lin in zip(vm.stats, vm.lin):
        N, s, Pn = acc[int(lin)]
        want = np.array([float(N)] + [x / float(N) for x in s] + [x / float(N) for x in Pn])
        assert np.array_equal(row.view(np.uint64), want.view(np.uint64))
    for leaf in (0.0, -1.0, float("nan"), float("inf"), 1e-6):   # the last: far more than 2^26 cells
        assert V.build(tgt, nrm, leaf) is None
    assert V.build(tgt, np.full_like(nrm, np.nan), 0.5) is None


def test_restatement_beats_point_to_point_on_disjoint_halves(pkg, O):
    """2 x 4000 points of one bumpy surface, no point shared, 10 degrees about (0.3, -0.5, 1), normals by 20-NN PCA on each cloud
    as it is passed in, leaf 0.1 (2.6 points per voxel): the f64 numpy prototype gave 6.9e-5 against point-to-point's 1.2e-2."""
    src, tgt, R_true, t_true = V.halves_pair(pkg.synth, 8, 4000, 10.0, axis=[0.3, -0.5, 1.0])
    sn = O.normals_pcl(src.astype(F64), 20).astype(F32)
    tn = O.normals_pcl(tgt.astype(F64), 20).astype(F32)
    vm = V.build(tgt, tn, 0.1)
    ref = V.icp_vgicp(O, src, sn, vm, max_iterations=200)
    eR, et = V.errors(ref["T"], R_true, t_true)
    p2p = O.icp(src, tgt, O.icp_params(max_iterations=200))
    pR, pt = V.errors(p2p["T"], R_true, t_true)
    print("vgicp: %d voxels (%.1f points each), %d passes, state %d, |R - R_true| %.2e, |t - t_true| %.2e;  point-to-point: %d passes, "
          "%.2e, %.2e" % (len(vm.lin), vm.mapped / len(vm.lin), ref["iterations"], ref["state"], eR, et, p2p["iterations"], pR, pt))
    assert ref["converged"]
    assert eR <= 1e-3 and eR <= 0.25 * pR


def test_restatement_sparse_scan_dense_map(pkg, O):
    """A 2000-point scan against the map of 20000 points, 10 degrees, leaf 0.1: the prototype gave 2.3e-4 and 1.6e-4."""
    src, tgt, R_true, t_true = V.halves_pair(pkg.synth, 5, 20000, 10.0, n_src=2000)
    sn = O.normals_pcl(src.astype(F64), 20).astype(F32)
    tn = O.normals_pcl(tgt.astype(F64), 20).astype(F32)
    ref = V.icp_vgicp(O, src, sn, V.build(tgt, tn, 0.1), max_iterations=200)
    eR, et = V.errors(ref["T"], R_true, t_true)
    print("%d passes, state %d, |R - R_true| %.2e, |t - t_true| %.2e" % (ref["iterations"], ref["state"], eR, et))
    assert eR <= 1e-3 and et <= 1e-3
