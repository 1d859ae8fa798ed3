"""CPU tests of point-to-plane ICP's host side: kss_rigid_from_p2l_sums against tests/p2l_ref.py bit for bit, the
degenerate case, and the public constants / symbols of the feature."""
import os
import re

import numpy as np

import p2l_ref as R
from conftest import ROOT

F32, F64 = np.float32, np.float64


def _sums_from_system(A, b):
    """A 32-slot record holding ATA = A (upper triangle) and ATb = b."""
    s = np.zeros(R.NSUMS, F64)
    s[0] = 100.0
    k = 1
    for i in range(6):
        for j in range(i, 6):
            s[k] = A[i, j]
            k += 1
    s[22:28] = b
    return s


def test_rigid_random_spd_bit_for_bit(pkg):
    rng = np.random.default_rng(11)
    for trial in range(200):
        M = rng.normal(size=(6 + trial % 5, 6)) * rng.uniform(0.01, 10.0, size=6)
        A = M.T @ M
        b = rng.normal(size=6) * 10.0 ** rng.uniform(-4, 0)
        s = _sums_from_system(A, b)
        T, rc = pkg.rigid_from_p2l_sums(s)
        Tr, degenerate = R.rigid(s)
        assert rc == 0 and not degenerate
        assert T.dtype == F32 and np.array_equal(T.view(np.uint32), Tr.view(np.uint32)), (trial, T, Tr)


def _linear_sums(x_true, n=500, seed=5):
    """Sums of correspondences whose residuals are exactly linear in the motion: r = v . x_true."""
    rng = np.random.default_rng(seed)
    src = rng.uniform(-1, 1, size=(n, 3)).astype(F32)
    nrm = rng.normal(size=(n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F32)
    sx, sy, sz = src[:, 0], src[:, 1], src[:, 2]
    nx, ny, nz = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    v = np.stack([nz * sy - ny * sz, nx * sz - nz * sx, ny * sx - nx * sy, nx, ny, nz], axis=1).astype(F64)
    r = v @ np.asarray(x_true, F64)
    s = np.zeros(R.NSUMS, F64)
    s[0] = n
    k = 1
    for p in range(6):
        for q in range(p, 6):
            s[k] = (v[:, p] * v[:, q]).sum()
            k += 1
    for p in range(6):
        s[22 + p] = (v[:, p] * r).sum()
    return s


def test_rigid_exact_linear_data_recovers_motion(pkg):
    for x_true in ([0.01, -0.02, 0.03, 0.1, -0.05, 0.2], [0.1, 0.05, -0.12, -0.3, 0.0, 0.01], [0.0] * 6):
        s = _linear_sums(x_true)
        T, rc = pkg.rigid_from_p2l_sums(s)
        Tr, degenerate = R.rigid(s)
        assert rc == 0 and not degenerate
        assert np.array_equal(T.view(np.uint32), Tr.view(np.uint32))
        assert np.abs(T.astype(F64) - R.construct(x_true).astype(F64)).max() <= 1e-6
        assert np.abs(T[:3, 3] - np.asarray(x_true[3:], F64)).max() <= 1e-6


def test_planar_target_is_degenerate(pkg):
    rng = np.random.default_rng(3)
    tgt = np.zeros((400, 3), F32)
    tgt[:, :2] = rng.uniform(-1, 1, size=(400, 2))
    nrm = np.tile(np.array([0, 0, 1], F32), (400, 1))
    src = tgt + np.array([0.01, 0.02, 0.05], F32)
    s, _ = R.sums(src, tgt, nrm, np.arange(400), 1.0)
    assert s[0] == 400
    T, rc = pkg.rigid_from_p2l_sums(s)
    assert rc == pkg.ERR_DEGENERATE == -7
    assert np.array_equal(T, np.eye(4, dtype=F32))
    assert R.rigid(s)[1]
    # and a record with nothing in it
    T, rc = pkg.rigid_from_p2l_sums(np.zeros(32))
    assert rc == -7 and np.array_equal(T, np.eye(4, dtype=F32))


def test_status_string(pkg):
    L = pkg.load_library()
    assert L.kss_status_string(-7) == b"degenerate point-to-plane system"
    assert L.kss_status_string(-6) == b"RCCL error"


def test_constants_and_symbols(pkg):
    assert pkg.P2L_NSUMS == 32 and pkg.STATE_DEGENERATE == 6
    hdr = open(os.path.join(ROOT, "include", "kssicp.h")).read()
    assert re.search(r"#define KSS_P2L_NSUMS 32\b", hdr)
    assert re.search(r"KSS_STATE_DEGENERATE = 6\b", hdr)
    assert re.search(r"KSS_ERR_DEGENERATE = -7\b", hdr)
    exported = set(pkg.exported_symbols())
    for s in ("kss_p2l_sums", "kss_p2l_sums_dev", "kss_rigid_from_p2l_sums", "kss_icp_p2l", "kss_icp_p2l_dev"):
        assert s in pkg.binding.SYMBOLS and s in exported, s
    for name in ("icp_p2l", "icp_p2l_dev", "p2l_sums"):
        assert callable(getattr(pkg.Context, name))
