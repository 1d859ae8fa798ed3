"""Symmetric ICP, the parts that need no GPU: the exported symbols and default parameters, the host-only step
kss_rigid_from_symm_sums bit for bit against the same expression in Python floats (the host's f64 +, -, *, /, sqrt are IEEE),
and the restatement in tests/symm_ref.py itself on the pairs the GPU tests use: disjoint halves of one surface turned by 65
degrees, which the symmetric step registers and both existing plane metrics lose -- the check that the GPU tests' inputs are
fair."""
import numpy as np
import pytest

import gicp_ref as G
import p2l_ref as P
import symm_ref as S

F32, F64 = np.float32, np.float64
NAMES = ["kss_symm_default_params", "kss_rigid_from_symm_sums", "kss_symm_sums", "kss_symm_sums_dev", "kss_icp_symm", "kss_icp_symm_dev"]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == F64 else np.uint32)


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)


def _record(seed, angle, n=400):
    """A record made by the restatement from random correspondences: a random target with random unit normals, the source the
    target turned by 0.5 rad about a random axis and shifted, every source paired with the point it came from; then the right-hand
    side scaled by angle / 0.5, so that the solved step (linear in it) has a rotation of about `angle` whatever the float
    rounding of the clouds."""
    rng = np.random.default_rng(seed)
    tgt = rng.uniform(-1, 1, size=(n, 3))
    tn = _unit(rng, n)
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + np.sin(0.5) * K + (1 - np.cos(0.5)) * (K @ K)
    src = (tgt @ R.T + 0.05 * rng.normal(size=3)).astype(F32)
    sn = (tn.astype(F64) @ R.T).astype(F32)
    s, _ = S.sums(src, sn, tgt.astype(F32), tn, np.arange(n, dtype=np.int32), 1e30)
    s[22:28] *= angle / 0.5
    return s


def test_symbols_exported_and_listed(pkg):
    exported = set(pkg.exported_symbols())
    for n in NAMES:
        assert n in pkg.binding.SYMBOLS and n in exported, n
    for n in ("symm_sums", "symm_sums_dev", "icp_symm", "icp_symm_dev"):
        assert callable(getattr(pkg.Context, n)), n


def test_default_params(pkg):
    sp = pkg.symm_params()
    assert sp.normals_k == 20 and sp.align_normals == 1
    sp = pkg.symm_params(normals_k=12, align_normals=0)
    assert sp.normals_k == 12 and sp.align_normals == 0
    with pytest.raises(AttributeError):
        pkg.symm_params(epsilon=0.5)
    L = pkg.load_library()
    assert L.kss_symm_default_params(None) == -1
    assert L.kss_rigid_from_symm_sums(None, None) == -1


@pytest.mark.parametrize("angle", [1e-9, 1e-6, 1e-3, 0.03, 0.3, 1.0])
def test_step_bit_for_bit_and_orthonormal(pkg, angle):
    for seed in range(8):
        s = _record(1000 + seed, angle)
        x = P.solve(s)
        assert x is not None
        got, rc = pkg.rigid_from_symm_sums(s)
        ref, degenerate = S.rigid(s)
        assert rc == 0 and not degenerate
        assert np.array_equal(_bits(got), _bits(ref)), (angle, seed, got, ref)
        # the solved rotation has about the size asked for: the half angle is atan|a|
        size = 2.0 * np.arctan(np.linalg.norm(x[:3]))
        assert 0.5 * angle <= size <= 2.0 * angle, (angle, size)
        # orthonormal to the float rounding of the entries
        R = got[:3, :3].astype(F64)
        assert np.abs(R @ R.T - np.eye(3)).max() <= 4e-7
        assert np.array_equal(got[3], np.array([0, 0, 0, 1], F32))
        H, _ = S.half(x)
        assert np.abs(H @ H.T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(H) - 1.0) <= 1e-12


def test_step_zero_rhs_is_identity_and_zero_diagonal_is_degenerate(pkg):
    s = _record(7, 0.1)
    z = s.copy()
    z[22:28] = 0.0
    got, rc = pkg.rigid_from_symm_sums(z)
    ref, degenerate = S.rigid(z)
    assert rc == 0 and not degenerate
    assert np.array_equal(got, np.eye(4, dtype=F32)) and np.array_equal(ref, np.eye(4, dtype=F32))
    d = s.copy()
    d[12] = 0.0          # the third diagonal entry of sum v v^T
    got, rc = pkg.rigid_from_symm_sums(d)
    ref, degenerate = S.rigid(d)
    assert rc == pkg.ERR_DEGENERATE and degenerate
    assert np.array_equal(got, np.eye(4, dtype=F32)) and np.array_equal(ref, np.eye(4, dtype=F32))


@pytest.fixture(scope="module")
def wide_pairs(pkg, O):
    """The 65 degree pairs of the GPU tests with the oracle's 20-NN PCA normals, shared by the tests below."""
    out = {}
    for seed in (8, 3):
        src, tgt, R_true, t_true = S.halves_pair(pkg.synth, seed, 2000, 65.0, axis=[0.3, -0.5, 1.0])
        sn = O.normals_pcl(src.astype(F64), 20).astype(F32)
        tn = O.normals_pcl(tgt.astype(F64), 20).astype(F32)
        out[seed] = (src, sn, tgt, tn, R_true, t_true)
    return out


@pytest.mark.parametrize("seed", [8, 3])
def test_restatement_registers_65_degrees_where_both_plane_metrics_fail(O, wide_pairs, seed):
    src, sn, tgt, tn, R_true, t_true = wide_pairs[seed]
    sym = S.icp_symm(O, src, sn, tgt, tn, max_iterations=100)
    sR, st = S.errors(sym["T"], R_true, t_true)
    p2l = P.icp_p2l(O, src, tgt, tn, max_iterations=100)
    pR, pt = S.errors(p2l["T"], R_true, t_true)
    gic = G.icp_gicp(O, src, sn, tgt, tn, max_iterations=100)
    gR, gt = S.errors(gic["T"], R_true, t_true)
    print("seed %d, 2 x 2000, 65 degrees: symmetric %d passes, state %d, |R - R_true| %.2e, |t - t_true| %.2e;  point-to-plane %d, %.2e, "
          "%.2e;  generalized %d, %.2e, %.2e" % (seed, sym["iterations"], sym["state"], sR, st, p2l["iterations"], pR, pt,
                                                 gic["iterations"], gR, gt))
    assert sym["converged"] and sR <= 1e-3
    assert pR >= 0.5 and gR >= 0.5


def test_restatement_normal_signs_do_not_matter(O, wide_pairs):
    src, sn, tgt, tn, _, _ = wide_pairs[8]
    rng = np.random.default_rng(21)
    sf, tf = sn.copy(), tn.copy()
    sf[rng.random(len(sf)) < 0.5] *= F32(-1.0)
    tf[rng.random(len(tf)) < 0.5] *= F32(-1.0)
    assert not np.array_equal(sf, sn) and not np.array_equal(tf, tn)
    a = S.icp_symm(O, src, sn, tgt, tn, max_iterations=100)
    b = S.icp_symm(O, src, sf, tgt, tf, max_iterations=100)
    assert a["iterations"] == b["iterations"] >= 2 and a["state"] == b["state"]
    assert np.array_equal(_bits(a["T"]), _bits(b["T"]))
    assert np.array_equal(_bits(a["trace_Tk"]), _bits(b["trace_Tk"]))
