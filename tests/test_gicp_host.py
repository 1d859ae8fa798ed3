"""Generalized ICP, the parts that need no GPU: the exported symbols and default parameters, the host-only helper
kss_gicp_metric bit for bit against the same expression in Python floats (the host's f64 +, -, *, / are IEEE), and the
restatement in tests/gicp_ref.py itself on the pair the GPU tests use: two independent samplings of one surface, where the
generalized metric recovers the motion an order better than point-to-point ICP -- the check that the GPU tests' inputs are
fair."""
import numpy as np
import pytest

import gicp_ref as G

F32, F64 = np.float32, np.float64
NAMES = ["kss_gicp_default_params", "kss_gicp_metric", "kss_gicp_sums", "kss_gicp_sums_dev", "kss_icp_gicp", "kss_icp_gicp_dev"]


def _bits(a):
    return np.ascontiguousarray(a, dtype=F64).view(np.uint64)


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def test_symbols_exported_and_listed(pkg):
    exported = set(pkg.exported_symbols())
    for n in NAMES:
        assert n in pkg.binding.SYMBOLS and n in exported, n
    for n in ("gicp_sums", "gicp_sums_dev", "icp_gicp", "icp_gicp_dev"):
        assert callable(getattr(pkg.Context, n)), n


def test_default_params(pkg):
    gp = pkg.gicp_params()
    assert _bits([gp.epsilon])[0] == _bits([1e-3])[0] and gp.normals_k == 20
    gp = pkg.gicp_params(epsilon=0.25, normals_k=12)
    assert gp.epsilon == 0.25 and gp.normals_k == 12
    with pytest.raises(AttributeError):
        pkg.gicp_params(overlap=0.5)
    assert pkg.load_library().kss_gicp_default_params(None) == -1


@pytest.mark.parametrize("eps", [1e-3, 1e-2, 1.0])
def test_metric_bit_for_bit(pkg, eps):
    rng = np.random.default_rng(11)
    nq = _unit(rng, 200).astype(F32)
    m = _unit(rng, 200)
    cases = [(nq[i], m[i]) for i in range(200)]
    cases += [(nq[i], s * nq[i].astype(F64)) for i in range(20) for s in (1.0, -1.0)]            # nq = +-m: the least det
    cases += [(np.array(a, F32), np.array(b, F64)) for a in np.eye(3) for b in np.eye(3)]       # axis normals: exact zeros
    for a, b in cases:
        got, ok = pkg.gicp_metric(a, b, eps)
        ref = G.metric_py(a, b, eps)
        assert ok and ref is not None
        assert np.array_equal(_bits(got), _bits(ref)), (a, b, eps, got, ref)
        # it is the inverse: C M = I to rounding at the condition 2 / eps
        e = 1.0 - eps
        a64 = a.astype(F64)
        Cm = 2.0 * np.eye(3) - e * (np.outer(a64, a64) + np.outer(b, b))
        Mm = np.array([[got[0], got[1], got[2]], [got[1], got[3], got[4]], [got[2], got[4], got[5]]])
        assert np.abs(Cm @ Mm - np.eye(3)).max() <= 1e-15 * (2.0 / eps) * 8
    # the vectorised restatement the GPU tests use is the same expression
    okv, Mv = G.metric(nq.astype(F64), m, eps)
    assert okv.all()
    for i in range(0, 200, 17):
        assert np.array_equal(_bits(Mv[i]), _bits(G.metric_py(nq[i], m[i], eps)))


def test_metric_epsilon_one_is_half_identity(pkg):
    rng = np.random.default_rng(12)
    for a, b in zip(_unit(rng, 10).astype(F32), _unit(rng, 10)):
        got, ok = pkg.gicp_metric(a, b, 1.0)
        assert ok and np.array_equal(got, [0.5, 0.0, 0.0, 0.5, 0.0, 0.5])


def test_metric_dropped_and_bad_arguments(pkg):
    nan, inf = float("nan"), float("inf")
    for a, b in (([nan, 0, 1], [0, 0, 1]), ([0, 0, 1], [0, nan, 1]), ([inf, 0, 0], [0, 0, 1]), ([0, 0, 1], [0, -inf, 0])):
        got, ok = pkg.gicp_metric(a, b, 1e-3)
        assert not ok and G.metric_py(a, b, 1e-3) is None
        assert np.array_equal(got, np.zeros(6))
    # normals that are not of unit length can make C indefinite: dropped, not solved
    got, ok = pkg.gicp_metric([0, 0, 2], [0, 0, 2], 1e-3)
    assert not ok and G.metric_py([0, 0, 2], [0, 0, 2], 1e-3) is None
    for eps in (0.0, -1.0, 2.0, nan):
        with pytest.raises(pkg.KssError) as e:
            pkg.gicp_metric([0, 0, 1], [0, 0, 1], eps)
        assert e.value.status == -1


def test_restatement_beats_point_to_point_on_disjoint_halves(pkg, O):
    """The GPU test's known-motion pair on the restatement alone: 2 x 4000 points of one bumpy surface, no point shared, 10
    degrees about (0.3, -0.5, 1), normals by 20-NN PCA on each cloud as it is passed in."""
    src, tgt, R_true, t_true = G.halves_pair(pkg.synth, 8, 4000, 10.0, axis=[0.3, -0.5, 1.0])
    assert not (src[:, None, 0] == tgt[None, :, 0]).any()
    sn = O.normals_pcl(src.astype(F64), 20).astype(F32)
    tn = O.normals_pcl(tgt.astype(F64), 20).astype(F32)
    ref = G.icp_gicp(O, src, sn, tgt, tn)
    eR, et = G.errors(ref["T"], R_true, t_true)
    p2p = O.icp(src, tgt, O.icp_params(max_iterations=200))
    pR, pt = G.errors(p2p["T"], R_true, t_true)
    print("gicp: %d passes, state %d, |R - R_true| %.2e, |t - t_true| %.2e;  point-to-point: %d passes, %.2e, %.2e" % (
        ref["iterations"], ref["state"], eR, et, p2p["iterations"], pR, pt))
    assert ref["converged"]
    assert eR <= 1e-3 and eR <= 0.25 * pR
