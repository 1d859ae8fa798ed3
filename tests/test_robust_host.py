"""Robust ICP, the parts that need no GPU: the exported symbols, the host-only helpers kss_robust_weight / kss_robust_scale2 /
kss_robust_default_params bit for bit against numpy (the host's division and sqrt are IEEE), and the restatement in
tests/robust_ref.py itself: with the L2 loss it is the oracle's ICP, with the three robust losses it recovers the two outlier
pairs that plain least squares does not -- the check that the GPU tests' inputs are fair."""
import numpy as np
import pytest

import robust_ref as RR

F32, F64 = np.float32, np.float64
NAMES = ["kss_robust_default_params", "kss_robust_weight", "kss_robust_scale2", "kss_robust_sums", "kss_robust_sums_dev",
         "kss_icp_robust", "kss_icp_robust_dev"]


def _bits(x):
    return int(np.array([x], F64).view(np.uint64)[0])


def test_symbols_exported_and_listed(pkg):
    exported = set(pkg.exported_symbols())
    for n in NAMES:
        assert n in pkg.binding.SYMBOLS and n in exported, n


def test_constants_match_restatement(pkg):
    assert [pkg.LOSS_L2, pkg.LOSS_HUBER, pkg.LOSS_TUKEY, pkg.LOSS_CAUCHY] == RR.LOSSES
    assert (pkg.METRIC_POINT, pkg.METRIC_PLANE) == (RR.POINT, RR.PLANE) and pkg.ROBUST_NINFO == RR.NINFO


@pytest.mark.parametrize("loss", RR.LOSSES)
def test_default_params(pkg, loss):
    for metric in (RR.POINT, RR.PLANE):
        rp = pkg.robust_params(loss, metric)
        assert (rp.loss, rp.metric) == (loss, metric)
        assert rp.scale == 0.0 and rp.min_scale == 0.0 and not rp.trace_robust
        assert _bits(rp.tune) == _bits(RR.TUNE[loss])
    for bad in ((-1, 0), (4, 0), (0, 2), (0, -1)):
        with pytest.raises(pkg.KssError) as e:
            pkg.robust_params(*bad)
        assert e.value.status == -1


def _xs(c2):
    c2 = F64(c2)
    return [0.0, 5e-324, float(np.nextafter(c2, F64(0.0))), float(c2), float(np.nextafter(c2, F64(np.inf))), float(F64(1e30) * c2),
            float("inf"), float("nan")]


@pytest.mark.parametrize("loss", RR.LOSSES)
def test_weight_bit_for_bit(pkg, loss):
    for c2 in (1.0, 0.0625, 3.7e-5, 1.0 / 3.0, 7.25e12, 2.0 ** -300):
        for x in _xs(c2) + [0.3 * c2, 0.999 * c2, 2.5 * c2, 17.0 * c2]:
            got, ref = pkg.robust_weight(loss, x, c2), float(RR.weight(loss, x, c2))
            assert _bits(got) == _bits(ref), (loss, x, c2, got, ref)
    # the c2 == 0 rule
    for x in (0.0, -0.0, 5e-324, 1.0, float("inf"), float("nan")):
        got = pkg.robust_weight(loss, x, 0.0)
        assert got == (1.0 if loss == RR.L2 or x == 0.0 else 0.0), (loss, x, got)
        assert _bits(got) == _bits(float(RR.weight(loss, x, 0.0)))
    # at the scale itself: Huber takes it with <=, Tukey drops it with <
    if loss == RR.HUBER:
        assert pkg.robust_weight(loss, 0.0625, 0.0625) == 1.0
    if loss == RR.TUKEY:
        assert pkg.robust_weight(loss, 0.0625, 0.0625) == 0.0
        assert pkg.robust_weight(loss, float(np.nextafter(F64(0.0625), F64(0.0))), 0.0625) > 0.0
    with pytest.raises(pkg.KssError):
        pkg.robust_weight(7, 1.0, 1.0)


def test_scale2_bit_for_bit(pkg):
    rng = np.random.default_rng(3)
    keys = [F32(0.0), F32(-0.0), F32(1e-45), F32(1.1754944e-38), F32(3.4e38), F32(0.37), F32(np.inf)]
    keys += list(rng.uniform(0.0, 2.0, 40).astype(F32))
    for metric in (RR.POINT, RR.PLANE):
        for tune in (1.345, 4.685, 2.385, 1.0, 1e-3):
            for min_scale in (0.0, 1e-3, 0.5):
                for key in keys:
                    got, ref = pkg.robust_scale2(metric, tune, key, min_scale), float(RR.scale2(metric, tune, key, min_scale))
                    assert _bits(got) == _bits(ref), (metric, tune, min_scale, key, got, ref)
    assert pkg.robust_scale2(RR.POINT, 1.345, F32(0.0), 0.25) == 0.0625      # the floor
    for bad in ((2, 1.0, 0.5, 0.0), (0, 0.0, 0.5, 0.0), (0, float("inf"), 0.5, 0.0), (0, float("nan"), 0.5, 0.0), (0, 1.0, -0.5, 0.0),
                (0, 1.0, float("nan"), 0.0), (0, 1.0, 0.5, -1.0)):
        with pytest.raises(pkg.KssError) as e:
            pkg.robust_scale2(*bad)
        assert e.value.status == -1


def test_outlier_pair_definition(pkg):
    S = pkg.synth
    src, tgt, R, t = S.make_outlier_pair(2, 4000, 10.0, 0.3)
    base_src, base_tgt = S.make_pair(2, 4000, R=S.rot_axis_angle(S.sphere(7002, 1)[0], np.deg2rad(10.0)), t=(0.02, -0.01, 0.03),
                                     shape="bumpy")
    k = 1200
    assert src.dtype == F32 and np.array_equal(tgt, base_tgt) and np.array_equal(src[k:], base_src[k:])
    u = np.stack([S.u01(9002, k, j * k) for j in range(3)], 1)
    assert np.array_equal(src[:k], (base_src[:k].astype(F64) + (u - 0.5) * 1.2).astype(F32))
    assert np.allclose(R @ R.T, np.eye(3), atol=1e-12) and np.array_equal(t, [0.02, -0.01, 0.03])


def _errors(T, R_true, t_true):
    return np.abs(T[:3, :3] - R_true).max(), np.abs(T[:3, 3] - t_true).max()


def test_restatement_l2_is_the_oracle_icp(pkg, O):
    src, tgt, _, _, _ = RR.pair(pkg, O, RR.PAIRS[0])
    ref = RR.reference(pkg, O, RR.PAIRS[0], RR.L2, RR.POINT)
    orc = O.icp(src, tgt, O.icp_params(max_iterations=200))
    assert ref["iterations"] == orc["iterations"] == 14
    # (the two sides add the same terms in different orders: the trimmed test's bound on T between two such loops)
    assert np.abs(orc["T"] - ref["T"]).max() <= 5e-6


@pytest.mark.parametrize("metric", [RR.POINT, RR.PLANE], ids=["point", "plane"])
@pytest.mark.parametrize("spec", RR.PAIRS, ids=lambda s: "pair%d" % s[0])
def test_restatement_recovers_where_l2_does_not(pkg, O, spec, metric):
    _, _, _, R_true, t_true = RR.pair(pkg, O, spec)
    for loss in (RR.HUBER, RR.TUKEY, RR.CAUCHY):
        ref = RR.reference(pkg, O, spec, loss, metric)
        eR, et = _errors(ref["T"], R_true, t_true)
        print("pair %d metric %d loss %d: %d passes, state %d, |R - R_true| %.2e, |t - t_true| %.2e" % (
            spec[0], metric, loss, ref["iterations"], ref["state"], eR, et))
        assert ref["converged"] and eR < 2e-3 and et < 2e-3
    l2 = RR.reference(pkg, O, spec, RR.L2, metric)
    eR, et = _errors(l2["T"], R_true, t_true)
    print("pair %d metric %d L2: %d passes, |R - R_true| %.2e, |t - t_true| %.2e" % (spec[0], metric, l2["iterations"], eR, et))
    assert max(eR, et) >= (1.3e-2 if metric == RR.PLANE else 5.5e-3)
