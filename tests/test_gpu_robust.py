"""Robust ICP on the device (kss_robust_sums[_dev], kss_icp_robust[_dev]) against the independent restatement in
tests/robust_ref.py: one pass over crafted correspondences (counts and scale exactly, sums to rounding), the loop on two
pairs with 30-40 % gross outliers for both metrics and the three losses, the L2 anchors to kss_icp_p2l and kss_icp_trimmed bit
for bit, the invariances of test_gpu_trim.py, and the endings."""

import numpy as np
import pytest

import robust_ref as RR

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
METRICS = [RR.POINT, RR.PLANE]
ROBUST = [RR.HUBER, RR.TUKEY, RR.CAUCHY]
SIZES = [1, 2, 63, 64, 65, 257, 4096, 100000]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == F64 else np.uint32)


def _rp(pkg, loss, metric, **kw):
    return pkg.robust_params(loss, metric, **kw)


# ---- one pass over crafted correspondences: (n, rng) -> (src, tgt, normals, idx, max_d2) ----
def _mixed(n, rng):
    """Random correspondences with every way of not being a candidate, and residuals that are exactly 0."""
    nt = n // 2 + 3
    tgt = rng.uniform(-1.0, 1.0, (nt, 3)).astype(F32)
    nrm = rng.normal(size=(nt, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F32)
    nrm[rng.random(nt) < 0.1, rng.integers(0, 3)] = np.nan             # targets without a finite normal
    idx = rng.integers(0, nt, n).astype(np.int32)
    src = (tgt[idx] + rng.normal(size=(n, 3)).astype(F32) * F32(0.1)).astype(F32)
    far = rng.random(n) < 0.15
    src[far] += F32(3.0)                                               # d2 above max_d2
    same = rng.random(n) < 0.1
    src[same] = tgt[idx[same]]                                         # d2 = 0 and r = 0
    bad = rng.random(n) < 0.1
    idx[bad] = rng.choice(np.array([-1, -7, nt, nt + 5, 2 ** 31 - 1], np.int64), int(bad.sum())).astype(np.int32)
    return src, tgt, nrm, idx, 1.5


def _lattice(n, rng, heights):
    """Targets on a lattice of multiples of 1/64 with the normal (0, 0, 1), sources straight above them at the given heights:
    d2 = h*h and r = -h exactly, in float."""
    nt = n // 2 + 3
    tgt = (rng.integers(-64, 65, (nt, 3)) / 64.0).astype(F32)
    nrm = np.tile(np.array([0, 0, 1], F32), (nt, 1))
    idx = rng.integers(0, nt, n).astype(np.int32)
    src = tgt[idx].copy()
    src[:, 2] += rng.choice(np.asarray(heights, F32), n)
    return src, tgt, nrm, idx, 1.5


def _all_equal(n, rng):
    """Every residual the same: the median is a tie, and a fixed scale of 0.25 equals every x."""
    return _lattice(n, rng, [0.25])


def _steps(n, rng):
    """Residuals 0, 0.25 and 0.5: with the fixed scale 0.25 a third of the x lie below c2, a third ON it, a third above."""
    return _lattice(n, rng, [0.0, 0.25, 0.5])


SETS = [_mixed, _all_equal, _steps]
SCALES = [dict(), dict(scale=0.25), dict(min_scale=0.2)]      # automatic, fixed, automatic with a floor


def _check_pass(got, ref):
    (gs, gi), (rs, ra, ri) = got, ref
    assert gi[0] == ri[0] and gi[3] == ri[3], (gi, ri)                                  # m, cnt
    assert _bits(gi[1:2])[0] == _bits(ri[1:2])[0], (gi, ri)                             # c2, bit pattern
    assert _bits(gi[2:3])[0] == _bits(gs[0:1])[0]
    ncol = len(rs)
    assert gs[ncol - 3] == ri[0] and gs[ncol - 1] == ri[3]
    assert np.all(np.abs(gs - rs) <= 1e-12 * ra), np.abs(gs - rs) / np.maximum(ra, 1e-300)


@pytest.mark.parametrize("gen", SETS, ids=lambda g: g.__name__.strip("_"))
@pytest.mark.parametrize("n", SIZES)
def test_robust_sums_match_restatement(pkg, ctx, n, gen):
    src, tgt, nrm, idx, max_d2 = gen(n, np.random.default_rng(n + 31 * SETS.index(gen)))
    d2 = RR.PR.dist2(src, tgt, np.clip(idx, 0, len(tgt) - 1))
    for metric in METRICS:
        nr = nrm if metric == RR.PLANE else None
        for loss in RR.LOSSES:
            for kw in SCALES:
                rp = _rp(pkg, loss, metric, **kw)
                got = ctx.robust_sums(src, tgt, nr, idx, max_d2, rp)
                ref = RR.one_pass(src, tgt, nr, idx, d2, max_d2, loss, metric, **kw)
                _check_pass(got, ref)
                again = ctx.robust_sums(src, tgt, nr, idx, max_d2, rp)
                assert np.array_equal(_bits(got[0]), _bits(again[0])) and np.array_equal(_bits(got[1]), _bits(again[1]))
                if loss == RR.L2:
                    assert got[0][0] == got[1][3] == got[1][0]                          # every candidate, weight 1
                if gen is not _mixed and kw.get("scale") and n >= 63:
                    # x == c2 exactly for the sources at height 0.25: Huber takes them (<=), Tukey drops them (<)
                    at = int((src[:, 2] - tgt[idx][:, 2] == F32(0.25)).sum())
                    below = int((src[:, 2] == tgt[idx][:, 2]).sum())
                    assert at > 0
                    if loss == RR.HUBER:
                        assert got[1][3] == n
                    if loss == RR.TUKEY:
                        assert got[1][3] == below


def test_robust_sums_dev_matches_host(pkg, ctx):
    import torch
    for n, gen in ((65, _mixed), (4096, _mixed), (4096, _steps)):
        src, tgt, nrm, idx, max_d2 = gen(n, np.random.default_rng(7 + n))
        s, t, nr, ix = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (src, tgt, nrm, idx))
        torch.cuda.synchronize()
        for metric in METRICS:
            for loss in RR.LOSSES:
                for kw in SCALES:
                    rp = _rp(pkg, loss, metric, **kw)
                    h = ctx.robust_sums(src, tgt, nrm if metric == RR.PLANE else None, idx, max_d2, rp)
                    d = ctx.robust_sums_dev(s.data_ptr(), t.data_ptr(), nr.data_ptr() if metric == RR.PLANE else None, ix.data_ptr(),
                                            n, len(tgt), max_d2, rp)
                    assert np.array_equal(_bits(h[0]), _bits(d[0])) and np.array_equal(_bits(h[1]), _bits(d[1]))


# ---- the loop ----
def _errors(T, R_true, t_true):
    return np.abs(T[:3, :3] - R_true).max(), np.abs(T[:3, 3] - t_true).max()


@pytest.mark.parametrize("loss", ROBUST, ids=["huber", "tukey", "cauchy"])
@pytest.mark.parametrize("metric", METRICS, ids=["point", "plane"])
@pytest.mark.parametrize("spec", RR.PAIRS, ids=lambda s: "pair%d" % s[0])
def test_icp_robust_matches_restatement_and_recovers(pkg, ctx, O, spec, metric, loss):
    src, tgt, nrm, R_true, t_true = RR.pair(pkg, O, spec)
    nr = nrm if metric == RR.PLANE else None
    got = ctx.icp_robust(src, tgt, nr, loss=loss, metric=metric, params=ctx.icp_params(max_iterations=200), trace_cap=256)
    ref = RR.reference(pkg, O, spec, loss, metric)
    eR, et = _errors(got["T"], R_true, t_true)
    print("pair %d metric %d loss %d: library %d it. state %d, restatement %d it. state %d, max|T - T_ref| %.2e, vs truth %.2e / %.2e" % (
        spec[0], metric, loss, got["iterations"], got["state"], ref["iterations"], ref["state"], np.abs(got["T"] - ref["T"]).max(), eR, et))
    assert got["iterations"] == ref["iterations"] >= 1
    assert got["state"] == ref["state"] and got["converged"] == ref["converged"]
    # pass 0 sees the same positions on both sides: counts and scale agree exactly
    g0, r0 = got["trace_robust"][0], ref["trace_robust"][0]
    assert g0[0] == r0[0] and g0[3] == r0[3]
    assert _bits(g0[1:2])[0] == _bits(r0[1:2])[0]
    s0, q0 = got["trace_sums"][0], ref["trace_sums"][0]
    assert np.all(np.abs(s0 - q0) <= 1e-9 * np.maximum(np.abs(q0), 1.0))
    # later passes through the transforms
    assert np.abs(got["trace_Tk"] - ref["trace_Tk"]).max() <= 1e-6
    assert np.abs(got["T"] - ref["T"]).max() <= 5e-6
    assert abs(got["fitness"] - ref["fitness"]) <= 1e-9 * max(1.0, ref["fitness"])
    assert np.array_equal(_bits(got["robust_info"]), _bits(got["trace_robust"][-1]))
    # recovery through the library: the yardstick's bar
    assert eR < 2e-3 and et < 2e-3


def test_plain_icp_misses_the_bar_on_pair3(pkg, ctx, O):
    src, tgt, _, R_true, t_true = RR.pair(pkg, O, RR.PAIRS[1])
    got = ctx.icp(src, tgt, params=ctx.icp_params(max_iterations=200))
    eR, et = _errors(got["T"], R_true, t_true)
    print("kss_icp on pair 3: %d it., vs truth %.2e / %.2e" % (got["iterations"], eR, et))
    assert max(eR, et) >= 2e-3


# ---- anchors: the L2 loss is the unweighted step, bit for bit ----
@pytest.mark.parametrize("spec", RR.PAIRS, ids=lambda s: "pair%d" % s[0])
def test_l2_plane_is_icp_p2l_bit_for_bit(pkg, ctx, O, spec):
    src, tgt, nrm, _, _ = RR.pair(pkg, O, spec)
    a = ctx.icp_p2l(src, tgt, nrm, params=ctx.icp_params(max_iterations=60), trace_cap=64)
    for kw in (dict(), dict(scale=0.05)):
        b = ctx.icp_robust(src, tgt, nrm, rp=_rp(pkg, RR.L2, RR.PLANE, **kw), params=ctx.icp_params(max_iterations=60), trace_cap=64)
        assert a["iterations"] == b["iterations"] >= 1 and a["state"] == b["state"] and a["converged"] == b["converged"]
        assert np.array_equal(_bits(a["T"]), _bits(b["T"]))
        assert np.array_equal(_bits(a["trace_Tk"]), _bits(b["trace_Tk"]))
        assert np.array_equal(_bits(a["trace_sums"][:, 0:29]), _bits(b["trace_sums"][:, 0:29]))
        assert np.array_equal(_bits(a["trace_sums"][:, 30]), _bits(b["trace_sums"][:, 30]))
        assert np.array_equal(b["trace_sums"][:, 0], b["trace_sums"][:, 31]) and np.array_equal(b["trace_sums"][:, 0], b["trace_robust"][:, 3])


@pytest.mark.parametrize("spec", RR.PAIRS, ids=lambda s: "pair%d" % s[0])
def test_l2_point_is_icp_trimmed_overlap_one_bit_for_bit(pkg, ctx, O, spec):
    src, tgt, _, _, _ = RR.pair(pkg, O, spec)
    a = ctx.icp_trimmed(src, tgt, None, overlap=1.0, metric=RR.POINT, params=ctx.icp_params(max_iterations=60), trace_cap=64)
    for kw in (dict(), dict(scale=0.05)):
        b = ctx.icp_robust(src, tgt, None, rp=_rp(pkg, RR.L2, RR.POINT, **kw), params=ctx.icp_params(max_iterations=60), trace_cap=64)
        assert a["iterations"] == b["iterations"] >= 1 and a["state"] == b["state"] and a["converged"] == b["converged"]
        assert np.array_equal(_bits(a["T"]), _bits(b["T"]))
        assert np.array_equal(_bits(a["trace_Tk"]), _bits(b["trace_Tk"]))
        assert np.array_equal(_bits(a["trace_sums"][:, 0:17]), _bits(b["trace_sums"][:, 0:17]))
        assert np.array_equal(b["trace_sums"][:, 0], b["trace_sums"][:, 19]) and np.array_equal(b["trace_sums"][:, 0], b["trace_robust"][:, 3])
        assert np.all(b["trace_sums"][:, 18] == 0.0)


# ---- invariances ----
@pytest.mark.parametrize("metric", METRICS, ids=["point", "plane"])
def test_icp_robust_engines_and_knobs_bit_identical(pkg, ctx, O, metric):
    src, tgt, nrm, _, _ = RR.pair(pkg, O, RR.PAIRS[0])
    nr = nrm if metric == RR.PLANE else None
    for rp in (_rp(pkg, RR.TUKEY, metric), _rp(pkg, RR.HUBER, metric, scale=0.02)):
        runs = []
        for kw in (dict(nn_mode=pkg.NN_BRUTE), dict(nn_mode=pkg.NN_GRID), dict(nn_mode=pkg.NN_AUTO),
                   dict(nn_mode=pkg.NN_BRUTE, nn_sources_per_thread=1, nn_target_splits=3),
                   dict(nn_mode=pkg.NN_BRUTE, nn_sources_per_thread=8, nn_target_splits=1)):
            runs.append(ctx.icp_robust(src, tgt, nr, rp=rp, params=ctx.icp_params(max_iterations=40, **kw), trace_cap=64))
        a = runs[0]
        assert a["iterations"] >= 2
        for b in runs[1:]:
            assert b["iterations"] == a["iterations"] and b["state"] == a["state"]
            assert np.array_equal(_bits(b["trace_Tk"]), _bits(a["trace_Tk"]))
            assert np.array_equal(_bits(b["trace_sums"]), _bits(a["trace_sums"]))
            assert np.array_equal(_bits(b["trace_robust"]), _bits(a["trace_robust"]))
            assert np.array_equal(_bits(b["T"]), _bits(a["T"]))
            # (the fitness is the NN engine's own sum: test_gpu_trim.py's bound between two summation orders)
            assert abs(b["fitness"] - a["fitness"]) <= 2.0 * len(src) * 2.0 ** -53 * a["fitness"]


def test_icp_robust_computed_normals_equal_given(pkg, ctx, O):
    src, tgt, _, _, _ = RR.pair(pkg, O, RR.PAIRS[1])
    nrm = ctx.normals(tgt.astype(F64), 20).astype(F32)
    rp = _rp(pkg, RR.CAUCHY, RR.PLANE)
    a = ctx.icp_robust(src, tgt, nrm, rp=rp, trace_cap=64)
    b = ctx.icp_robust(src, tgt, None, rp=rp, trace_cap=64)
    assert a["iterations"] == b["iterations"] >= 1 and a["state"] == b["state"]
    assert np.array_equal(_bits(a["trace_Tk"]), _bits(b["trace_Tk"]))
    assert np.array_equal(_bits(a["trace_robust"]), _bits(b["trace_robust"]))
    assert np.array_equal(_bits(a["T"]), _bits(b["T"]))
    assert a["fitness"] == b["fitness"]
    assert np.array_equal(_bits(a["robust_info"]), _bits(a["trace_robust"][-1]))


@pytest.mark.parametrize("metric", METRICS, ids=["point", "plane"])
def test_icp_robust_dev_matches_host(pkg, ctx, O, metric):
    import torch
    src, tgt, nrm, _, _ = RR.pair(pkg, O, RR.PAIRS[1])
    rp = _rp(pkg, RR.HUBER, metric)
    h = ctx.icp_robust(src, tgt, nrm if metric == RR.PLANE else None, rp=rp)
    s, t, nr = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (src, tgt, nrm))
    torch.cuda.synchronize()
    r, info = ctx.icp_robust_dev(s.data_ptr(), len(src), t.data_ptr(), len(tgt), nr.data_ptr() if metric == RR.PLANE else None,
                                 ctx.icp_params(), rp=rp)
    assert r.iterations == h["iterations"] and r.state == h["state"]
    assert np.array_equal(_bits(r.matrix()), _bits(h["T"]))
    assert r.fitness == h["fitness"]
    assert np.array_equal(_bits(info), _bits(h["robust_info"]))


# ---- endings ----
@pytest.mark.parametrize("metric", METRICS, ids=["point", "plane"])
def test_ending_tukey_tiny_scale_keeps_nothing(pkg, ctx, O, metric):
    src, tgt, nrm, _, _ = RR.pair(pkg, O, RR.PAIRS[1])
    got = ctx.icp_robust(src, tgt, nrm if metric == RR.PLANE else None, rp=_rp(pkg, RR.TUKEY, metric, scale=1e-30))
    assert got["state"] == 5 and got["iterations"] == 0 and not got["converged"]
    assert got["robust_info"][0] > 0.9 * len(src) and got["robust_info"][3] < 3 and got["robust_info"][1] == 1e-30 * 1e-30
    assert np.array_equal(got["T"], np.eye(4, dtype=F32))


@pytest.mark.parametrize("metric", METRICS, ids=["point", "plane"])
def test_ending_no_candidate(pkg, ctx, O, metric):
    src, tgt, nrm, _, _ = RR.pair(pkg, O, RR.PAIRS[1])
    got = ctx.icp_robust(src, tgt, nrm if metric == RR.PLANE else None, loss=RR.HUBER, metric=metric,
                         params=ctx.icp_params(max_corr_dist=1e-9))
    assert got["state"] == 5 and got["iterations"] == 0 and not got["converged"]
    assert np.array_equal(got["robust_info"], np.zeros(4))
    assert np.array_equal(got["T"], np.eye(4, dtype=F32))


def test_ending_planar_target_degenerate(pkg, ctx):
    g = np.linspace(-1, 1, 40)
    tgt = np.stack(np.meshgrid(g, g), -1).reshape(-1, 2)
    tgt = np.concatenate([tgt, np.zeros((len(tgt), 1))], 1).astype(F32)
    src = (tgt[::2] + np.array([0.01, -0.02, 0.05])).astype(F32)
    nrm = np.tile(np.array([0, 0, 1], F32), (len(tgt), 1))
    for loss in ROBUST:
        got = ctx.icp_robust(src, tgt, nrm, loss=loss, metric=RR.PLANE)
        assert got["state"] == pkg.STATE_DEGENERATE and not got["converged"] and got["iterations"] == 0
        assert np.isfinite(got["T"]).all()


def test_ending_argument_errors(pkg, ctx, O):
    src, tgt, nrm, _, _ = RR.pair(pkg, O, RR.PAIRS[1])
    idx = np.zeros(len(src), np.int32)

    def both(rp, normals):
        for call in (lambda: ctx.icp_robust(src, tgt, normals, rp=rp), lambda: ctx.robust_sums(src, tgt, normals, idx, 1.0, rp)):
            with pytest.raises(pkg.KssError) as e:
                call()
            assert e.value.status == -1

    nan, inf = float("nan"), float("inf")
    for field, values in (("loss", (-1, 4)), ("metric", (-1, 2)), ("scale", (-0.5, inf, nan)), ("tune", (0.0, -1.0, inf, nan)),
                          ("min_scale", (-0.5,))):
        for v in values:
            rp = pkg.robust_params(RR.HUBER, RR.POINT)
            setattr(rp, field, v)
            both(rp, None)
    both(pkg.robust_params(RR.HUBER, RR.POINT), nrm)                   # normals with the point metric
    p = ctx.icp_params()
    p.allreduce = pkg.binding.ALLREDUCE_FN(lambda user, values, n: 0)
    for metric in METRICS:
        with pytest.raises(pkg.KssError) as e:
            ctx.icp_robust(src, tgt, nrm if metric == RR.PLANE else None, loss=RR.HUBER, metric=metric, params=p)
        assert e.value.status == -1
    # the context still works
    got = ctx.icp_robust(src, tgt, None, loss=RR.HUBER, metric=RR.POINT)
    assert got["iterations"] >= 1
