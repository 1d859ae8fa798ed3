"""Robust symmetric ICP on the device (kss_symm_robust_sums, kss_icp_symm_robust[_dev]) against the independent
restatement in tests/symm_robust_ref.py: the sums and the scale edges, KSS_LOSS_L2 against kss_icp_symm, the loop, its
invariances, the two headline scenes and the argument checks."""

import numpy as np
import pytest

import robust_ref as RR
import symm_ref as S
import symm_robust_ref as SR

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SHARED = list(range(29)) + [30]          # the slots kss_icp_symm and the L2 form share


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == F64 else np.uint32)


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)


def _normals(ctx, cloud):
    return ctx.normals(cloud.astype(F64), 20).astype(F32)


def _rp(pkg, loss, **kw):
    return pkg.robust_params(loss, RR.PLANE, **kw)


def _same(a, b, ns):
    assert b["iterations"] == a["iterations"] and b["state"] == a["state"] and b["converged"] == a["converged"]
    assert np.array_equal(_bits(b["trace_Tk"]), _bits(a["trace_Tk"]))
    assert np.array_equal(_bits(b["trace_sums"]), _bits(a["trace_sums"]))
    assert np.array_equal(_bits(b["trace_robust"]), _bits(a["trace_robust"]))
    assert np.array_equal(_bits(b["robust_info"]), _bits(a["robust_info"]))
    assert np.array_equal(_bits(b["T"]), _bits(a["T"]))
    # (the fitness is the NN engine's own sum: the bound between two summation orders)
    assert abs(b["fitness"] - a["fitness"]) <= 2.0 * ns * 2.0 ** -53 * a["fitness"]


# ---- 1. sums against the restatement ----
_INPUTS = {}


def _inputs(pkg, n):
    """The inputs of test_symm_sums_match_restatement (tests/test_gpu_symm.py), built once per n."""
    if n not in _INPUTS:
        rng = np.random.default_rng(n)
        nt = max(1, n // 2 + 7)
        src = rng.uniform(-1, 1, size=(n, 3)).astype(F32)
        tgt = rng.uniform(-1, 1, size=(nt, 3)).astype(F32)
        sn, tn = _unit(rng, n), _unit(rng, nt)
        tn[rng.random(nt) < 0.05] = np.nan
        tn[rng.random(nt) < 0.02, 1] = np.inf
        sn[rng.random(n) < 0.05] = np.nan
        sn[rng.random(n) < 0.02, 2] = -np.inf
        idx = rng.integers(0, nt, size=n).astype(np.int32)
        Rn = pkg.synth.rot_axis_angle(rng.normal(size=3), rng.uniform(0.1, 3.0)).astype(F32)
        _INPUTS[n] = (src, sn, tgt, tn, idx, Rn)
    return _INPUTS[n]


@pytest.mark.parametrize("align", [1, 0])
@pytest.mark.parametrize("scale", [0.05, 0.0], ids=["fixed", "auto"])
@pytest.mark.parametrize("loss", RR.LOSSES, ids=["l2", "huber", "tukey", "cauchy"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 20000])
def test_sums_match_restatement(pkg, ctx, n, loss, scale, align):
    """One lane, a wave's edges, a workgroup's edge, several workgroups with a grid-stride tail.  The counts and c2 are exact; every
    slot within 1e-12 * sum|term|, the bound of the symmetric and the robust sums tests."""
    src, sn, tgt, tn, idx, Rn = _inputs(pkg, n)
    max_d2 = 1.5
    sp = pkg.symm_params(align_normals=align)
    rp = _rp(pkg, loss, scale=scale)
    got, info = ctx.symm_robust_sums(src, sn, tgt, tn, idx, max_d2, Rn=Rn, sp=sp, rp=rp)
    ref, absc, rinfo, _ = SR.one_pass(src, sn, tgt, tn, idx, S.P.dist2(src, tgt, idx), max_d2, loss, Rn, align, scale)
    err = np.abs(got - ref) / np.maximum(absc, 1e-300)
    print("n %d loss %d scale %g align %d: m %d cnt %d c2 %.17g, max |got - ref| / sum|term| %.2e" % (
        n, loss, scale, align, int(info[0]), int(info[3]), info[1], err.max()))
    assert info[0] == rinfo[0] and info[3] == rinfo[3]
    assert got[29] == ref[29] == info[0] and got[31] == ref[31] == info[3]
    assert _bits(info[1:2])[0] == _bits(rinfo[1:2])[0]
    assert info[2] == got[0]
    assert np.all(np.abs(got - ref) <= 1e-12 * absc), err
    again, info2 = ctx.symm_robust_sums(src, sn, tgt, tn, idx, max_d2, Rn=Rn, sp=sp, rp=rp)
    assert np.array_equal(_bits(got), _bits(again)) and np.array_equal(_bits(info), _bits(info2))


# ---- 2. scale edges ----
def _edge_inputs(pkg):
    src, sn, tgt, tn, idx, Rn = _inputs(pkg, 257)
    sn, tn = np.nan_to_num(sn, nan=0.5, posinf=0.5, neginf=-0.5), np.nan_to_num(tn, nan=0.5, posinf=0.5, neginf=-0.5)
    return src, sn, tgt, tn, idx, Rn


def test_scale_edge_no_candidate(pkg, ctx):
    """max_d2 = 0 and no source on its target: m = 0, c2 = 0, the record all zero."""
    src, sn, tgt, tn, idx, Rn = _edge_inputs(pkg)
    assert np.all(S.P.dist2(src, tgt, idx) > 0)
    for loss in RR.LOSSES:
        got, info = ctx.symm_robust_sums(src, sn, tgt, tn, idx, 0.0, Rn=Rn, rp=_rp(pkg, loss))
        assert np.array_equal(got, np.zeros(32)) and np.array_equal(info, np.zeros(4))


@pytest.mark.parametrize("min_scale", [0.0, 1e-3])
def test_scale_edge_median_zero(pkg, ctx, min_scale):
    """More than half of the sources exactly on their targets: the median key is 0.  Without a floor c2 = 0 and exactly the x == 0
    candidates are kept; with min_scale = 1e-3, c2 = 1e-6 bit for bit."""
    src, sn, tgt, tn, idx, Rn = _edge_inputs(pkg)
    src = src.copy()
    on = np.arange(len(src)) % 5 < 3                        # 155 of 257
    src[on] = tgt[idx[on]]
    d2 = S.P.dist2(src, tgt, idx)
    for loss in (RR.HUBER, RR.TUKEY, RR.CAUCHY):
        got, info = ctx.symm_robust_sums(src, sn, tgt, tn, idx, 1.5, Rn=Rn, rp=_rp(pkg, loss, min_scale=min_scale))
        ref, absc, rinfo, keys = SR.one_pass(src, sn, tgt, tn, idx, d2, 1.5, loss, Rn, 1, 0.0, None, min_scale)
        assert info[0] == rinfo[0] >= on.sum() and np.sort(keys[~np.isnan(keys)])[int(np.ceil(0.5 * info[0])) - 1] == 0.0
        if min_scale == 0.0:
            assert info[1] == 0.0
            assert info[3] == rinfo[3] == int((keys == 0.0).sum())
            assert got[30] == 0.0 and np.all(got[22:28] == 0.0)
        else:
            assert _bits(info[1:2])[0] == _bits(np.array([F64(1e-3) * F64(1e-3)]))[0]
            assert info[3] == rinfo[3]
        assert np.all(np.abs(got - ref) <= 1e-12 * absc)


def test_scale_edge_tukey_tiny_scale_keeps_nothing(pkg, ctx):
    src, tgt, _, _ = SR.halves_pair(pkg.synth, 9, 257, 5.0)
    sn, tn = _normals(ctx, src), _normals(ctx, tgt)
    got = ctx.icp_symm_robust(src, tgt, sn, tn, rp=_rp(pkg, RR.TUKEY, scale=1e-30))
    assert got["state"] == 5 and got["iterations"] == 0 and not got["converged"]
    assert got["robust_info"][0] > 0 and got["robust_info"][3] == 0 and got["robust_info"][1] == 1e-30 * 1e-30
    assert np.array_equal(got["T"], np.eye(4, dtype=F32))


# ---- 3. KSS_LOSS_L2 is kss_icp_symm bit for bit ----
@pytest.mark.parametrize("seed,n,n_src,deg", [(1, 3000, None, 5.0), (2, 2500, 1800, 10.0)])
def test_l2_is_icp_symm_bit_for_bit(pkg, ctx, seed, n, n_src, deg):
    src, tgt, _, _ = SR.halves_pair(pkg.synth, seed, n, deg, n_src=n_src)
    sn, tn = _normals(ctx, src), _normals(ctx, tgt)
    a = ctx.icp_symm(src, tgt, sn, tn, params=ctx.icp_params(max_iterations=60), trace_cap=64)
    assert a["iterations"] >= 2
    for rp in (_rp(pkg, RR.L2, scale=0.05), _rp(pkg, RR.L2)):
        b = ctx.icp_symm_robust(src, tgt, sn, tn, rp=rp, params=ctx.icp_params(max_iterations=60), trace_cap=64)
        assert b["iterations"] == a["iterations"] and b["state"] == a["state"] and b["converged"] == a["converged"]
        assert np.array_equal(_bits(b["T"]), _bits(a["T"]))
        assert np.array_equal(_bits(b["trace_Tk"]), _bits(a["trace_Tk"]))
        assert np.array_equal(_bits(b["trace_sums"][:, SHARED]), _bits(a["trace_sums"][:, SHARED]))
        assert _bits(np.array([b["last_mse"]]))[0] == _bits(np.array([a["last_mse"]]))[0]
        assert _bits(np.array([b["fitness"]]))[0] == _bits(np.array([a["fitness"]]))[0]
        assert np.array_equal(b["trace_sums"][:, 29], a["trace_sums"][:, 0])       # m = cnt = the symmetric kept count
        assert np.array_equal(b["trace_sums"][:, 31], a["trace_sums"][:, 0])


# ---- 4. the loop against the restatement ----
def _loop_pair(pkg, which):
    if which == "A":
        return SR.scene_a(pkg.synth)
    src, tgt, R_true, t_true = SR.halves_pair(pkg.synth, 2, 2500, 10.0, n_src=1800)
    return SR.outliers(pkg.synth, src, 2, 0.3), tgt, R_true, t_true


@pytest.mark.parametrize("loss", [RR.TUKEY, RR.HUBER], ids=["tukey", "huber"])
@pytest.mark.parametrize("which", ["A", "halves2"])
def test_icp_matches_restatement(pkg, ctx, O, which, loss):
    """The tolerances of test_gpu_symm.py and test_gpu_robust.py."""
    src, tgt, _, _ = _loop_pair(pkg, which)
    sn, tn = _normals(ctx, src), _normals(ctx, tgt)
    got = ctx.icp_symm_robust(src, tgt, sn, tn, rp=_rp(pkg, loss), params=ctx.icp_params(max_iterations=100), trace_cap=128)
    ref = SR.icp_symm_robust(O, src, sn, tgt, tn, loss, max_iterations=100)
    s0, r0 = got["trace_sums"][0], ref["trace_sums"][0]
    print("%s loss %d: %d / %d passes, state %d / %d, |trace_Tk| %.2e  |T| %.2e  |fitness| %.2e  first sums %.2e" % (
        which, loss, got["iterations"], ref["iterations"], got["state"], ref["state"],
        np.abs(got["trace_Tk"] - ref["trace_Tk"]).max() if got["iterations"] == ref["iterations"] else -1.0,
        np.abs(got["T"] - ref["T"]).max(), abs(got["fitness"] - ref["fitness"]), (np.abs(s0 - r0) / np.maximum(np.abs(r0), 1.0)).max()))
    assert got["iterations"] == ref["iterations"] >= 1
    assert got["state"] == ref["state"] and got["converged"] == ref["converged"]
    assert np.abs(got["trace_Tk"] - ref["trace_Tk"]).max() <= 1e-6
    assert np.abs(got["T"] - ref["T"]).max() <= 5e-6
    assert abs(got["fitness"] - ref["fitness"]) <= 1e-9 * max(1.0, ref["fitness"])
    i0, j0 = got["trace_robust"][0], ref["trace_robust"][0]
    assert i0[0] == j0[0] and i0[3] == j0[3]
    assert _bits(i0[1:2])[0] == _bits(j0[1:2])[0]
    assert np.all(np.abs(s0 - r0) <= 1e-9 * np.maximum(np.abs(r0), 1.0))
    assert np.array_equal(_bits(got["robust_info"]), _bits(got["trace_robust"][-1]))


# ---- 5. invariances, bit for bit ----
def test_engines_and_knobs_bit_identical(pkg, ctx):
    src, tgt, _, _ = SR.halves_pair(pkg.synth, 4, 4000, 12.0, n_src=3500)
    src = SR.outliers(pkg.synth, src, 4, 0.2)
    sn, tn = _normals(ctx, src), _normals(ctx, tgt)
    for rp in (_rp(pkg, RR.TUKEY), _rp(pkg, RR.HUBER, scale=0.04)):
        runs = []
        for kw in (dict(nn_mode=pkg.NN_BRUTE), dict(nn_mode=pkg.NN_GRID), dict(nn_mode=pkg.NN_AUTO),
                   dict(nn_mode=pkg.NN_BRUTE, nn_sources_per_thread=1, nn_target_splits=3),
                   dict(nn_mode=pkg.NN_BRUTE, nn_sources_per_thread=8, nn_target_splits=1)):
            runs.append(ctx.icp_symm_robust(src, tgt, sn, tn, rp=rp, params=ctx.icp_params(max_iterations=40, **kw), trace_cap=64))
        assert runs[0]["iterations"] >= 2
        for b in runs[1:]:
            _same(runs[0], b, len(src))


def test_normal_signs_do_not_matter(pkg, ctx):
    src, tgt, _, _ = SR.halves_pair(pkg.synth, 5, 3000, 8.0, n_src=2600)
    src = SR.outliers(pkg.synth, src, 5, 0.2)
    sn, tn = _normals(ctx, src), _normals(ctx, tgt)
    rng = np.random.default_rng(5)
    sf, tf = sn.copy(), tn.copy()
    sf[rng.random(len(sf)) < 0.5] *= F32(-1.0)
    tf[rng.random(len(tf)) < 0.3] *= F32(-1.0)
    assert not np.array_equal(sf, sn) and not np.array_equal(tf, tn)
    for rp in (_rp(pkg, RR.TUKEY), _rp(pkg, RR.CAUCHY, scale=0.04)):
        a = ctx.icp_symm_robust(src, tgt, sn, tn, rp=rp, trace_cap=64)
        assert a["iterations"] >= 2
        b = ctx.icp_symm_robust(src, tgt, sf, tf, rp=rp, trace_cap=64)
        _same(a, b, len(src))
        assert _bits(np.array([b["fitness"]]))[0] == _bits(np.array([a["fitness"]]))[0]
    idx, _ = ctx.nn(src, tgt)
    a = ctx.symm_robust_sums(src, sn, tgt, tn, idx, rp=_rp(pkg, RR.TUKEY))
    b = ctx.symm_robust_sums(src, sf, tgt, tf, idx, rp=_rp(pkg, RR.TUKEY))
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))


def test_computed_normals_equal_given(pkg, ctx):
    src, tgt, _, _ = SR.halves_pair(pkg.synth, 6, 3000, 8.0, n_src=2200)
    src = SR.outliers(pkg.synth, src, 6, 0.2)
    sn, tn = _normals(ctx, src), _normals(ctx, tgt)
    rp = _rp(pkg, RR.TUKEY)
    a = ctx.icp_symm_robust(src, tgt, sn, tn, rp=rp, trace_cap=64)
    assert a["iterations"] >= 1
    for s_, t_ in ((None, tn), (sn, None), (None, None)):
        b = ctx.icp_symm_robust(src, tgt, s_, t_, rp=rp, trace_cap=64)
        _same(a, b, len(src))
        assert b["fitness"] == a["fitness"]


def test_dev_matches_host(pkg, ctx):
    import torch
    src, tgt, _, _ = SR.halves_pair(pkg.synth, 7, 3000, 10.0, n_src=2000)
    src = SR.outliers(pkg.synth, src, 7, 0.2)
    sn, tn = _normals(ctx, src), _normals(ctx, tgt)
    s, t, dsn, dtn = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (src, tgt, sn, tn))
    idx, _ = ctx.nn(src, tgt)
    di = torch.from_numpy(idx).cuda()
    torch.cuda.synchronize()
    for rp in (_rp(pkg, RR.TUKEY), _rp(pkg, RR.HUBER, scale=0.04)):
        h = ctx.icp_symm_robust(src, tgt, sn, tn, rp=rp)
        for d_s, d_t in ((dsn.data_ptr(), dtn.data_ptr()), (None, None)):
            r, info = ctx.icp_symm_robust_dev(s.data_ptr(), len(src), d_s, t.data_ptr(), len(tgt), d_t, ctx.icp_params(), rp=rp)
            assert r.iterations == h["iterations"] >= 1 and r.state == h["state"]
            assert np.array_equal(_bits(r.matrix()), _bits(h["T"]))
            assert r.fitness == h["fitness"]
            assert np.array_equal(_bits(info), _bits(h["robust_info"]))
        a = ctx.symm_robust_sums(src, sn, tgt, tn, idx, rp=rp)
        b = ctx.symm_robust_sums_dev(s.data_ptr(), dsn.data_ptr(), t.data_ptr(), dtn.data_ptr(), di.data_ptr(), len(src), len(tgt), rp=rp)
        assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))


# ---- 6. the headline ----
@pytest.mark.parametrize("name,bar", [("A", 3e-3), ("B", 2e-2)])
def test_only_the_combination_registers_the_scene(pkg, ctx, O, name, bar):
    """tests/test_symm_robust_host.py's conditions on the device: max_iterations = 100, the library's normals at k = 20 on the
    clouds as given.  The restatement gives Tukey 3.3e-4 / 4.2e-4 and Cauchy 3.5e-4 / 3.0e-4 (A / B), plain symmetric 8.3e-3 /
    7.6e-2, Tukey point-to-plane 1.2 / 1.2."""
    src, tgt, _, _, R_true, t_true = SR.scene(pkg, O, name)
    sn, tn = _normals(ctx, src), _normals(ctx, tgt)
    p = dict(max_iterations=100)
    for loss in (RR.TUKEY, RR.CAUCHY):
        got = ctx.icp_symm_robust(src, tgt, sn, tn, rp=_rp(pkg, loss), params=ctx.icp_params(**p))
        eR, et = SR.errors(got["T"], R_true, t_true)
        print("scene %s loss %d: %d passes, state %d, |R - R_true| %.2e, |t - t_true| %.2e" % (name, loss, got["iterations"], got["state"], eR, et))
        assert got["converged"] and got["state"] in (2, 3, 4)
        assert eR <= 1e-3
    hub = ctx.icp_symm_robust(src, tgt, sn, tn, rp=_rp(pkg, RR.HUBER), params=ctx.icp_params(**p))
    plain = ctx.icp_symm(src, tgt, sn, tn, params=ctx.icp_params(**p))
    p2l = ctx.icp_robust(src, tgt, tn, rp=_rp(pkg, RR.TUKEY), params=ctx.icp_params(**p))
    eH, eS, eP = (SR.errors(x["T"], R_true, t_true)[0] for x in (hub, plain, p2l))
    print("scene %s: Huber symmetric %.2e in %d, plain symmetric %.2e in %d, Tukey point-to-plane %.2e in %d" % (
        name, eH, hub["iterations"], eS, plain["iterations"], eP, p2l["iterations"]))
    assert eS >= bar
    assert eP >= 0.5


# ---- 7. arguments ----
def test_bad_arguments(pkg, ctx):
    src, tgt, _, _ = SR.halves_pair(pkg.synth, 9, 2000, 5.0)
    sn, tn = _normals(ctx, src), _normals(ctx, tgt)
    idx = np.zeros(len(src), np.int32)

    def refused(call):
        with pytest.raises(pkg.KssError) as e:
            call()
        assert e.value.status == -1

    def both(rp=None, sp=None, s_=sn):
        rp = rp if rp is not None else _rp(pkg, RR.TUKEY)
        refused(lambda: ctx.icp_symm_robust(src, tgt, s_, tn, sp=sp, rp=rp))
        refused(lambda: ctx.symm_robust_sums(src, s_, tgt, tn, idx, sp=sp, rp=rp))

    nan, inf = float("nan"), float("inf")
    both(rp=pkg.robust_params(RR.TUKEY, RR.POINT))
    for field, values in (("loss", (-1, 4)), ("metric", (-1, 2)), ("scale", (-0.5, inf, nan)), ("tune", (0.0, -1.0, inf, nan)),
                          ("min_scale", (-0.5,))):
        for v in values:
            rp = _rp(pkg, RR.TUKEY)
            setattr(rp, field, v)
            both(rp=rp)
    for al in (2, -1):
        both(sp=pkg.symm_params(align_normals=al))
    for k in (2, 65):                          # normals_k is checked where a set of normals has to be computed
        both(sp=pkg.symm_params(normals_k=k), s_=None)
    p = ctx.icp_params()
    p.allreduce = pkg.binding.ALLREDUCE_FN(lambda user, values, n: 0)
    refused(lambda: ctx.icp_symm_robust(src, tgt, sn, tn, rp=_rp(pkg, RR.TUKEY), params=p))
    # the context still works, normals_k is not read when both sets are given, and the batched forms are what they were: a
    # batch of one pair is the single-pair call
    got = ctx.icp_symm_robust(src, tgt, sn, tn, sp=pkg.symm_params(normals_k=2), rp=_rp(pkg, RR.TUKEY))
    assert got["iterations"] >= 1
    so, to = [0, len(src)], [0, len(tgt)]
    res, _ = ctx.icp_symm_batch(src, so, tgt, to, sn, tn)
    assert np.array_equal(_bits(res[0].matrix()), _bits(ctx.icp_symm(src, tgt, sn, tn)["T"]))
    res, info, _ = ctx.icp_robust_batch(src, so, tgt, to, tn, rp=_rp(pkg, RR.TUKEY))
    one = ctx.icp_robust(src, tgt, tn, rp=_rp(pkg, RR.TUKEY))
    assert np.array_equal(_bits(res[0].matrix()), _bits(one["T"])) and np.array_equal(_bits(info[0]), _bits(one["robust_info"]))
