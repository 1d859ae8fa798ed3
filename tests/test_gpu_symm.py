"""Symmetric ICP on the device (kss_symm_sums, kss_icp_symm[_dev]) against the independent restatement in tests/symm_ref.py,
and its invariances: the NN engine and its tuning knobs, the signs of the normals, computed vs given normals, host vs device
pointers.  The pairs are two independent samplings of one surface (gicp_ref.halves_pair): no source point is a target point."""

import numpy as np
import pytest

import symm_ref as S

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == F64 else np.uint32)


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)


def _normals(ctx, cloud):
    return ctx.normals(cloud.astype(F64), 20).astype(F32)


def _same(a, b):
    assert b["iterations"] == a["iterations"] and b["state"] == a["state"] and b["converged"] == a["converged"]
    assert np.array_equal(_bits(b["trace_Tk"]), _bits(a["trace_Tk"]))
    assert np.array_equal(_bits(b["trace_sums"]), _bits(a["trace_sums"]))
    assert np.array_equal(_bits(b["T"]), _bits(a["T"]))
    assert _bits(np.array([b["fitness"]])) == _bits(np.array([a["fitness"]]))


@pytest.mark.parametrize("align", [1, 0])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 20000])
def test_symm_sums_match_restatement(pkg, ctx, n, align):
    """One lane, a wave's edges, a workgroup's edge, several workgroups with a grid-stride tail; 1e-12 * sum|term| per slot is the
    bound of the p2l and gicp sums tests."""
    rng = np.random.default_rng(n)
    nt = max(1, n // 2 + 7)
    src = rng.uniform(-1, 1, size=(n, 3)).astype(F32)
    tgt = rng.uniform(-1, 1, size=(nt, 3)).astype(F32)
    sn, tn = _unit(rng, n), _unit(rng, nt)
    tn[rng.random(nt) < 0.05] = np.nan        # non-finite normals on either side drop the correspondence
    tn[rng.random(nt) < 0.02, 1] = np.inf
    sn[rng.random(n) < 0.05] = np.nan
    sn[rng.random(n) < 0.02, 2] = -np.inf
    idx = rng.integers(0, nt, size=n).astype(np.int32)
    max_d2 = 1.5                              # part of the random pairs are farther apart
    Rn = pkg.synth.rot_axis_angle(rng.normal(size=3), rng.uniform(0.1, 3.0)).astype(F32)
    sp = pkg.symm_params(align_normals=align)
    got = ctx.symm_sums(src, sn, tgt, tn, idx, max_d2, Rn=Rn, sp=sp)
    ref, absc = S.sums(src, sn, tgt, tn, idx, max_d2, Rn=Rn, align=align)
    err = np.abs(got - ref) / np.maximum(absc, 1e-300)
    print("n %d align %d: kept %d of %d, max |got - ref| / sum|term| %.2e" % (n, align, int(got[0]), n, err.max()))
    assert got[0] == ref[0]
    assert np.all(np.abs(got - ref) <= 1e-12 * absc), err
    assert got[31] == 0.0
    again = ctx.symm_sums(src, sn, tgt, tn, idx, max_d2, Rn=Rn, sp=sp)
    assert np.array_equal(_bits(got), _bits(again))
    if n == 257:                              # no Rn is the identity
        a = ctx.symm_sums(src, sn, tgt, tn, idx, max_d2, sp=sp)
        b = ctx.symm_sums(src, sn, tgt, tn, idx, max_d2, Rn=np.eye(3), sp=sp)
        assert np.array_equal(_bits(a), _bits(b))
        ri, ai = S.sums(src, sn, tgt, tn, idx, max_d2, align=align)
        assert a[0] == ri[0] and np.all(np.abs(a - ri) <= 1e-12 * ai)


@pytest.mark.parametrize("seed,n,n_src,deg", [(1, 3000, None, 5.0), (2, 2500, 1800, 10.0), (3, 2000, None, 15.0)])
def test_icp_symm_matches_restatement(pkg, ctx, O, seed, n, n_src, deg):
    """test_gpu_p2l's tolerances (the measured spread is in DESIGN.md 2.16)."""
    src, tgt, _, _ = S.halves_pair(pkg.synth, seed, n, deg, n_src=n_src)
    sn, tn = _normals(ctx, src), _normals(ctx, tgt)
    got = ctx.icp_symm(src, tgt, sn, tn, params=ctx.icp_params(max_iterations=60), trace_cap=64)
    ref = S.icp_symm(O, src, sn, tgt, tn, max_iterations=60)
    print("pair %d: %d / %d passes, state %d / %d" % (seed, got["iterations"], ref["iterations"], got["state"], ref["state"]))
    assert got["iterations"] == ref["iterations"] >= 1
    assert got["state"] == ref["state"] and got["converged"] == ref["converged"]
    s0, r0 = got["trace_sums"][0], ref["trace_sums"][0]
    print("  |trace_Tk| %.2e  |T| %.2e  |fitness| %.2e  first sums %.2e" % (
        np.abs(got["trace_Tk"] - ref["trace_Tk"]).max(), np.abs(got["T"] - ref["T"]).max(), abs(got["fitness"] - ref["fitness"]),
        (np.abs(s0 - r0) / np.maximum(np.abs(r0), 1.0)).max()))
    assert np.abs(got["trace_Tk"] - ref["trace_Tk"]).max() <= 1e-6
    assert np.abs(got["T"] - ref["T"]).max() <= 5e-6
    assert abs(got["fitness"] - ref["fitness"]) <= 1e-9 * max(1.0, ref["fitness"])
    # the first pass sees the same correspondences: its sums agree to rounding
    assert s0[0] == r0[0]
    assert np.all(np.abs(s0 - r0) <= 1e-9 * np.maximum(np.abs(r0), 1.0))


def test_icp_symm_engines_and_knobs_bit_identical(pkg, ctx):
    src, tgt, _, _ = S.halves_pair(pkg.synth, 4, 4000, 12.0, n_src=3500)
    sn, tn = _normals(ctx, src), _normals(ctx, tgt)
    runs = []
    for kw in (dict(nn_mode=pkg.NN_BRUTE), dict(nn_mode=pkg.NN_GRID), dict(nn_mode=pkg.NN_AUTO),
               dict(nn_mode=pkg.NN_BRUTE, nn_sources_per_thread=1, nn_target_splits=3),
               dict(nn_mode=pkg.NN_BRUTE, nn_sources_per_thread=8, nn_target_splits=1)):
        runs.append(ctx.icp_symm(src, tgt, sn, tn, params=ctx.icp_params(max_iterations=40, **kw), trace_cap=64))
    assert runs[0]["iterations"] >= 2
    for b in runs[1:]:
        _same(runs[0], b)


def test_icp_symm_normal_signs_do_not_matter(pkg, ctx):
    src, tgt, _, _ = S.halves_pair(pkg.synth, 5, 3000, 8.0, n_src=2600)
    sn, tn = _normals(ctx, src), _normals(ctx, tgt)
    rng = np.random.default_rng(5)
    sf, tf = sn.copy(), tn.copy()
    sf[rng.random(len(sf)) < 0.5] *= F32(-1.0)
    tf[rng.random(len(tf)) < 0.3] *= F32(-1.0)
    assert not np.array_equal(sf, sn) and not np.array_equal(tf, tn)
    a = ctx.icp_symm(src, tgt, sn, tn, trace_cap=64)
    assert a["iterations"] >= 2
    _same(a, ctx.icp_symm(src, tgt, sf, tf, trace_cap=64))


def test_icp_symm_computed_normals_equal_given(pkg, ctx):
    src, tgt, _, _ = S.halves_pair(pkg.synth, 6, 3000, 8.0, n_src=2200)
    sn, tn = _normals(ctx, src), _normals(ctx, tgt)
    a = ctx.icp_symm(src, tgt, sn, tn, trace_cap=64)
    assert a["iterations"] >= 1
    for s_, t_ in ((None, tn), (sn, None), (None, None)):
        _same(a, ctx.icp_symm(src, tgt, s_, t_, trace_cap=64))
    # normals_k is read when a set is computed
    sn12, tn12 = (ctx.normals(x.astype(F64), 12).astype(F32) for x in (src, tgt))
    _same(ctx.icp_symm(src, tgt, sn12, tn12, trace_cap=64), ctx.icp_symm(src, tgt, None, None, sp=pkg.symm_params(normals_k=12), trace_cap=64))


def test_icp_symm_dev_matches_host(pkg, ctx):
    import torch
    src, tgt, _, _ = S.halves_pair(pkg.synth, 7, 3000, 10.0, n_src=2000)
    sn, tn = _normals(ctx, src), _normals(ctx, tgt)
    h = ctx.icp_symm(src, tgt, sn, tn)
    s, t, dsn, dtn = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (src, tgt, sn, tn))
    torch.cuda.synchronize()
    for d_s, d_t in ((dsn.data_ptr(), dtn.data_ptr()), (None, dtn.data_ptr()), (dsn.data_ptr(), None), (None, None)):
        r = ctx.icp_symm_dev(s.data_ptr(), len(src), d_s, t.data_ptr(), len(tgt), d_t, ctx.icp_params())
        assert r.iterations == h["iterations"] >= 1 and r.state == h["state"]
        assert np.array_equal(_bits(r.matrix()), _bits(h["T"]))
        assert r.fitness == h["fitness"]
    idx, _ = ctx.nn(src, tgt)
    di = torch.from_numpy(idx).cuda()
    torch.cuda.synchronize()
    a = ctx.symm_sums(src, sn, tgt, tn, idx)
    b = ctx.symm_sums_dev(s.data_ptr(), dsn.data_ptr(), t.data_ptr(), dtn.data_ptr(), di.data_ptr(), len(src), len(tgt))
    assert np.array_equal(_bits(a), _bits(b))


def test_icp_symm_recovers_known_motion(pkg, ctx):
    """test_icp_gicp_recovers_known_motion's pair: 2 x 4000 points, 10 degrees about (0.3, -0.5, 1); the f64 numpy prototype
    gives 9.6e-5 and 9.7e-5 in 3 passes."""
    src, tgt, R_true, t_true = S.halves_pair(pkg.synth, 8, 4000, 10.0, axis=[0.3, -0.5, 1.0])
    got = ctx.icp_symm(src, tgt)
    eR, et = S.errors(got["T"], R_true, t_true)
    print("%d passes, state %d, |R - R_true| %.2e, |t - t_true| %.2e" % (got["iterations"], got["state"], eR, et))
    assert got["converged"] and got["state"] in (2, 3, 4)
    assert eR <= 1e-3


def test_icp_symm_recovers_65_degrees_where_point_to_plane_fails(pkg, ctx):
    """2 x 2000 points, 65 degrees about (0.3, -0.5, 1): the restatement (tests/test_symm_host.py) converges in 7 passes at
    2.9e-4 where point-to-plane and generalized ICP end in a wrong minimum at 1.2."""
    src, tgt, R_true, t_true = S.halves_pair(pkg.synth, 8, 2000, 65.0, axis=[0.3, -0.5, 1.0])
    sn, tn = _normals(ctx, src), _normals(ctx, tgt)
    p = ctx.icp_params(max_iterations=100)
    got = ctx.icp_symm(src, tgt, sn, tn, params=p)
    eR, et = S.errors(got["T"], R_true, t_true)
    p2l = ctx.icp_p2l(src, tgt, tn, params=ctx.icp_params(max_iterations=100))
    pR, pt = S.errors(p2l["T"], R_true, t_true)
    print("symmetric: %d passes, state %d, |R - R_true| %.2e, |t - t_true| %.2e;  point-to-plane: %d passes, %.2e, %.2e" % (
        got["iterations"], got["state"], eR, et, p2l["iterations"], pR, pt))
    assert got["converged"] and got["state"] in (2, 3, 4)
    assert eR <= 1e-3
    assert pR >= 0.5


def test_icp_symm_planar_pair_is_degenerate(pkg, ctx):
    """test_icp_p2l_planar_target_degenerate's clouds with both sets of normals exactly (0, 0, 1): three columns of every v are
    exactly zero, the system is singular as point-to-plane's is."""
    g = np.linspace(-1, 1, 40)
    tgt = np.stack(np.meshgrid(g, g), -1).reshape(-1, 2)
    tgt = np.concatenate([tgt, np.zeros((len(tgt), 1))], 1).astype(F32)
    src = (tgt[::2] + np.array([0.01, -0.02, 0.05])).astype(F32)
    tn = np.tile(np.array([0, 0, 1], F32), (len(tgt), 1))
    sn = np.tile(np.array([0, 0, 1], F32), (len(src), 1))
    got = ctx.icp_symm(src, tgt, sn, tn)
    assert got["state"] == pkg.STATE_DEGENERATE and not got["converged"] and got["iterations"] == 0
    assert np.array_equal(got["T"], np.eye(4, dtype=F32))


def test_icp_symm_bad_arguments(pkg, ctx):
    src, tgt, _, _ = S.halves_pair(pkg.synth, 9, 2000, 5.0)
    sn, tn = _normals(ctx, src), _normals(ctx, tgt)
    got = ctx.icp_symm(src + np.float32(100.0), tgt, sn, tn)
    assert got["state"] == 5 and got["iterations"] == 0 and not got["converged"]
    assert np.array_equal(got["T"], np.eye(4, dtype=F32))
    p = ctx.icp_params()
    cb = pkg.binding.ALLREDUCE_FN(lambda user, values, n: 0)
    p.allreduce = cb
    with pytest.raises(pkg.KssError) as e:
        ctx.icp_symm(src, tgt, sn, tn, params=p)
    assert e.value.status == -1
    idx = np.zeros(len(src), np.int32)
    for al in (2, -1):
        with pytest.raises(pkg.KssError) as e:
            ctx.icp_symm(src, tgt, sn, tn, sp=pkg.symm_params(align_normals=al))
        assert e.value.status == -1
        with pytest.raises(pkg.KssError) as e:
            ctx.symm_sums(src, sn, tgt, tn, idx, sp=pkg.symm_params(align_normals=al))
        assert e.value.status == -1
    for k in (2, 65):                          # normals_k is checked where a set of normals has to be computed
        with pytest.raises(pkg.KssError) as e:
            ctx.icp_symm(src, tgt, None, tn, sp=pkg.symm_params(normals_k=k))
        assert e.value.status == -1
        with pytest.raises(pkg.KssError) as e:
            ctx.symm_sums(src, None, tgt, tn, idx, sp=pkg.symm_params(normals_k=k))
        assert e.value.status == -1
    ctx.icp_symm(src, tgt, sn, tn, sp=pkg.symm_params(normals_k=2))   # not read when both sets are given
