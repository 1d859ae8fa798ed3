"""Point-to-plane ICP on the device (kss_p2l_sums, kss_icp_p2l[_dev]) against the independent restatement in
tests/p2l_ref.py, and its invariances: the NN engine and its tuning knobs, computed vs given normals, host vs device
pointers."""

import numpy as np
import pytest

import p2l_ref as R

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == F64 else np.uint32)


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 100000])
def test_p2l_sums_match_restatement(ctx, n):
    rng = np.random.default_rng(n)
    nt = max(1, n // 2 + 7)
    src = rng.uniform(-1, 1, size=(n, 3)).astype(F32)
    tgt = rng.uniform(-1, 1, size=(nt, 3)).astype(F32)
    nrm = _unit(rng, nt)
    nrm[rng.random(nt) < 0.05] = np.nan       # non-finite normals drop the correspondence
    nrm[rng.random(nt) < 0.02, 1] = np.inf
    idx = rng.integers(0, nt, size=n).astype(np.int32)
    max_d2 = 1.5                              # part of the random pairs are farther apart
    got = ctx.p2l_sums(src, tgt, nrm, idx, max_d2)
    ref, absc = R.sums(src, tgt, nrm, idx, max_d2)
    assert got[0] == ref[0]
    assert np.all(np.abs(got - ref) <= 1e-12 * absc), np.abs(got - ref) / np.maximum(absc, 1e-300)
    assert got[31] == 0.0
    again = ctx.p2l_sums(src, tgt, nrm, idx, max_d2)
    assert np.array_equal(_bits(got), _bits(again))


def _bumpy(pkg, pair_id, n, deg, n_src=None, t=(0.02, -0.01, 0.03)):
    axis = pkg.synth.sphere(7000 + pair_id, 1)[0]
    return pkg.synth.make_pair(pair_id, n, R=pkg.synth.rot_axis_angle(axis, np.deg2rad(deg)), t=t, shape="bumpy", n_src=n_src)


def _normals(ctx, tgt):
    return ctx.normals(tgt.astype(F64), 20).astype(F32)


@pytest.mark.parametrize("pair_id,n,n_src,deg", [(1, 3000, None, 5.0), (2, 2500, 1800, 10.0), (3, 2000, 2600, 15.0)])
def test_icp_p2l_matches_restatement(pkg, ctx, O, pair_id, n, n_src, deg):
    src, tgt = _bumpy(pkg, pair_id, n, deg, n_src=n_src)
    nrm = _normals(ctx, tgt)
    got = ctx.icp_p2l(src, tgt, nrm, params=ctx.icp_params(max_iterations=60), trace_cap=64)
    ref = R.icp_p2l(O, src, tgt, nrm, max_iterations=60)
    assert got["iterations"] == ref["iterations"] >= 1
    assert got["state"] == ref["state"] and got["converged"] == ref["converged"]
    assert np.abs(got["trace_Tk"] - ref["trace_Tk"]).max() <= 1e-6
    assert np.abs(got["T"] - ref["T"]).max() <= 5e-6
    assert abs(got["fitness"] - ref["fitness"]) <= 1e-9 * max(1.0, ref["fitness"])
    # the first pass sees the same correspondences: its sums agree to rounding
    s0, r0 = got["trace_sums"][0], ref["trace_sums"][0]
    assert s0[0] == r0[0]
    assert np.all(np.abs(s0 - r0) <= 1e-9 * np.maximum(np.abs(r0), 1.0))


def test_icp_p2l_engines_and_knobs_bit_identical(pkg, ctx):
    src, tgt = _bumpy(pkg, 4, 4000, 12.0, n_src=3500)
    nrm = _normals(ctx, tgt)
    runs = []
    for kw in (dict(nn_mode=pkg.NN_BRUTE), dict(nn_mode=pkg.NN_GRID), dict(nn_mode=pkg.NN_AUTO),
               dict(nn_mode=pkg.NN_BRUTE, nn_sources_per_thread=1, nn_target_splits=3),
               dict(nn_mode=pkg.NN_BRUTE, nn_sources_per_thread=8, nn_target_splits=1)):
        runs.append(ctx.icp_p2l(src, tgt, nrm, params=ctx.icp_params(max_iterations=40, **kw), trace_cap=64))
    a = runs[0]
    assert a["iterations"] >= 2
    for b in runs[1:]:
        assert b["iterations"] == a["iterations"] and b["state"] == a["state"]
        assert np.array_equal(_bits(b["trace_Tk"]), _bits(a["trace_Tk"]))
        assert np.array_equal(_bits(b["trace_sums"]), _bits(a["trace_sums"]))
        assert np.array_equal(_bits(b["T"]), _bits(a["T"]))
        assert _bits(np.array([b["fitness"]])) == _bits(np.array([a["fitness"]]))


def test_icp_p2l_computed_normals_equal_given(pkg, ctx):
    src, tgt = _bumpy(pkg, 5, 3000, 8.0)
    nrm = _normals(ctx, tgt)
    a = ctx.icp_p2l(src, tgt, nrm, trace_cap=64, fitness_corr=True)
    b = ctx.icp_p2l(src, tgt, None, trace_cap=64, fitness_corr=True)
    assert a["iterations"] == b["iterations"] >= 1 and a["state"] == b["state"]
    assert np.array_equal(_bits(a["trace_Tk"]), _bits(b["trace_Tk"]))
    assert np.array_equal(_bits(a["T"]), _bits(b["T"]))
    assert a["fitness"] == b["fitness"]
    assert np.array_equal(a["fitness_idx"], b["fitness_idx"]) and np.array_equal(_bits(a["fitness_d2"]), _bits(b["fitness_d2"]))


def test_icp_p2l_dev_matches_host(pkg, ctx):
    import torch
    src, tgt = _bumpy(pkg, 6, 3000, 10.0, n_src=2000)
    nrm = _normals(ctx, tgt)
    p = ctx.icp_params()
    h = ctx.icp_p2l(src, tgt, nrm, params=p)
    s, t, nr = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (src, tgt, nrm))
    torch.cuda.synchronize()
    for d_n in (nr.data_ptr(), None):
        r = ctx.icp_p2l_dev(s.data_ptr(), len(src), t.data_ptr(), len(tgt), d_n, ctx.icp_params())
        assert r.iterations == h["iterations"] and r.state == h["state"]
        assert np.array_equal(_bits(r.matrix()), _bits(h["T"]))
        assert r.fitness == h["fitness"]


def test_icp_p2l_recovers_known_motion(pkg, ctx):
    Rt = pkg.synth.rot_axis_angle([0.3, -0.5, 1.0], np.deg2rad(10.0))
    t = np.array([0.02, -0.01, 0.03])
    src, tgt = pkg.synth.make_pair(8, 20000, R=Rt, t=t, shape="bumpy")
    got = ctx.icp_p2l(src, tgt)
    assert got["converged"] and got["state"] in (2, 3, 4)
    R_true, t_true = Rt.T, -Rt.T @ t          # source = Rt target + t  ->  T maps source onto target
    assert np.abs(got["T"][:3, :3] - R_true).max() <= 1e-3
    assert np.abs(got["T"][:3, 3] - t_true).max() <= 1e-3


def test_icp_p2l_planar_target_degenerate(pkg, ctx):
    g = np.linspace(-1, 1, 40)
    tgt = np.stack(np.meshgrid(g, g), -1).reshape(-1, 2)
    tgt = np.concatenate([tgt, np.zeros((len(tgt), 1))], 1).astype(F32)
    src = (tgt[::2] + np.array([0.01, -0.02, 0.05])).astype(F32)
    nrm = np.tile(np.array([0, 0, 1], F32), (len(tgt), 1))
    got = ctx.icp_p2l(src, tgt, nrm)
    assert got["state"] == pkg.STATE_DEGENERATE and not got["converged"] and got["iterations"] == 0
    assert np.isfinite(got["T"]).all()


def test_icp_p2l_far_apart_no_correspondences(pkg, ctx):
    src, tgt = _bumpy(pkg, 9, 2000, 5.0)
    got = ctx.icp_p2l(src + np.float32(100.0), tgt, _normals(ctx, tgt))
    assert got["state"] == 5 and got["iterations"] == 0 and not got["converged"]
    assert np.array_equal(got["T"], np.eye(4, dtype=F32))


def test_icp_p2l_rejects_allreduce(pkg, ctx):
    src, tgt = _bumpy(pkg, 10, 1000, 5.0)
    p = ctx.icp_params()
    cb = pkg.binding.ALLREDUCE_FN(lambda user, values, n: 0)
    p.allreduce = cb
    with pytest.raises(pkg.KssError) as e:
        ctx.icp_p2l(src, tgt, _normals(ctx, tgt), params=p)
    assert e.value.status == -1
