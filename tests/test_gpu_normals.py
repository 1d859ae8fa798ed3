"""The surface-normal kernel (normals_kernel behind kss_normals, cloud_normals_dev and batch_normals_dev) point by point against
tests/normals_ref.py: the smallest eigenvector of the float covariance from a float64 eigen solve, with a bound per point that
grows with the point's own conditioning.  Every input is also run through the oracle on the CPU by
tests/test_normals_host.py, which fixes the constant C and the judged shares; nothing here is measured on the device."""

import numpy as np
import pytest

import gicp_ref as G
import normals_ref as N

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == F64 else np.uint32)


@pytest.fixture(scope="module")
def ref(pkg, O):
    return N.reference(pkg.synth, O)


@pytest.mark.parametrize("name", N.NAMES)
def test_normals_meet_every_rule(ctx, ref, name):
    """Rules (a) .. (d) on the device's normals, the device against the oracle within 2 C B on the rows judged and finite in
    both, and bit for bit on the rows whose normal does not depend on the trigonometric roots (rule (e))."""
    c, tr, no = ref[name]
    nd = ctx.normals(c.P, c.k)                                # KSS_OK, or this raises
    assert nd.shape == c.P.shape and nd.dtype == F64
    r = N.rules(c.P, c.k, nd, N.C, tr=tr)
    fin = np.isfinite(nd).all(axis=1)
    ok = tr["judged"] & fin
    with np.errstate(all="ignore"):
        ratio = np.where(ok, N.sin_to_v0(nd, tr) / tr["B"], 0.0)
        both = ok & np.isfinite(no).all(axis=1)
        dist = np.where(both, np.linalg.norm(nd - no, axis=1) / tr["B"], 0.0)
    far = N.apart(c.P, c.k, nd, no, N.C, tr=tr)
    differ = N.fallback_differs(nd, no, tr)
    print("%s: n %d k %d judged %.4f non-finite rows %d (oracle %d) largest sin / B %.3f, |n_dev - n_oracle| / B %.3f; offenders %s, "
          "apart %d, trig-free rows %d of which differ %d" % (
              name, len(c.P), c.k, tr["judged"].mean(), int((~fin).sum()), int((~np.isfinite(no).all(axis=1)).sum()), ratio.max(),
              dist.max(), {x: len(v) for x, v in r.items()}, len(far), int(tr["sure"].sum()), len(differ)))
    offenders = N.check(c.P, c.k, nd, N.C, tr=tr, only=c.only)
    assert len(offenders) == 0, offenders[:10]
    assert len(far) == 0, far[:10]
    assert len(differ) == 0, differ[:10]
    if c.share is not None:
        assert tr["judged"].mean() >= c.share
    if name == "plane_exact":                                 # computeRoots2 everywhere: (0, 0, -1) to within the bound
        assert tr["fb"].all() and tr["judged"].all()
        assert np.all(np.linalg.norm(np.cross(nd, [0.0, 0.0, 1.0]), axis=1) <= N.C * tr["B"]) and np.all(nd[:, 2] < 0)
    if name == "origin_point":
        assert len(N.rules(c.P, c.k, nd, N.C, tr=tr)["c"]) == 0 and fin[0]


def test_degenerate_clouds_end_icp_with_a_documented_state(pkg, ctx, ref):
    """Computed normals of 30 coincident points (no finite direction exists) as a source or a target: every family that takes
    its surface model from the kernel ends in NO_CORRESPONDENCES or DEGENERATE, the same bits twice."""
    flat = ref["coincident"][0].P.astype(F32)
    bumpy = pkg.synth.bumpy(4, 6000).astype(F32)
    calls = (lambda: ctx.icp_p2l(flat, bumpy), lambda: ctx.icp_p2l(bumpy, flat), lambda: ctx.icp_gicp(flat, bumpy),
             lambda: ctx.icp_symm(flat, bumpy))
    for call in calls:
        a, b = call(), call()
        print("state %d after %d passes" % (a["state"], a["iterations"]))
        assert a["state"] in (5, pkg.STATE_DEGENERATE) and not a["converged"]
        assert a["state"] == b["state"] and a["iterations"] == b["iterations"]
        assert np.array_equal(_bits(a["T"]), _bits(b["T"]))
        assert np.isfinite(a["T"]).all()


def _same(a, b):
    assert b["iterations"] == a["iterations"] and b["state"] == a["state"] and b["converged"] == a["converged"]
    assert np.array_equal(_bits(b["trace_Tk"]), _bits(a["trace_Tk"]))
    assert np.array_equal(_bits(b["trace_sums"]), _bits(a["trace_sums"]))
    assert np.array_equal(_bits(b["T"]), _bits(a["T"]))
    assert _bits(np.array([b["fitness"]])) == _bits(np.array([a["fitness"]]))


@pytest.mark.parametrize("k", [3, 33, 64])
def test_icp_entry_points_compute_kss_normals(pkg, ctx, k):
    """normals_k = k with no normals given is kss_normals at k rounded to float: the smallest and the largest k the parameter
    structs allow and the first of the K = 64 k-NN bucket."""
    src, tgt, _, _ = G.halves_pair(pkg.synth, 21, 1500, 8.0, n_src=1100)
    sn, tn = (ctx.normals(x.astype(F64), k).astype(F32) for x in (src, tgt))
    p = dict(max_iterations=30)
    a = ctx.icp_gicp(src, tgt, sn, tn, gp=pkg.gicp_params(normals_k=k), params=ctx.icp_params(**p), trace_cap=32)
    assert a["iterations"] >= 1
    _same(a, ctx.icp_gicp(src, tgt, None, None, gp=pkg.gicp_params(normals_k=k), params=ctx.icp_params(**p), trace_cap=32))
    a = ctx.icp_symm(src, tgt, sn, tn, sp=pkg.symm_params(normals_k=k), params=ctx.icp_params(**p), trace_cap=32)
    assert a["iterations"] >= 1
    _same(a, ctx.icp_symm(src, tgt, None, None, sp=pkg.symm_params(normals_k=k), params=ctx.icp_params(**p), trace_cap=32))


@pytest.mark.parametrize("k", [3, 33, 64])
def test_batch_computes_kss_normals_at_odd_offsets(pkg, ctx, k):
    """1001, 1500 and 777 points: the second and third clouds start at odd point offsets, so the slice whose normals are
    computed is only 4-byte aligned."""
    pairs = [G.halves_pair(pkg.synth, 30 + i, n, 6.0 + 2 * i)[:2] for i, n in enumerate((1001, 1500, 777))]
    so = np.concatenate([[0], np.cumsum([len(s) for s, _ in pairs])]).astype(np.int64)
    to = np.concatenate([[0], np.cumsum([len(t) for _, t in pairs])]).astype(np.int64)
    assert so[1] % 2 == 1 and so[2] % 2 == 1 and to[1] % 2 == 1 and to[2] % 2 == 1
    s, t = np.concatenate([s for s, _ in pairs]), np.concatenate([t for _, t in pairs])
    sn = np.concatenate([ctx.normals(s_.astype(F64), k).astype(F32) for s_, _ in pairs])
    tn = np.concatenate([ctx.normals(t_.astype(F64), k).astype(F32) for _, t_ in pairs])
    gp = pkg.gicp_params(normals_k=k)
    given, _ = ctx.icp_gicp_batch(s, so, t, to, sn, tn, gp=gp, params=ctx.icp_params(max_iterations=30))
    computed, _ = ctx.icp_gicp_batch(s, so, t, to, None, None, gp=gp, params=ctx.icp_params(max_iterations=30))
    for a, b in zip(given, computed):
        assert a.iterations == b.iterations >= 1 and a.state == b.state and bool(a.converged) == bool(b.converged)
        assert np.array_equal(_bits(a.matrix()), _bits(b.matrix()))
        assert _bits(np.array([a.last_mse])) == _bits(np.array([b.last_mse]))
        assert _bits(np.array([a.fitness])) == _bits(np.array([b.fitness]))


def test_normals_are_deterministic_across_calls_and_contexts(pkg, ctx, ref):
    other = pkg.Context(0)
    try:
        for name in ("bumpy4_k64", "bumpy4_plus100", "lattice", "coincident"):
            c = ref[name][0]
            a = ctx.normals(c.P, c.k)
            assert np.array_equal(_bits(a), _bits(ctx.normals(c.P, c.k)))
            assert np.array_equal(_bits(a), _bits(other.normals(c.P, c.k)))
    finally:
        other.close()


def test_normals_bad_arguments(pkg, ctx):
    P = pkg.synth.bumpy(3, 300)
    for k in (0, 65, -1):
        with pytest.raises(pkg.KssError) as e:
            ctx.normals(P, k)
        assert e.value.status == -1
    assert np.isfinite(ctx.normals(P, 1)).sum() == 0          # one neighbour: no direction, no finite component
    assert ctx.normals(P, 64).shape == (300, 3)
