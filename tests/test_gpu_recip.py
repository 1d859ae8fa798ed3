"""Reciprocal ICP on the device (kss_recip_filter[_dev], kss_icp_recip[_dev]) against the independent restatement
in tests/recip_ref.py: the filter bit for bit on maps that exercise every path of the reverse search, the loop on the seven scenes
of DESIGN.md 2.25's table with both metrics, the anchor to kss_icp_o2o and kss_icp_trimmed bit for bit on an injective mutual
scene, the engines and knobs on exact ties, and the endings."""

import numpy as np
import pytest

import o2o_ref as OR
import recip_ref as RR

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
PAIRS = [(1, 6000, 10.0, -0.35, 0.5), (2, 6000, 15.0, -0.2, 0.6), (3, 8000, 8.0, -0.5, 0.3)]      # test_gpu_trim.py's
METRICS = [RR.POINT, RR.PLANE]
LENGTHS = [1, 63, 64, 65, 255, 256, 257, 1000, 5000]
QNAN = 0x7FC00000


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == F64 else np.uint32)


def _f32_bits(x):
    return int(np.array([x], F32).view(np.uint32)[0])


# ---- input sets of the filter: (n, rng, O) -> (src, tgt, idx int32, d2 float32, max_d2) ----
def _nt(n):
    return max(1, (3 * n) // 4)


def _exact_nn(n, rng, O):
    src, tgt = rng.uniform(-1, 1, (n, 3)).astype(F32), rng.uniform(-1, 1, (_nt(n), 3)).astype(F32)
    return (src, tgt) + tuple(O.nn_brute(src, tgt)) + (4.0,)


def _random_map(n, rng, O):
    """Not the NN map: the balls are large and most winners take the escape."""
    src, tgt = rng.uniform(-1, 1, (n, 3)).astype(F32), rng.uniform(-1, 1, (_nt(n), 3)).astype(F32)
    idx = rng.integers(0, len(tgt), n).astype(np.int32)
    return src, tgt, idx, RR.dist2(src, tgt[idx]), 100.0


def _one_point(n, rng, O):
    """Every source at one point: one cell holds them all, they all choose one target at one d2, the lowest index survives."""
    tgt = rng.uniform(-1, 1, (_nt(n), 3)).astype(F32)
    src = np.tile(np.array([[0.3, -0.2, 0.1]], F32), (n, 1))
    return (src, tgt) + tuple(O.nn_brute(src, tgt)) + (4.0,)


def _duplicates(n, rng, O):
    src, tgt = rng.uniform(-1, 1, (n, 3)).astype(F32), rng.uniform(-1, 1, (_nt(n), 3)).astype(F32)
    k = min(50, n // 2)
    src[n - k:] = src[:k]
    return (src, tgt) + tuple(O.nn_brute(src, tgt)) + (4.0,)


def _far_outside(n, rng, O):
    """Sources far outside the target's box with a huge max_d2: they all fall into border cells."""
    tgt = rng.uniform(-1, 1, (_nt(n), 3)).astype(F32)
    src = (rng.uniform(-1, 1, (n, 3)) * np.array([40.0, 3.0, 1.0]) + np.array([60.0, -20.0, 0.0])).astype(F32)
    src[::3] = (rng.uniform(-1, 1, (len(src[::3]), 3))).astype(F32)
    return (src, tgt) + tuple(O.nn_brute(src, tgt)) + (1e12,)


def _planar(n, rng, O):
    src, tgt = rng.uniform(-1, 1, (n, 3)).astype(F32), rng.uniform(-1, 1, (_nt(n), 3)).astype(F32)
    src[:, 2] = 0.0
    tgt[:, 2] = 0.0
    return (src, tgt) + tuple(O.nn_brute(src, tgt)) + (4.0,)


def _collinear(n, rng, O):
    src, tgt = rng.uniform(-1, 1, (n, 3)).astype(F32), rng.uniform(-1, 1, (_nt(n), 3)).astype(F32)
    src[:, 1:] = np.array([0.25, -0.5], F32)
    tgt[:, 1:] = np.array([0.25, -0.5], F32)
    return (src, tgt) + tuple(O.nn_brute(src, tgt)) + (4.0,)


def _one_target(n, rng, O):
    src = rng.uniform(-1, 1, (n, 3)).astype(F32)
    tgt = np.array([[0.1, 0.2, -0.3]], F32)
    return (src, tgt) + tuple(O.nn_brute(src, tgt)) + (4.0,)


def _odd_d2(n, rng, O):
    """The exact map with d2 replaced by -0.0f, +0.0f, denormals and the true value in turn, and one NaN d2 row."""
    src, tgt, idx, d2, _ = _exact_nn(n, rng, O)
    pick = rng.integers(0, 4, n)
    den = rng.integers(1, 0x800000, n).astype(np.uint32).view(F32)
    d2 = np.where(pick == 0, F32(-0.0), np.where(pick == 1, F32(0.0), np.where(pick == 2, den, d2))).astype(F32)
    d2[n // 2] = np.nan
    return src, tgt, idx, d2, 4.0


SETS = [_exact_nn, _random_map, _one_point, _duplicates, _far_outside, _planar, _collinear, _one_target, _odd_d2]


@pytest.mark.parametrize("gen", SETS, ids=lambda g: g.__name__.strip("_"))
@pytest.mark.parametrize("n", LENGTHS)
def test_filter_bit_exact(ctx, O, n, gen):
    import torch
    src, tgt, idx, d2, max_d2 = gen(n, np.random.default_rng(n + 31 * SETS.index(gen)), O)
    assert idx.dtype == np.int32 and d2.dtype == F32 and len(idx) == len(d2) == len(src) == n
    want_i, want_d, m, u, r = RR.filter_direct(src, tgt, idx, d2, max_d2)
    if gen not in (_random_map, _odd_d2):          # an exact NN map: the restatement's other form says the same
        alt = RR.filter_nn(O, src, tgt, idx, d2, max_d2)
        assert alt[2:] == (m, u, r) and np.array_equal(alt[0], want_i) and np.array_equal(_bits(alt[1]), _bits(want_d))
    got_i, got_d, gm, gu, gr = ctx.recip_filter(src, tgt, idx, d2, max_d2)
    print("%s n %d: m %d u %d r %d (library %d %d %d)" % (gen.__name__, n, m, u, r, gm, gu, gr))
    assert (gm, gu, gr) == (m, u, r)
    assert np.array_equal(got_i, want_i)
    assert np.array_equal(_bits(got_d), _bits(want_d))
    assert r == int(((want_i >= 0) & OR.candidates(idx, d2, len(tgt), max_d2)).sum()) <= u <= m
    if gen is _one_point:
        assert (m, u, r) == (n, 1, 1) and want_i[0] == idx[0] and np.all(want_i[1:] == -1)
    if gen is _random_map and n >= 1000:
        assert r < u          # the check is live on large balls
    # either output may be missing, the outputs may be the inputs
    only_i = ctx.recip_filter(src, tgt, idx, d2, max_d2, want_d2=False)
    only_d = ctx.recip_filter(src, tgt, idx, d2, max_d2, want_idx=False)
    assert only_i[1] is None and only_d[0] is None and only_i[2:] == only_d[2:] == (m, u, r)
    assert np.array_equal(only_i[0], want_i) and np.array_equal(_bits(only_d[1]), _bits(want_d))
    al = ctx.recip_filter(src, tgt, idx, d2, max_d2, alias=True)
    assert al[2:] == (m, u, r) and np.array_equal(al[0], want_i) and np.array_equal(_bits(al[1]), _bits(want_d))
    # the device form on separate outputs, then on its own inputs
    ds, dt = torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda()
    di, dd = torch.from_numpy(idx).cuda(), torch.from_numpy(d2).cuda()
    oi, od = torch.empty_like(di), torch.empty_like(dd)
    torch.cuda.synchronize()
    args = (ds.data_ptr(), n, dt.data_ptr(), len(tgt), di.data_ptr(), dd.data_ptr(), max_d2, 0)
    assert ctx.recip_filter_dev(*args, oi.data_ptr(), od.data_ptr()) == (m, u, r)
    assert np.array_equal(di.cpu().numpy(), idx) and np.array_equal(_bits(dd.cpu().numpy()), _bits(d2))      # the inputs are read only
    assert np.array_equal(oi.cpu().numpy(), want_i) and np.array_equal(_bits(od.cpu().numpy()), _bits(want_d))
    assert ctx.recip_filter_dev(*args, di.data_ptr(), dd.data_ptr()) == (m, u, r)
    assert np.array_equal(di.cpu().numpy(), want_i) and np.array_equal(_bits(dd.cpu().numpy()), _bits(want_d))


def test_filter_non_finite_sources_neither_fault_nor_bin(ctx, O):
    """Outside the definition: asserted is only that the call returns and that the rows far from the non-finite ones are untouched."""
    rng = np.random.default_rng(77)
    src, tgt, idx, d2, max_d2 = _exact_nn(1000, rng, O)
    want = RR.filter_direct(src, tgt, idx, d2, max_d2)
    bad = src.copy()
    bad[10] = np.nan
    bad[20, 1] = np.inf
    bad[30, 2] = -np.inf
    d2b = d2.copy()
    d2b[[10, 20, 30]] = np.nan          # what the NN pass gives such a source: no candidate
    got = ctx.recip_filter(bad, tgt, idx, d2b, max_d2)
    ref = RR.filter_direct(bad, tgt, idx, d2b, max_d2)
    assert got[2:] == ref[2:] and np.array_equal(got[0], ref[0]) and np.array_equal(_bits(got[1]), _bits(ref[1]))
    assert got[2] == want[2] - 3


# ---- the loop ----
def _normals(ctx, tgt):
    return ctx.normals(tgt.astype(F64), 20).astype(F32)


def _bumpy(pkg, pair_id, n, deg, n_src=None, t=(0.02, -0.01, 0.03)):
    axis = pkg.synth.sphere(7000 + pair_id, 1)[0]
    return pkg.synth.make_pair(pair_id, n, R=pkg.synth.rot_axis_angle(axis, np.deg2rad(deg)), t=t, shape="bumpy", n_src=n_src)


def _partial(pkg, spec):
    src, tgt, R, t, ov = pkg.synth.make_partial_pair(*spec)
    return src, tgt, R.T, -R.T @ t


def _with_outliers(pkg, src, pair_id):
    """The first fifth of the source rows moved by (u - 0.5) * 1.2, u[:, j] = u01(9100 + pair_id, k, j * k)."""
    k = len(src) // 5
    u = np.stack([pkg.synth.u01(9100 + pair_id, k, j * k) for j in range(3)], axis=1)
    out = src.astype(F64)
    out[:k] += (u - 0.5) * 1.2
    return out.astype(F32)


def _scene(pkg, name):
    """(src, tgt, R_true, t_true) with T_true mapping the source onto the target; the seven scenes of DESIGN.md 2.25's table and the
    three plain pairs."""
    kind, k = name.split(":")
    k = int(k)
    if kind == "outlier":
        spec = {1: (1, 6000, 10.0, 0.2), 2: (2, 6000, 15.0, 0.3), 3: (3, 8000, 8.0, 0.4)}[k]
        src, tgt, R, t = pkg.synth.make_outlier_pair(*spec)
        return src, tgt, R.T, -R.T @ t
    src, tgt, R_true, t_true = _partial(pkg, PAIRS[k - 1])
    if kind == "partial_outliers":
        src = _with_outliers(pkg, src, k)
    elif kind == "sparse":
        src = np.ascontiguousarray(src[::4])
    else:
        assert kind == "plain"
    return src, tgt, R_true, t_true


TABLE = ["outlier:1", "outlier:2", "outlier:3", "partial_outliers:1", "partial_outliers:2", "sparse:1", "sparse:2"]
O2O_MISSES = {"outlier:3", "partial_outliers:1", "sparse:1", "sparse:2"}      # its restatement ends >= 5.9e-2 there
CASES = [(s, 1.0) for s in TABLE] + [("plain:%d" % k, ov) for k in (1, 2, 3) for ov in (1.0, 0.9)]
# plane metric: the recovery bar is asserted where the restatement, run on the CPU with tests/normals_ref.py's normals, ends below
# 2e-3 (DESIGN.md 2.25 records the values: 1.2e-4 .. 3.5e-4 on these but partial pair 2 + outliers at 1.95e-3; partial pair 1 +
# outliers ends at 5.5e-3 and carries no bar)
PLANE_RECOVERS = {"outlier:1", "outlier:2", "outlier:3", "partial_outliers:2", "sparse:1", "sparse:2", "plain:1", "plain:2", "plain:3"}

_REF = {}


def _reference(O, name, src, tgt, nrm, overlap, metric):
    key = (name, overlap, metric)
    if key not in _REF:
        _REF[key] = RR.icp_recip(O, src, tgt, nrm, overlap, metric, max_iterations=200)
    return _REF[key]


def _err(T, R_true, t_true):
    return max(np.abs(T[:3, :3] - R_true).max(), np.abs(T[:3, 3] - t_true).max())


def _check_loop(pkg, ctx, O, name, overlap, metric, **kw):
    src, tgt, R_true, t_true = _scene(pkg, name)
    nrm = _normals(ctx, tgt) if metric == RR.PLANE else None
    got = ctx.icp_recip(src, tgt, nrm, overlap=overlap, metric=metric, params=ctx.icp_params(max_iterations=200, **kw), trace_cap=256)
    ref = _reference(O, name, src, tgt, nrm, overlap, metric)
    err = _err(got["T"], R_true, t_true)
    print("%s metric %d overlap %.1f: library %d it. state %d, restatement %d it. state %d, max|T - T_ref| %.2e, vs truth %.2e (restatement "
          "%.2e), pass 0 {r, k, tau, kept, m, u} %s, last %s" % (name, metric, overlap, got["iterations"], got["state"], ref["iterations"],
                                                                 ref["state"], np.abs(got["T"] - ref["T"]).max(), err,
                                                                 _err(ref["T"], R_true, t_true), got["trace_recip"][0], got["recip_info"]))
    assert got["iterations"] == ref["iterations"] >= 1
    assert got["state"] == ref["state"] and got["converged"] == ref["converged"]
    # pass 0 sees the same positions on both sides: the rejection and the selection agree exactly
    g0, r0 = got["trace_recip"][0], ref["trace_recip"][0]
    assert g0[0] == r0[0] and g0[1] == r0[1] and g0[3] == r0[3] and g0[4] == r0[4] and g0[5] == r0[5]
    assert _f32_bits(g0[2]) == _f32_bits(r0[2]) and g0[2] == r0[2]
    assert g0[0] < g0[5] <= g0[4]          # r < u in pass 0: the check is live
    s0, q0 = got["trace_sums"][0], ref["trace_sums"][0]
    assert s0[0] == q0[0]
    assert np.all(np.abs(s0 - q0) <= 1e-9 * np.maximum(np.abs(q0), 1.0))
    # later passes through the transforms
    assert np.abs(got["trace_Tk"] - ref["trace_Tk"]).max() <= 1e-6
    assert np.abs(got["T"] - ref["T"]).max() <= 5e-6
    assert abs(got["fitness"] - ref["fitness"]) <= 1e-9 * max(1.0, ref["fitness"])
    assert np.array_equal(got["recip_info"], got["trace_recip"][-1])
    assert got["recip_info"][4] == ref["recip_info"][4]
    return src, tgt, nrm, R_true, t_true, err


@pytest.mark.parametrize("name,overlap", CASES, ids=["%s-%.1f" % c for c in CASES])
def test_icp_recip_matches_restatement_and_recovers(pkg, ctx, O, name, overlap):
    src, tgt, nrm, R_true, t_true, err = _check_loop(pkg, ctx, O, name, overlap, RR.POINT)
    # recovery with nothing told to the method: the project's bar (tests/test_gpu_o2o.py, tests/test_gpu_trim.py)
    assert err < 2e-3
    if name in O2O_MISSES:      # ... which one-to-one misses on the same scene
        o2o = ctx.icp_o2o(src, tgt, None, overlap=1.0, metric=RR.POINT, params=ctx.icp_params(max_iterations=200))
        e = _err(o2o["T"], R_true, t_true)
        print("    kss_icp_o2o at overlap 1.0: %.2e" % e)
        assert not e < 2e-3


@pytest.mark.parametrize("name,overlap", CASES, ids=["%s-%.1f" % c for c in CASES])
def test_icp_recip_plane_matches_restatement(pkg, ctx, O, name, overlap):
    err = _check_loop(pkg, ctx, O, name, overlap, RR.PLANE)[-1]
    if name in PLANE_RECOVERS:
        assert err < 2e-3


@pytest.mark.parametrize("nn_mode", ["grid", "brute"])
@pytest.mark.parametrize("metric", METRICS, ids=["point", "plane"])
def test_icp_recip_source_forms_match_restatement(pkg, ctx, O, metric, nn_mode):
    """The single pair is a batch of one descriptor without the row -> pair table and without states, in both forms
    its sources take: the cell-list engine re-orders them (read through the permutation), the brute-force engine leaves them in
    place.  test_icp_recip_engines_and_knobs_bit_identical compares the engines with each other only; here each is held against the
    restatement, with the bounds of _check_loop."""
    mode = pkg.NN_GRID if nn_mode == "grid" else pkg.NN_BRUTE
    err = _check_loop(pkg, ctx, O, "outlier:1", 1.0, metric, nn_mode=mode)[-1]
    assert err < 2e-3


# ---- the anchor: every source nearest to its own point and vice versa, in every pass ----
def _lattice_pair(pkg):
    """tests/test_gpu_o2o.py's scene.  Target: a 40 x 40 lattice of spacing 0.05 centred on the origin, every x and y moved by less
    than 0.01, z a height field: no two points closer than 0.04.  Source: 1000 of its points in a shuffled order, turned 0.3 degrees,
    moved about 0.003, jitter 1e-4: less than 0.011 from where it was, so every source is nearest to its own point -- and, no other
    source being within 0.04 - 0.011 of that point, the nearest source of it."""
    S = pkg.synth
    g = (np.arange(40) - 19.5) * 0.05
    xy = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    xy = xy + 0.01 * np.stack([S.u01(811, 1600), S.u01(812, 1600)], 1)
    z = 0.15 * np.sin(3.0 * xy[:, 0]) * np.cos(2.0 * xy[:, 1]) + 0.05 * xy[:, 0] * xy[:, 1]
    tgt = np.concatenate([xy, z[:, None]], 1)
    pick = S.permutation(813, 1600)[:1000]
    R = S.rot_axis_angle([0.2, 0.1, 1.0], np.deg2rad(0.3))
    src = tgt[pick] @ R.T + np.array([0.002, -0.0015, 0.001]) + 1e-4 * (2.0 * S.u01(814, 3000).reshape(1000, 3) - 1.0)
    return src.astype(F32), tgt.astype(F32)


def _same_run(a, b):
    assert a["iterations"] == b["iterations"] and a["state"] == b["state"] and a["converged"] == b["converged"]
    assert np.array_equal(_bits(a["T"]), _bits(b["T"]))
    assert _bits(np.array([a["last_mse"]])) == _bits(np.array([b["last_mse"]]))
    assert np.array_equal(_bits(a["trace_Tk"]), _bits(b["trace_Tk"]))
    assert np.array_equal(_bits(a["trace_sums"]), _bits(b["trace_sums"]))
    assert _bits(np.array([a["fitness"]])) == _bits(np.array([b["fitness"]]))


@pytest.mark.parametrize("nn_fma", [0, 1])
@pytest.mark.parametrize("overlap", [1.0, 0.5])
@pytest.mark.parametrize("metric", METRICS, ids=["point", "plane"])
def test_anchor_mutual_scene_is_icp_o2o_and_icp_trimmed_bit_for_bit(pkg, ctx, metric, overlap, nn_fma):
    src, tgt = _lattice_pair(pkg)
    nrm = _normals(ctx, tgt) if metric == RR.PLANE else None
    kw = dict(max_iterations=10, fixed_iterations=1, nn_fma=nn_fma)
    b = ctx.icp_o2o(src, tgt, nrm, overlap=overlap, metric=metric, params=ctx.icp_params(**kw), trace_cap=16)
    c = ctx.icp_recip(src, tgt, nrm, overlap=overlap, metric=metric, params=ctx.icp_params(**kw), trace_cap=16)
    tt = c["trace_recip"]
    assert c["iterations"] == 10 and len(tt) == 10
    assert np.all(tt[:, 0] == 1000) and np.all(tt[:, 4] == 1000) and np.all(tt[:, 5] == 1000)      # r == u == m in every pass
    _same_run(b, c)
    assert np.array_equal(_bits(b["trace_o2o"]), _bits(tt[:, :5]))
    assert np.array_equal(_bits(b["o2o_info"]), _bits(c["recip_info"][:5]))
    if nn_fma == 0:
        a = ctx.icp_trimmed(src, tgt, nrm, overlap=overlap, metric=metric, params=ctx.icp_params(**kw), trace_cap=16)
        _same_run(a, c)
        assert np.array_equal(_bits(a["trace_trim"]), _bits(tt[:, :4]))
        assert np.array_equal(_bits(a["trim_info"]), _bits(c["recip_info"][:4]))


# ---- engines and knobs on exact ties ----
@pytest.mark.parametrize("metric", METRICS, ids=["point", "plane"])
def test_icp_recip_engines_and_knobs_bit_identical(pkg, ctx, metric):
    src, tgt = _partial(pkg, PAIRS[1])[:2]
    src = np.concatenate([src, src[:50]])          # 50 exact duplicate rows: the same target at the same d2, the lower index wins
    nrm = _normals(ctx, tgt) if metric == RR.PLANE else None
    runs = []
    for kw in (dict(nn_mode=pkg.NN_BRUTE), dict(nn_mode=pkg.NN_GRID), dict(nn_mode=pkg.NN_AUTO),
               dict(nn_mode=pkg.NN_BRUTE, nn_sources_per_thread=1, nn_target_splits=3),
               dict(nn_mode=pkg.NN_BRUTE, nn_sources_per_thread=8, nn_target_splits=1)):
        runs.append(ctx.icp_recip(src, tgt, nrm, overlap=0.9, metric=metric, params=ctx.icp_params(max_iterations=40, **kw),
                                  trace_cap=64, fitness_corr=True))
    a = runs[0]
    assert a["iterations"] >= 2
    # of a duplicate and its original never both survive: of the two equal keys the lower index wins the target
    assert np.all(a["trace_recip"][:, 5] <= a["trace_recip"][:, 4] - 50)
    assert np.all(a["trace_recip"][:, 0] <= a["trace_recip"][:, 5])
    for b in runs[1:]:
        assert b["iterations"] == a["iterations"] and b["state"] == a["state"]
        assert np.array_equal(_bits(b["trace_Tk"]), _bits(a["trace_Tk"]))
        assert np.array_equal(_bits(b["trace_sums"]), _bits(a["trace_sums"]))
        assert np.array_equal(_bits(b["trace_recip"]), _bits(a["trace_recip"]))
        assert np.array_equal(_bits(b["recip_info"]), _bits(a["recip_info"]))
        assert np.array_equal(_bits(b["T"]), _bits(a["T"]))
        assert _bits(np.array([b["last_mse"]])) == _bits(np.array([a["last_mse"]]))
        # fitness_idx / fitness_d2 are the unfiltered NN: every source has one
        assert np.array_equal(b["fitness_idx"], a["fitness_idx"]) and np.array_equal(_bits(b["fitness_d2"]), _bits(a["fitness_d2"]))
        # (the bound of test_gpu_trim.py for two summation orders of the NN engines' f64 sum over all sources)
        assert abs(b["fitness"] - a["fitness"]) <= 2.0 * len(src) * 2.0 ** -53 * a["fitness"]
    assert np.all(a["fitness_idx"] >= 0) and np.all(np.isfinite(a["fitness_d2"]))


@pytest.mark.parametrize("metric", METRICS, ids=["point", "plane"])
def test_icp_recip_dev_matches_host(pkg, ctx, metric):
    import torch
    src, tgt = _partial(pkg, PAIRS[0])[:2]
    nrm = _normals(ctx, tgt)
    h = ctx.icp_recip(src, tgt, nrm if metric == RR.PLANE else None, overlap=0.9, metric=metric)
    s, t, nr = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (src, tgt, nrm))
    torch.cuda.synchronize()
    for d_n in ((nr.data_ptr(), None) if metric == RR.PLANE else (None,)):
        r, info = ctx.icp_recip_dev(s.data_ptr(), len(src), t.data_ptr(), len(tgt), d_n, ctx.icp_params(), overlap=0.9, metric=metric)
        assert r.iterations == h["iterations"] and r.state == h["state"]
        assert np.array_equal(_bits(r.matrix()), _bits(h["T"]))
        assert r.fitness == h["fitness"]
        assert np.array_equal(_bits(info), _bits(h["recip_info"]))


# ---- endings: each leaves the context clean ----
class _Witness:
    """kss_icp_recip and kss_icp_o2o on a fixed pair: what the context gave before must be what it gives afterwards."""

    def __init__(self, pkg, ctx):
        self.ctx = ctx
        self.src, self.tgt = _bumpy(pkg, 11, 3000, 7.0, n_src=2500)
        self.nrm = _normals(ctx, self.tgt)
        self.before = self.run()

    def run(self):
        a = self.ctx.icp_recip(self.src, self.tgt, self.nrm, overlap=0.9, metric=RR.PLANE, trace_cap=64)
        b = self.ctx.icp_o2o(self.src, self.tgt, None, overlap=0.7, metric=RR.POINT, trace_cap=64)
        return a, b

    def check(self):
        for x, y in zip(self.before, self.run()):
            assert x["iterations"] == y["iterations"] and x["state"] == y["state"]
            assert np.array_equal(_bits(x["T"]), _bits(y["T"]))
            assert np.array_equal(_bits(x["trace_sums"]), _bits(y["trace_sums"]))
            assert _bits(np.array([x["fitness"]])) == _bits(np.array([y["fitness"]]))


@pytest.mark.parametrize("metric", METRICS, ids=["point", "plane"])
def test_ending_too_few_kept(pkg, ctx, metric):
    w = _Witness(pkg, ctx)
    src, tgt = _bumpy(pkg, 12, 500, 5.0)
    nrm = _normals(ctx, tgt) if metric == RR.PLANE else None
    got = ctx.icp_recip(src, tgt, nrm, overlap=0.001, metric=metric)       # k = 1 < min_correspondences = 3
    info = got["recip_info"]
    assert got["state"] == 5 and got["iterations"] == 0 and not got["converged"]
    assert info[4] == 500 and 1 <= info[0] <= info[5] <= 500 and info[1] == 1 and 1 <= info[3] < 3
    assert np.array_equal(got["T"], np.eye(4, dtype=F32))
    w.check()


@pytest.mark.parametrize("metric", METRICS, ids=["point", "plane"])
def test_ending_no_candidate(pkg, ctx, metric):
    w = _Witness(pkg, ctx)
    src, tgt = _bumpy(pkg, 9, 2000, 5.0)
    nrm = _normals(ctx, tgt) if metric == RR.PLANE else None
    got = ctx.icp_recip(src + np.float32(100.0), tgt, nrm, overlap=1.0, metric=metric)
    assert got["state"] == 5 and got["iterations"] == 0 and not got["converged"]
    assert np.array_equal(got["recip_info"], np.zeros(6))
    assert np.array_equal(got["T"], np.eye(4, dtype=F32))
    w.check()


def test_ending_planar_target_degenerate(pkg, ctx):
    w = _Witness(pkg, ctx)
    g = np.linspace(-1, 1, 40)
    tgt = np.stack(np.meshgrid(g, g), -1).reshape(-1, 2)
    tgt = np.concatenate([tgt, np.zeros((len(tgt), 1))], 1).astype(F32)
    src = (tgt[::2] + np.array([0.01, -0.02, 0.05])).astype(F32)
    nrm = np.tile(np.array([0, 0, 1], F32), (len(tgt), 1))
    got = ctx.icp_recip(src, tgt, nrm, overlap=1.0, metric=RR.PLANE)
    assert got["state"] == pkg.STATE_DEGENERATE and not got["converged"] and got["iterations"] == 0
    assert np.isfinite(got["T"]).all()
    assert got["recip_info"][4] == len(src) and got["recip_info"][0] >= 3
    w.check()


@pytest.mark.parametrize("metric", METRICS, ids=["point", "plane"])
def test_ending_no_iterations(pkg, ctx, metric):
    src, tgt = _bumpy(pkg, 13, 1500, 5.0)
    nrm = _normals(ctx, tgt) if metric == RR.PLANE else None
    got = ctx.icp_recip(src, tgt, nrm, overlap=1.0, metric=metric, params=ctx.icp_params(max_iterations=0), trace_cap=8)
    ref = ctx.icp_trimmed(src, tgt, nrm, overlap=1.0, metric=metric, params=ctx.icp_params(max_iterations=0), trace_cap=8)
    assert got["iterations"] == 0 and len(got["trace_recip"]) == 0 and np.array_equal(got["recip_info"], np.zeros(6))
    assert np.array_equal(got["T"], np.eye(4, dtype=F32))
    assert got["state"] == ref["state"] and got["converged"] == ref["converged"] and got["fitness"] == ref["fitness"]


def test_ending_argument_errors(pkg, ctx):
    import ctypes as C
    w = _Witness(pkg, ctx)
    src, tgt = _bumpy(pkg, 10, 1000, 5.0)
    nrm = _normals(ctx, tgt)
    p = ctx.icp_params()
    p.allreduce = pkg.binding.ALLREDUCE_FN(lambda user, values, n: 0)
    with pytest.raises(pkg.KssError) as e:
        ctx.icp_recip(src, tgt, nrm, overlap=0.5, metric=RR.PLANE, params=p)
    assert e.value.status == -1
    w.check()
    for overlap in (0.0, -0.5, 1.0000001, float("nan")):
        with pytest.raises(pkg.KssError) as e:
            ctx.icp_recip(src, tgt, None, overlap=overlap, metric=RR.POINT)
        assert e.value.status == -1
    with pytest.raises(pkg.KssError) as e:
        ctx.icp_recip(src, tgt, nrm, overlap=0.5, metric=RR.POINT)          # the point metric takes no normals
    assert e.value.status == -1
    with pytest.raises(pkg.KssError) as e:
        ctx.icp_recip(src, tgt, None, overlap=0.5, metric=7)
    assert e.value.status == -1
    with pytest.raises(pkg.KssError) as e:
        ctx.icp_recip(src[:0], tgt, None)
    assert e.value.status == -1
    w.check()
    # a NULL rp, NULL result, NULL clouds, NULL params
    L, q, res, info = ctx.L, ctx.icp_params(), pkg.IcpResult(), np.zeros(6)
    rp = pkg.recip_params()
    sp, tp = src.ctypes.data_as(C.c_void_p), tgt.ctypes.data_as(C.c_void_p)
    ip = info.ctypes.data_as(C.c_void_p)
    assert L.kss_icp_recip(ctx.h, sp, len(src), tp, len(tgt), None, C.byref(q), None, C.byref(res), ip) == -1
    assert L.kss_icp_recip(ctx.h, sp, len(src), tp, len(tgt), None, C.byref(q), C.byref(rp), None, ip) == -1
    assert L.kss_icp_recip(ctx.h, None, len(src), tp, len(tgt), None, C.byref(q), C.byref(rp), C.byref(res), ip) == -1
    assert L.kss_icp_recip(ctx.h, sp, len(src), tp, len(tgt), None, None, C.byref(rp), C.byref(res), ip) == -1
    w.check()
    # the filter alone
    idx, d2 = np.zeros(10, np.int32), np.zeros(10, F32)
    i_p, d_p, i3 = idx.ctypes.data_as(C.c_void_p), d2.ctypes.data_as(C.c_void_p), np.zeros(3).ctypes.data_as(C.c_void_p)
    assert L.kss_recip_filter(ctx.h, sp, 10, tp, 5, i_p, d_p, 1.0, 0, None, None, None) == -1
    assert L.kss_recip_filter(ctx.h, None, 10, tp, 5, i_p, d_p, 1.0, 0, None, None, i3) == -1
    assert L.kss_recip_filter(ctx.h, sp, 10, None, 5, i_p, d_p, 1.0, 0, None, None, i3) == -1
    assert L.kss_recip_filter(ctx.h, sp, 10, tp, 5, None, d_p, 1.0, 0, None, None, i3) == -1
    assert L.kss_recip_filter(ctx.h, sp, 0, tp, 5, i_p, d_p, 1.0, 0, None, None, i3) == -1
    assert L.kss_recip_filter(ctx.h, sp, 10, tp, 0, i_p, d_p, 1.0, 0, None, None, i3) == -1
    assert L.kss_recip_filter(ctx.h, sp, 10, tp, -3, i_p, d_p, 1.0, 0, None, None, i3) == -1
    w.check()
