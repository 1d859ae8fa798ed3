"""One-to-one ICP on the device (kss_o2o_filter[_dev], kss_icp_o2o[_dev]) against the independent restatement in
tests/o2o_ref.py: the filter bit for bit, the loop on the three partly overlapping pairs of tests/test_gpu_trim.py with both
metrics at overlap 1.0 and 0.9, the anchor to kss_icp_trimmed bit for bit on an injective scene, the engines and knobs on exact
ties, and the endings."""

import numpy as np
import pytest

import o2o_ref as OR
import trim_ref as TR

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
PAIRS = [(1, 6000, 10.0, -0.35, 0.5), (2, 6000, 15.0, -0.2, 0.6), (3, 8000, 8.0, -0.5, 0.3)]      # test_gpu_trim.py's
METRICS = [OR.POINT, OR.PLANE]
LENGTHS = [1, 2, 63, 64, 65, 257, 4096, 100000]
INT32_MAX = 2 ** 31 - 1


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == F64 else np.uint32)


def _f32_bits(x):
    return int(np.array([x], F32).view(np.uint32)[0])


# ---- input sets of the filter: (n, rng) -> (idx int32, d2 float32, nt, max_d2) ----
def _uniform(n, rng):
    nt = max(1, n // 4)
    return rng.integers(0, nt, n).astype(np.int32), rng.uniform(0.0, 1.0, n).astype(F32), nt, 1.0


def _one_target(n, rng):
    nt = max(1, n // 4)
    return np.full(n, nt - 1, np.int32), rng.uniform(0.0, 1.0, n).astype(F32), nt, 1.0


def _injective(n, rng):
    return rng.permutation(n).astype(np.int32), rng.uniform(0.0, 1.0, n).astype(F32), n, 1.0


def _one_value(n, rng):
    nt = max(1, n // 4)
    return rng.integers(0, nt, n).astype(np.int32), np.full(n, 0.37, F32), nt, 1.0


def _zeros(n, rng):
    nt = max(1, n // 4)
    return rng.integers(0, nt, n).astype(np.int32), np.where(rng.random(n) < 0.5, F32(-0.0), F32(0.0)).astype(F32), nt, 1.0


def _denormals(n, rng):
    nt = max(1, n // 4)
    d = rng.integers(1, 0x800000, n).astype(np.uint32).view(F32)      # every denormal pattern
    pick = rng.integers(0, 4, n)
    d = np.where(pick == 0, F32(0.0), d)
    d = np.where(pick == 1, F32(-0.0), d)
    return rng.integers(0, nt, n).astype(np.int32), d.astype(F32), nt, 1.0


def _mixed(n, rng):
    nt = max(1, n // 4)
    idx = rng.integers(0, nt, n).astype(np.int32)
    d = rng.uniform(0.0, 2.0, n).astype(F32)
    d[rng.random(n) < 0.10] = F32(2.5)          # above max_d2
    d[rng.random(n) < 0.05] = np.nan
    d[rng.random(n) < 0.05] = F32(-0.5)
    d[rng.random(n) < 0.02] = np.inf
    idx[rng.random(n) < 0.05] = -1
    idx[rng.random(n) < 0.05] = nt
    idx[rng.random(n) < 0.05] = INT32_MAX
    return idx, d, nt, 2.0


SETS = [_uniform, _one_target, _injective, _one_value, _zeros, _denormals, _mixed]


@pytest.mark.parametrize("gen", SETS, ids=lambda g: g.__name__.strip("_"))
@pytest.mark.parametrize("n", LENGTHS)
def test_filter_bit_exact(ctx, n, gen):
    import torch
    idx, d2, nt, max_d2 = gen(n, np.random.default_rng(n + 31 * SETS.index(gen)))
    assert idx.dtype == np.int32 and d2.dtype == F32 and len(idx) == len(d2) == n
    want_i, want_d, m, u = OR.filter(idx, d2, nt, max_d2)
    got_i, got_d, gm, gu = ctx.o2o_filter(idx, d2, nt, max_d2)
    assert (gm, gu) == (m, u)
    assert np.array_equal(got_i, want_i)
    assert np.array_equal(_bits(got_d), _bits(want_d))
    if gen is _injective:
        assert m == u == n and np.array_equal(got_i, idx) and np.array_equal(_bits(got_d), _bits(d2))
    if gen is _one_target:
        assert u == 1 and m == n
    # either output may be missing
    only_i = ctx.o2o_filter(idx, d2, nt, max_d2, want_d2=False)
    only_d = ctx.o2o_filter(idx, d2, nt, max_d2, want_idx=False)
    assert only_i[1] is None and only_d[0] is None and only_i[2:] == only_d[2:] == (m, u)
    assert np.array_equal(only_i[0], want_i) and np.array_equal(_bits(only_d[1]), _bits(want_d))
    # the device form on separate outputs, then on its own inputs
    di, dd = torch.from_numpy(idx).cuda(), torch.from_numpy(d2).cuda()
    oi, od = torch.empty_like(di), torch.empty_like(dd)
    torch.cuda.synchronize()
    assert ctx.o2o_filter_dev(di.data_ptr(), dd.data_ptr(), n, nt, max_d2, oi.data_ptr(), od.data_ptr()) == (m, u)
    assert np.array_equal(di.cpu().numpy(), idx) and np.array_equal(_bits(dd.cpu().numpy()), _bits(d2))      # the inputs are read only
    assert np.array_equal(oi.cpu().numpy(), want_i) and np.array_equal(_bits(od.cpu().numpy()), _bits(want_d))
    assert ctx.o2o_filter_dev(di.data_ptr(), dd.data_ptr(), n, nt, max_d2, di.data_ptr(), dd.data_ptr()) == (m, u)
    assert np.array_equal(di.cpu().numpy(), want_i) and np.array_equal(_bits(dd.cpu().numpy()), _bits(want_d))


# ---- the loop ----
def _normals(ctx, tgt):
    return ctx.normals(tgt.astype(F64), 20).astype(F32)


def _partial(pkg, spec):
    src, tgt, R, t, ov = pkg.synth.make_partial_pair(*spec)
    return src, tgt, R.T, -R.T @ t


def _bumpy(pkg, pair_id, n, deg, n_src=None, t=(0.02, -0.01, 0.03)):
    axis = pkg.synth.sphere(7000 + pair_id, 1)[0]
    return pkg.synth.make_pair(pair_id, n, R=pkg.synth.rot_axis_angle(axis, np.deg2rad(deg)), t=t, shape="bumpy", n_src=n_src)


@pytest.mark.parametrize("overlap", [1.0, 0.9])
@pytest.mark.parametrize("metric", METRICS, ids=["point", "plane"])
@pytest.mark.parametrize("spec", PAIRS, ids=lambda s: "pair%d" % s[0])
def test_icp_o2o_matches_restatement_and_recovers(pkg, ctx, O, spec, metric, overlap):
    src, tgt, R_true, t_true = _partial(pkg, spec)
    nrm = _normals(ctx, tgt) if metric == OR.PLANE else None
    got = ctx.icp_o2o(src, tgt, nrm, overlap=overlap, metric=metric, params=ctx.icp_params(max_iterations=200), trace_cap=256)
    ref = OR.icp_o2o(O, src, tgt, nrm, overlap, metric, max_iterations=200)
    print("pair %d metric %d overlap %.1f: library %d it. state %d, restatement %d it. state %d, max|T - T_ref| %.2e, vs truth %.2e / %.2e" % (
        spec[0], metric, overlap, got["iterations"], got["state"], ref["iterations"], ref["state"], np.abs(got["T"] - ref["T"]).max(),
        np.abs(got["T"][:3, :3] - R_true).max(), np.abs(got["T"][:3, 3] - t_true).max()))
    assert got["iterations"] == ref["iterations"] >= 1
    assert got["state"] == ref["state"] and got["converged"] == ref["converged"]
    # pass 0 sees the same positions on both sides: the rejection and the selection agree exactly
    g0, r0 = got["trace_o2o"][0], ref["trace_o2o"][0]
    assert g0[0] == r0[0] and g0[1] == r0[1] and g0[3] == r0[3] and g0[4] == r0[4]
    assert _f32_bits(g0[2]) == _f32_bits(r0[2]) and g0[2] == r0[2]
    assert g0[0] < g0[4] == len(src)          # sources share targets on these pairs: the rejection is live
    s0, q0 = got["trace_sums"][0], ref["trace_sums"][0]
    assert s0[0] == q0[0]
    assert np.all(np.abs(s0 - q0) <= 1e-9 * np.maximum(np.abs(q0), 1.0))
    # later passes through the transforms
    assert np.abs(got["trace_Tk"] - ref["trace_Tk"]).max() <= 1e-6
    assert np.abs(got["T"] - ref["T"]).max() <= 5e-6
    assert abs(got["fitness"] - ref["fitness"]) <= 1e-9 * max(1.0, ref["fitness"])
    assert np.array_equal(got["o2o_info"], got["trace_o2o"][-1])
    assert got["o2o_info"][4] == ref["o2o_info"][4]
    # recovery through the library with nothing told: the trimmed yardstick's bar ...
    assert np.abs(got["T"][:3, :3] - R_true).max() < 2e-3
    assert np.abs(got["T"][:3, 3] - t_true).max() < 2e-3
    if overlap == 1.0:      # ... which all correspondences miss on the same pair
        full = ctx.icp_trimmed(src, tgt, nrm, overlap=1.0, metric=metric, params=ctx.icp_params(max_iterations=200))
        err = max(np.abs(full["T"][:3, :3] - R_true).max(), np.abs(full["T"][:3, 3] - t_true).max())
        print("    kss_icp_trimmed at overlap 1.0: %.2e" % err)
        assert not err < 2e-3


# ---- the anchor: an injective NN map in every pass ----
def _lattice_pair(pkg):
    """Target: a 40 x 40 lattice of spacing 0.05 centred on the origin, every x and y moved by less than 0.01, z a height field:
    no two points closer than 0.04.  Source: 1000 of its points in a shuffled order, turned 0.3 degrees, moved about 0.003, jitter
    1e-4: at most 1.42 * 0.00524 + 0.0027 + 0.0002 < 0.011 from where it was, so every source is nearest to its own point."""
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


@pytest.mark.parametrize("overlap", [1.0, 0.5])
@pytest.mark.parametrize("metric", METRICS, ids=["point", "plane"])
def test_anchor_injective_scene_is_icp_trimmed_bit_for_bit(pkg, ctx, metric, overlap):
    src, tgt = _lattice_pair(pkg)
    nrm = _normals(ctx, tgt) if metric == OR.PLANE else None
    kw = dict(max_iterations=10, fixed_iterations=1)
    a = ctx.icp_trimmed(src, tgt, nrm, overlap=overlap, metric=metric, params=ctx.icp_params(**kw), trace_cap=16)
    b = ctx.icp_o2o(src, tgt, nrm, overlap=overlap, metric=metric, params=ctx.icp_params(**kw), trace_cap=16)
    assert a["iterations"] == b["iterations"] == 10 and a["state"] == b["state"] and a["converged"] == b["converged"]
    tt = b["trace_o2o"]
    assert len(tt) == 10
    assert np.all(tt[:, 4] == tt[:, 0]) and np.all(tt[:, 0] == len(src))      # m == u in every pass: the scene is injective
    assert np.array_equal(_bits(a["T"]), _bits(b["T"]))
    assert _bits(np.array([a["last_mse"]])) == _bits(np.array([b["last_mse"]]))
    assert np.array_equal(_bits(a["trace_Tk"]), _bits(b["trace_Tk"]))
    assert np.array_equal(_bits(a["trace_sums"]), _bits(b["trace_sums"]))
    assert np.array_equal(_bits(a["trace_trim"]), _bits(tt[:, :4]))
    assert np.array_equal(_bits(a["trim_info"]), _bits(b["o2o_info"][:4]))
    assert _bits(np.array([a["fitness"]])) == _bits(np.array([b["fitness"]]))


# ---- engines and knobs on exact ties ----
@pytest.mark.parametrize("metric", METRICS, ids=["point", "plane"])
def test_icp_o2o_engines_and_knobs_bit_identical(pkg, ctx, metric):
    src, tgt = _partial(pkg, PAIRS[1])[:2]
    src = np.concatenate([src, src[:50]])          # 50 exact duplicate rows: the same target at the same d2, the lower index wins
    nrm = _normals(ctx, tgt) if metric == OR.PLANE else None
    runs = []
    for kw in (dict(nn_mode=pkg.NN_BRUTE), dict(nn_mode=pkg.NN_GRID), dict(nn_mode=pkg.NN_AUTO),
               dict(nn_mode=pkg.NN_BRUTE, nn_sources_per_thread=1, nn_target_splits=3),
               dict(nn_mode=pkg.NN_BRUTE, nn_sources_per_thread=8, nn_target_splits=1)):
        runs.append(ctx.icp_o2o(src, tgt, nrm, overlap=0.9, metric=metric, params=ctx.icp_params(max_iterations=40, **kw),
                                trace_cap=64, fitness_corr=True))
    a = runs[0]
    assert a["iterations"] >= 2
    # a duplicate never survives beside its original: of the two equal keys the lower index wins
    assert np.all(a["trace_o2o"][:, 0] <= a["trace_o2o"][:, 4] - 50)
    for b in runs[1:]:
        assert b["iterations"] == a["iterations"] and b["state"] == a["state"]
        assert np.array_equal(_bits(b["trace_Tk"]), _bits(a["trace_Tk"]))
        assert np.array_equal(_bits(b["trace_sums"]), _bits(a["trace_sums"]))
        assert np.array_equal(_bits(b["trace_o2o"]), _bits(a["trace_o2o"]))
        assert np.array_equal(_bits(b["o2o_info"]), _bits(a["o2o_info"]))
        assert np.array_equal(_bits(b["T"]), _bits(a["T"]))
        assert _bits(np.array([b["last_mse"]])) == _bits(np.array([a["last_mse"]]))
        # fitness_idx / fitness_d2 are the unfiltered NN: every source has one
        assert np.array_equal(b["fitness_idx"], a["fitness_idx"]) and np.array_equal(_bits(b["fitness_d2"]), _bits(a["fitness_d2"]))
        # (the bound of test_gpu_trim.py for two summation orders of the NN engines' f64 sum over all sources)
        assert abs(b["fitness"] - a["fitness"]) <= 2.0 * len(src) * 2.0 ** -53 * a["fitness"]
    assert np.all(a["fitness_idx"] >= 0) and np.all(np.isfinite(a["fitness_d2"]))
    for b in (runs[3], runs[4]):
        assert _bits(np.array([b["fitness"]])) == _bits(np.array([a["fitness"]]))


@pytest.mark.parametrize("metric", METRICS, ids=["point", "plane"])
def test_icp_o2o_dev_matches_host(pkg, ctx, metric):
    import torch
    src, tgt = _partial(pkg, PAIRS[0])[:2]
    nrm = _normals(ctx, tgt)
    h = ctx.icp_o2o(src, tgt, nrm if metric == OR.PLANE else None, overlap=0.9, metric=metric)
    s, t, nr = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (src, tgt, nrm))
    torch.cuda.synchronize()
    for d_n in ((nr.data_ptr(), None) if metric == OR.PLANE else (None,)):
        r, info = ctx.icp_o2o_dev(s.data_ptr(), len(src), t.data_ptr(), len(tgt), d_n, ctx.icp_params(), overlap=0.9, metric=metric)
        assert r.iterations == h["iterations"] and r.state == h["state"]
        assert np.array_equal(_bits(r.matrix()), _bits(h["T"]))
        assert r.fitness == h["fitness"]
        assert np.array_equal(_bits(info), _bits(h["o2o_info"]))


# ---- endings: each leaves the context clean ----
class _Witness:
    """kss_icp_o2o and kss_icp_trimmed on a fixed pair: what the context gave before must be what it gives afterwards."""

    def __init__(self, pkg, ctx):
        self.ctx = ctx
        self.src, self.tgt = _bumpy(pkg, 11, 3000, 7.0, n_src=2500)
        self.nrm = _normals(ctx, self.tgt)
        self.before = self.run()

    def run(self):
        a = self.ctx.icp_o2o(self.src, self.tgt, self.nrm, overlap=0.9, metric=OR.PLANE, trace_cap=64)
        b = self.ctx.icp_trimmed(self.src, self.tgt, None, overlap=0.7, metric=OR.POINT, trace_cap=64)
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
    nrm = _normals(ctx, tgt) if metric == OR.PLANE else None
    got = ctx.icp_o2o(src, tgt, nrm, overlap=0.001, metric=metric)       # k = 1 < min_correspondences = 3
    info = got["o2o_info"]
    assert got["state"] == 5 and got["iterations"] == 0 and not got["converged"]
    assert info[4] == 500 and 1 <= info[0] <= 500 and info[1] == 1 and 1 <= info[3] < 3
    assert np.array_equal(got["T"], np.eye(4, dtype=F32))
    w.check()


@pytest.mark.parametrize("metric", METRICS, ids=["point", "plane"])
def test_ending_no_candidate(pkg, ctx, metric):
    w = _Witness(pkg, ctx)
    src, tgt = _bumpy(pkg, 9, 2000, 5.0)
    nrm = _normals(ctx, tgt) if metric == OR.PLANE else None
    got = ctx.icp_o2o(src + np.float32(100.0), tgt, nrm, overlap=1.0, metric=metric)
    assert got["state"] == 5 and got["iterations"] == 0 and not got["converged"]
    assert np.array_equal(got["o2o_info"], np.zeros(5))
    assert np.array_equal(got["T"], np.eye(4, dtype=F32))
    w.check()


def test_ending_planar_target_degenerate(pkg, ctx):
    w = _Witness(pkg, ctx)
    g = np.linspace(-1, 1, 40)
    tgt = np.stack(np.meshgrid(g, g), -1).reshape(-1, 2)
    tgt = np.concatenate([tgt, np.zeros((len(tgt), 1))], 1).astype(F32)
    src = (tgt[::2] + np.array([0.01, -0.02, 0.05])).astype(F32)
    nrm = np.tile(np.array([0, 0, 1], F32), (len(tgt), 1))
    got = ctx.icp_o2o(src, tgt, nrm, overlap=1.0, metric=OR.PLANE)
    assert got["state"] == pkg.STATE_DEGENERATE and not got["converged"] and got["iterations"] == 0
    assert np.isfinite(got["T"]).all()
    assert got["o2o_info"][4] == len(src) and got["o2o_info"][0] >= 3
    w.check()


@pytest.mark.parametrize("metric", METRICS, ids=["point", "plane"])
def test_ending_no_iterations(pkg, ctx, metric):
    src, tgt = _bumpy(pkg, 13, 1500, 5.0)
    nrm = _normals(ctx, tgt) if metric == OR.PLANE else None
    got = ctx.icp_o2o(src, tgt, nrm, overlap=1.0, metric=metric, params=ctx.icp_params(max_iterations=0), trace_cap=8)
    ref = ctx.icp_trimmed(src, tgt, nrm, overlap=1.0, metric=metric, params=ctx.icp_params(max_iterations=0), trace_cap=8)
    assert got["iterations"] == 0 and len(got["trace_o2o"]) == 0 and np.array_equal(got["o2o_info"], np.zeros(5))
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
        ctx.icp_o2o(src, tgt, nrm, overlap=0.5, metric=OR.PLANE, params=p)
    assert e.value.status == -1
    w.check()
    for overlap in (0.0, -0.5, 1.0000001, float("nan")):
        with pytest.raises(pkg.KssError) as e:
            ctx.icp_o2o(src, tgt, None, overlap=overlap, metric=OR.POINT)
        assert e.value.status == -1
    with pytest.raises(pkg.KssError) as e:
        ctx.icp_o2o(src, tgt, nrm, overlap=0.5, metric=OR.POINT)          # the point metric takes no normals
    assert e.value.status == -1
    with pytest.raises(pkg.KssError) as e:
        ctx.icp_o2o(src, tgt, None, overlap=0.5, metric=7)
    assert e.value.status == -1
    with pytest.raises(pkg.KssError) as e:
        ctx.icp_o2o(src[:0], tgt, None)
    assert e.value.status == -1
    # a NULL op, NULL result, NULL clouds
    L, q, res, info = ctx.L, ctx.icp_params(), pkg.IcpResult(), np.zeros(5)
    op = pkg.o2o_params()
    sp, tp = src.ctypes.data_as(C.c_void_p), tgt.ctypes.data_as(C.c_void_p)
    ip = info.ctypes.data_as(C.c_void_p)
    assert L.kss_icp_o2o(ctx.h, sp, len(src), tp, len(tgt), None, C.byref(q), None, C.byref(res), ip) == -1
    assert L.kss_icp_o2o(ctx.h, sp, len(src), tp, len(tgt), None, C.byref(q), C.byref(op), None, ip) == -1
    assert L.kss_icp_o2o(ctx.h, None, len(src), tp, len(tgt), None, C.byref(q), C.byref(op), C.byref(res), ip) == -1
    assert L.kss_icp_o2o(ctx.h, sp, len(src), tp, len(tgt), None, None, C.byref(op), C.byref(res), ip) == -1
    # the filter alone
    idx, d2 = np.zeros(10, np.int32), np.zeros(10, F32)
    for args in ((idx, d2, 0), (idx[:0], d2[:0], 5), (idx, d2, -3)):
        with pytest.raises(pkg.KssError) as e:
            ctx.o2o_filter(*args)
        assert e.value.status == -1
    assert L.kss_o2o_filter(ctx.h, idx.ctypes.data_as(C.c_void_p), d2.ctypes.data_as(C.c_void_p), 10, 5, 1.0, None, None, None) == -1
    assert L.kss_o2o_filter(ctx.h, None, d2.ctypes.data_as(C.c_void_p), 10, 5, 1.0, None, None, ip) == -1
    w.check()
