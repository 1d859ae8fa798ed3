"""Trimmed ICP on the device (kss_trim_threshold, kss_icp_trimmed[_dev]) against the independent restatement in
tests/trim_ref.py: the exact order statistic bit for bit, the loop on three partly overlapping pairs with both metrics,
the anchors to kss_icp_p2l (bit for bit) and kss_icp at overlap 1, the invariances of test_gpu_p2l.py, and the endings."""

import numpy as np
import pytest

import trim_ref as TR

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64

PAIRS = [(1, 6000, 10.0, -0.35, 0.5), (2, 6000, 15.0, -0.2, 0.6), (3, 8000, 8.0, -0.5, 0.3)]
FULL_PAIRS = [(1, 3000, None, 5.0), (2, 2500, 1800, 10.0), (3, 2000, 2600, 15.0)]      # test_gpu_p2l.py's
OVERLAPS = [1e-6, 0.25, 0.5, 0.999, 1.0]
METRICS = [TR.POINT, TR.PLANE]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == F64 else np.uint32)


def _f32_bits(x):
    return int(np.array([x], F32).view(np.uint32)[0])


# ---- value sets of the selection: (n, rng) -> (d2 float32, max_d2) ----
def _uniform(n, rng):
    return rng.uniform(0.0, 1.0, n).astype(F32), 1.0


def _all_equal(n, rng):
    return np.full(n, 0.37, F32), 1.0


def _two_values(n, rng):
    return np.where(rng.random(n) < 0.6, F32(0.25), F32(0.5)).astype(F32), 1.0


def _denormals(n, rng):
    d = rng.integers(1, 0x800000, n).astype(np.uint32).view(F32)      # every denormal pattern
    pick = rng.integers(0, 4, n)
    d = np.where(pick == 0, F32(0.0), d)
    d = np.where(pick == 1, F32(-0.0), d)
    return d.astype(F32), 1.0


def _lowest_digit(n, rng):
    return (np.uint32(0x3e800000) + rng.integers(0, 1024, n).astype(np.uint32)).view(F32), 1.0


def _mixed(n, rng):
    d = rng.uniform(0.0, 2.0, n).astype(F32)
    d[rng.random(n) < 0.10] = F32(2.5)          # above max_d2
    d[rng.random(n) < 0.02] = np.inf
    d[rng.random(n) < 0.02] = np.nan
    d[rng.random(n) < 0.02] = F32(-0.5)
    return d, 2.0


def _no_candidate(n, rng):
    d = rng.uniform(1.5, 3.0, n).astype(F32)
    d[rng.random(n) < 0.1] = np.nan
    d[rng.random(n) < 0.1] = F32(-1.0)
    d[rng.random(n) < 0.1] = np.inf
    return d, 1.0


SETS = [_uniform, _all_equal, _two_values, _denormals, _lowest_digit, _mixed, _no_candidate]


@pytest.mark.parametrize("gen", SETS, ids=lambda g: g.__name__.strip("_"))
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257, 4096, 100000, 3000001])
def test_trim_threshold_bit_exact(ctx, n, gen):
    d2, max_d2 = gen(n, np.random.default_rng(n + 17 * SETS.index(gen)))
    assert d2.dtype == F32 and len(d2) == n
    for overlap in OVERLAPS:
        _, m, k, tau, kept = TR.threshold(d2, max_d2, overlap)
        got = ctx.trim_threshold(d2, max_d2, overlap)
        again = ctx.trim_threshold(d2, max_d2, overlap)
        assert got[0] == m and got[1] == k, (overlap, got, m, k)
        assert got[2] == float(tau) and _f32_bits(got[2]) == _f32_bits(tau), (overlap, got, tau)
        assert got[3] == int(kept.sum()), (overlap, got, int(kept.sum()))
        assert np.array_equal(_bits(got), _bits(again))
        if gen is _two_values and n >= 63 and overlap in (0.25, 0.5):
            assert got[3] > got[1]          # the rank fell inside a tie: the whole tie is kept
    if gen is _no_candidate:
        assert m == 0


def test_trim_threshold_dev_matches_host(ctx):
    import torch
    d2, max_d2 = _mixed(50000, np.random.default_rng(5))
    d = torch.from_numpy(d2).cuda()
    torch.cuda.synchronize()
    for overlap in OVERLAPS:
        assert np.array_equal(_bits(ctx.trim_threshold_dev(d.data_ptr(), len(d2), max_d2, overlap)),
                              _bits(ctx.trim_threshold(d2, max_d2, overlap)))


def test_trim_threshold_rejects_bad_overlap(pkg, ctx):
    d2 = np.ones(10, F32)
    for overlap in (0.0, -0.5, 1.0000001, float("nan")):
        with pytest.raises(pkg.KssError) as e:
            ctx.trim_threshold(d2, 1.0, overlap)
        assert e.value.status == -1


# ---- the loop ----
def _normals(ctx, tgt):
    return ctx.normals(tgt.astype(F64), 20).astype(F32)


def _partial(pkg, spec):
    src, tgt, R, t, ov = pkg.synth.make_partial_pair(*spec)
    return src, tgt, R.T, -R.T @ t


def _bumpy(pkg, pair_id, n, deg, n_src=None, t=(0.02, -0.01, 0.03)):
    axis = pkg.synth.sphere(7000 + pair_id, 1)[0]
    return pkg.synth.make_pair(pair_id, n, R=pkg.synth.rot_axis_angle(axis, np.deg2rad(deg)), t=t, shape="bumpy", n_src=n_src)


@pytest.mark.parametrize("metric", METRICS, ids=["point", "plane"])
@pytest.mark.parametrize("spec", PAIRS, ids=lambda s: "pair%d" % s[0])
def test_icp_trimmed_matches_restatement_and_recovers(pkg, ctx, O, spec, metric):
    src, tgt, R_true, t_true = _partial(pkg, spec)
    nrm = _normals(ctx, tgt) if metric == TR.PLANE else None
    got = ctx.icp_trimmed(src, tgt, nrm, overlap=0.5, metric=metric, params=ctx.icp_params(max_iterations=200), trace_cap=256)
    ref = TR.icp_trimmed(O, src, tgt, nrm, 0.5, metric, max_iterations=200)
    print("pair %d metric %d: library %d it. state %d, restatement %d it. state %d, max|T - T_ref| %.2e, vs truth %.2e / %.2e" % (
        spec[0], metric, got["iterations"], got["state"], ref["iterations"], ref["state"], np.abs(got["T"] - ref["T"]).max(),
        np.abs(got["T"][:3, :3] - R_true).max(), np.abs(got["T"][:3, 3] - t_true).max()))
    assert got["iterations"] == ref["iterations"] >= 1
    assert got["state"] == ref["state"] and got["converged"] == ref["converged"]
    # pass 0 sees the same positions on both sides: the selection agrees exactly
    g0, r0 = got["trace_trim"][0], ref["trace_trim"][0]
    assert g0[0] == r0[0] and g0[1] == r0[1] and g0[3] == r0[3]
    assert _f32_bits(g0[2]) == _f32_bits(r0[2]) and g0[2] == r0[2]
    s0, q0 = got["trace_sums"][0], ref["trace_sums"][0]
    assert s0[0] == q0[0]
    assert np.all(np.abs(s0 - q0) <= 1e-9 * np.maximum(np.abs(q0), 1.0))
    # later passes through the transforms
    assert np.abs(got["trace_Tk"] - ref["trace_Tk"]).max() <= 1e-6
    assert np.abs(got["T"] - ref["T"]).max() <= 5e-6
    assert abs(got["fitness"] - ref["fitness"]) <= 1e-9 * max(1.0, ref["fitness"])
    assert np.array_equal(got["trim_info"], got["trace_trim"][-1])
    # recovery through the library: the yardstick's bar
    assert np.abs(got["T"][:3, :3] - R_true).max() < 2e-3
    assert np.abs(got["T"][:3, 3] - t_true).max() < 2e-3


def _anchor_pairs(pkg):
    out = [_bumpy(pkg, pid, n, deg, n_src=n_src) for pid, n, n_src, deg in FULL_PAIRS]
    out.append(_partial(pkg, PAIRS[0])[:2])
    return out


@pytest.mark.parametrize("which", [0, 1, 2, 3], ids=["full1", "full2", "full3", "partial1"])
def test_plane_overlap_one_is_icp_p2l_bit_for_bit(pkg, ctx, which):
    src, tgt = _anchor_pairs(pkg)[which]
    nrm = _normals(ctx, tgt)
    a = ctx.icp_p2l(src, tgt, nrm, params=ctx.icp_params(max_iterations=60), trace_cap=64)
    b = ctx.icp_trimmed(src, tgt, nrm, overlap=1.0, metric=TR.PLANE, params=ctx.icp_params(max_iterations=60), trace_cap=64)
    assert a["iterations"] == b["iterations"] >= 1 and a["state"] == b["state"] and a["converged"] == b["converged"]
    assert np.array_equal(_bits(a["T"]), _bits(b["T"]))
    assert np.array_equal(_bits(a["trace_sums"]), _bits(b["trace_sums"]))
    assert np.array_equal(_bits(a["trace_Tk"]), _bits(b["trace_Tk"]))
    assert _bits(np.array([a["last_mse"]])) == _bits(np.array([b["last_mse"]]))
    assert _bits(np.array([a["fitness"]])) == _bits(np.array([b["fitness"]]))
    tt = b["trace_trim"]
    assert np.all(tt[:, 1] == tt[:, 0]) and np.all(tt[:, 3] == b["trace_sums"][:, 0])


@pytest.mark.parametrize("which", [0, 1, 2, 3], ids=["full1", "full2", "full3", "partial1"])
def test_point_overlap_one_follows_icp(pkg, ctx, which):
    src, tgt = _anchor_pairs(pkg)[which]
    a = ctx.icp(src, tgt, params=ctx.icp_params(max_iterations=40, fixed_iterations=1))
    b = ctx.icp_trimmed(src, tgt, None, overlap=1.0, metric=TR.POINT, params=ctx.icp_params(max_iterations=40, fixed_iterations=1),
                        trace_cap=64)
    assert a["iterations"] == b["iterations"] == 40
    print("point anchor %d: max|T - T_icp| %.2e" % (which, np.abs(a["T"] - b["T"]).max()))
    assert np.abs(a["T"] - b["T"]).max() <= 5e-6
    assert np.all(b["trace_trim"][:, 1] == b["trace_trim"][:, 0])
    assert np.all(b["trace_sums"][:, 17:] == 0.0)


@pytest.mark.parametrize("metric", METRICS, ids=["point", "plane"])
def test_icp_trimmed_engines_and_knobs_bit_identical(pkg, ctx, metric):
    src, tgt = _partial(pkg, PAIRS[1])[:2]
    nrm = _normals(ctx, tgt) if metric == TR.PLANE else None
    runs = []
    for kw in (dict(nn_mode=pkg.NN_BRUTE), dict(nn_mode=pkg.NN_GRID), dict(nn_mode=pkg.NN_AUTO),
               dict(nn_mode=pkg.NN_BRUTE, nn_sources_per_thread=1, nn_target_splits=3),
               dict(nn_mode=pkg.NN_BRUTE, nn_sources_per_thread=8, nn_target_splits=1)):
        runs.append(ctx.icp_trimmed(src, tgt, nrm, overlap=0.5, metric=metric, params=ctx.icp_params(max_iterations=40, **kw),
                                    trace_cap=64))
    a = runs[0]
    assert a["iterations"] >= 2
    for b in runs[1:]:
        assert b["iterations"] == a["iterations"] and b["state"] == a["state"]
        assert np.array_equal(_bits(b["trace_Tk"]), _bits(a["trace_Tk"]))
        assert np.array_equal(_bits(b["trace_sums"]), _bits(a["trace_sums"]))
        assert np.array_equal(_bits(b["trace_trim"]), _bits(a["trace_trim"]))
        assert np.array_equal(_bits(b["T"]), _bits(a["T"]))
        # The fitness is the NN engine's own f64 sum of d2 over all sources, added in that engine's order: the same bits under
        # the brute-force engine's knobs, and rounding apart between engines: each order is within (n - 1) * 2^-53 relative of
        # the exact sum of the non-negative terms, so two orders differ by less than 2 n 2^-53 relative (1e-12 here).  Where
        # the aligned part's d2 are small beside the rest's -- as after a trimmed registration -- the f64 sum of the floats
        # is no longer exact and the order shows in the last bit.
        assert abs(b["fitness"] - a["fitness"]) <= 2.0 * len(src) * 2.0 ** -53 * a["fitness"]
    for b in (runs[3], runs[4]):
        assert _bits(np.array([b["fitness"]])) == _bits(np.array([a["fitness"]]))
    assert _bits(np.array([runs[1]["fitness"]])) == _bits(np.array([runs[2]["fitness"]]))      # AUTO picks the cell list here


def test_icp_trimmed_computed_normals_equal_given(pkg, ctx):
    src, tgt = _partial(pkg, PAIRS[2])[:2]
    nrm = _normals(ctx, tgt)
    a = ctx.icp_trimmed(src, tgt, nrm, overlap=0.5, metric=TR.PLANE, trace_cap=64, fitness_corr=True)
    b = ctx.icp_trimmed(src, tgt, None, overlap=0.5, metric=TR.PLANE, trace_cap=64, fitness_corr=True)
    assert a["iterations"] == b["iterations"] >= 1 and a["state"] == b["state"]
    assert np.array_equal(_bits(a["trace_Tk"]), _bits(b["trace_Tk"]))
    assert np.array_equal(_bits(a["trace_trim"]), _bits(b["trace_trim"]))
    assert np.array_equal(_bits(a["T"]), _bits(b["T"]))
    assert a["fitness"] == b["fitness"]
    assert np.array_equal(a["fitness_idx"], b["fitness_idx"]) and np.array_equal(_bits(a["fitness_d2"]), _bits(b["fitness_d2"]))


@pytest.mark.parametrize("metric", METRICS, ids=["point", "plane"])
def test_icp_trimmed_dev_matches_host(pkg, ctx, metric):
    import torch
    src, tgt = _partial(pkg, PAIRS[0])[:2]
    nrm = _normals(ctx, tgt)
    h = ctx.icp_trimmed(src, tgt, nrm if metric == TR.PLANE else None, overlap=0.5, metric=metric)
    s, t, nr = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (src, tgt, nrm))
    torch.cuda.synchronize()
    for d_n in ((nr.data_ptr(), None) if metric == TR.PLANE else (None,)):
        r, info = ctx.icp_trimmed_dev(s.data_ptr(), len(src), t.data_ptr(), len(tgt), d_n, ctx.icp_params(), overlap=0.5, metric=metric)
        assert r.iterations == h["iterations"] and r.state == h["state"]
        assert np.array_equal(_bits(r.matrix()), _bits(h["T"]))
        assert r.fitness == h["fitness"]
        assert np.array_equal(_bits(info), _bits(h["trim_info"]))


# ---- endings: each leaves the context clean ----
class _Witness:
    """kss_icp and kss_icp_p2l on a fixed pair: what the context gave before must be what it gives afterwards."""

    def __init__(self, pkg, ctx):
        self.ctx = ctx
        self.src, self.tgt = _bumpy(pkg, 11, 3000, 7.0, n_src=2500)
        self.nrm = _normals(ctx, self.tgt)
        self.before = self.run()

    def run(self):
        a = self.ctx.icp(self.src, self.tgt, trace_cap=64)
        b = self.ctx.icp_p2l(self.src, self.tgt, self.nrm, trace_cap=64)
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
    nrm = _normals(ctx, tgt) if metric == TR.PLANE else None
    got = ctx.icp_trimmed(src, tgt, nrm, overlap=0.001, metric=metric)       # k = 1 < min_correspondences = 3
    assert got["state"] == 5 and got["iterations"] == 0 and not got["converged"]
    assert got["trim_info"][0] == 500 and got["trim_info"][1] == 1 and 1 <= got["trim_info"][3] < 3
    assert np.array_equal(got["T"], np.eye(4, dtype=F32))
    w.check()


def test_ending_planar_target_degenerate(pkg, ctx):
    w = _Witness(pkg, ctx)
    g = np.linspace(-1, 1, 40)
    tgt = np.stack(np.meshgrid(g, g), -1).reshape(-1, 2)
    tgt = np.concatenate([tgt, np.zeros((len(tgt), 1))], 1).astype(F32)
    src = (tgt[::2] + np.array([0.01, -0.02, 0.05])).astype(F32)
    nrm = np.tile(np.array([0, 0, 1], F32), (len(tgt), 1))
    got = ctx.icp_trimmed(src, tgt, nrm, overlap=0.5, metric=TR.PLANE)
    assert got["state"] == pkg.STATE_DEGENERATE and not got["converged"] and got["iterations"] == 0
    assert np.isfinite(got["T"]).all()
    w.check()


@pytest.mark.parametrize("metric", METRICS, ids=["point", "plane"])
def test_ending_no_candidate(pkg, ctx, metric):
    w = _Witness(pkg, ctx)
    src, tgt = _bumpy(pkg, 9, 2000, 5.0)
    nrm = _normals(ctx, tgt) if metric == TR.PLANE else None
    got = ctx.icp_trimmed(src + np.float32(100.0), tgt, nrm, overlap=0.5, metric=metric)
    assert got["state"] == 5 and got["iterations"] == 0 and not got["converged"]
    assert np.array_equal(got["trim_info"], np.zeros(4))
    assert np.array_equal(got["T"], np.eye(4, dtype=F32))
    w.check()


def test_ending_argument_errors(pkg, ctx):
    w = _Witness(pkg, ctx)
    src, tgt = _bumpy(pkg, 10, 1000, 5.0)
    nrm = _normals(ctx, tgt)
    p = ctx.icp_params()
    p.allreduce = pkg.binding.ALLREDUCE_FN(lambda user, values, n: 0)
    with pytest.raises(pkg.KssError) as e:
        ctx.icp_trimmed(src, tgt, nrm, overlap=0.5, metric=TR.PLANE, params=p)
    assert e.value.status == -1
    w.check()
    for overlap in (0.0, -0.5, 1.0000001, float("nan")):
        with pytest.raises(pkg.KssError) as e:
            ctx.icp_trimmed(src, tgt, None, overlap=overlap, metric=TR.POINT)
        assert e.value.status == -1
    w.check()
    with pytest.raises(pkg.KssError) as e:
        ctx.icp_trimmed(src, tgt, nrm, overlap=0.5, metric=TR.POINT)
    assert e.value.status == -1
    w.check()
