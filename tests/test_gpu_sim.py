"""Similarity ICP on the device (kss_sim_sums, kss_icp_sim; include/kssicp.h) against the independent restatement
in tests/sim_ref.py: the record, the loop on two full and two partly overlapping pairs of wrong scale under the three NN engines,
the truth (and that the rigid step misses it), the anchor to kss_icp_trimmed bit for bit, the clamp in the loop and the endings."""
import functools

import numpy as np
import pytest

import sim_ref as SR
import trim_ref as TR

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SCENES = ["full0.9", "full1.1", "partial0.95", "partial1.05"]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == F64 else np.uint32)


def _f64_bits(x):
    return int(np.array([x], F64).view(np.uint64)[0])


@functools.lru_cache(maxsize=None)
def _scene(name):
    import __graft_entry__ as graft
    pkg = graft.load_package()
    kind, v = ("full", float(name[4:])) if name.startswith("full") else ("partial", float(name[7:]))
    return SR.full_scene(pkg, v) if kind == "full" else SR.partial_scene(pkg, v)


@functools.lru_cache(maxsize=None)
def _ref(name, scale_min=0.5, scale_max=2.0):
    """the restatement's run of a scene, computed once and shared (never modified)"""
    import __graft_entry__ as graft
    src, tgt, _, ov = _scene(name)
    return SR.icp_sim(graft.load_oracle(), src, tgt, ov, scale_min, scale_max)


@functools.lru_cache(maxsize=None)
def _ref_rigid(name):
    import __graft_entry__ as graft
    src, tgt, _, ov = _scene(name)
    return TR.icp_trimmed(graft.load_oracle(), src, tgt, None, ov, TR.POINT)


# ---- the record ----
@pytest.mark.parametrize("n", [1, 255, 257, 1000, 2048 * 256 + 300])
def test_record(pkg, ctx, n):
    import torch
    rng = np.random.default_rng(n)
    nt = 777
    tgt = rng.uniform(-1, 1, (nt, 3)).astype(F32)
    idx = rng.integers(0, nt, n).astype(np.int32)
    src = (tgt[idx] + rng.normal(size=(n, 3)) * 0.05).astype(F32)
    if n > 1:
        far = rng.random(n) < 0.1
        src[far] += F32(0.9)                      # above max_d2
        out = rng.random(n) < 0.05
        idx[out] = np.where(rng.random(int(out.sum())) < 0.5, -1 - rng.integers(0, 5, int(out.sum())), nt + rng.integers(0, 5, int(out.sum())))
        idx[-1] = nt                              # outside the target
        idx[0] = 0
    max_d2 = 0.04
    ref = SR.sums_for(src, tgt, idx, max_d2)
    s, t, i = (torch.from_numpy(x).cuda() for x in (src, tgt, idx))
    torch.cuda.synchronize()
    got = ctx.sim_sums_dev(s.data_ptr(), t.data_ptr(), i.data_ptr(), n, nt, max_d2)
    again = ctx.sim_sums_dev(s.data_ptr(), t.data_ptr(), i.data_ptr(), n, nt, max_d2)
    host = ctx.sim_sums(src, tgt, idx, max_d2)
    l2, _ = ctx.robust_sums(src, tgt, None, idx, max_d2, rp=pkg.robust_params(pkg.LOSS_L2, pkg.METRIC_POINT, scale=1.0))
    print("n %d: kept %d of %d, [17] %.17g ref %.17g" % (n, got[0], n, got[17], ref[17]))
    assert np.array_equal(_bits(got), _bits(again)) and np.array_equal(_bits(got), _bits(host))
    assert np.array_equal(_bits(got[:17]), _bits(l2[:17]))
    assert got[0] == ref[0] and (n == 1 or 0 < got[0] < n)
    assert abs(got[17] - ref[17]) <= 1e-9 * abs(ref[17])
    assert np.all(np.abs(got[:17] - ref[:17]) <= 1e-9 * np.maximum(np.abs(ref[:17]), 1.0))
    assert got[18] == 0.0 and got[19] == 0.0


# ---- the loop ----
def _check_against_ref(got, ref):
    assert got["iterations"] == ref["iterations"] >= 1
    assert got["state"] == ref["state"] and got["converged"] == ref["converged"]
    assert np.abs(got["trace_Tk"] - ref["trace_Tk"]).max() <= 1e-6
    assert np.abs(got["T"] - ref["T"]).max() <= 5e-6
    assert abs(got["fitness"] - ref["fitness"]) <= 1e-9 * max(1.0, ref["fitness"])
    assert abs(got["scale"] - ref["scale"]) <= 1e-6 * ref["scale"]
    assert np.array_equal(got["sim_info"], got["trace_sim"][-1]) and got["scale"] == got["sim_info"][5]
    # pass 0 sees the same positions on both sides: the selection agrees exactly, the sums to test_gpu_trim.py's bar
    g0, r0 = got["trace_sim"][0], ref["trace_sim"][0]
    assert np.array_equal(g0[:4], r0[:4])
    s0, q0 = got["trace_sums"][0], ref["trace_sums"][0]
    assert np.all(np.abs(s0 - q0) <= 1e-9 * np.maximum(np.abs(q0), 1.0))


@pytest.mark.parametrize("mode", ["brute", "grid", "auto"])
@pytest.mark.parametrize("name", SCENES)
def test_loop_matches_restatement(pkg, ctx, name, mode):
    src, tgt, truth, ov = _scene(name)
    nn = {"brute": pkg.NN_BRUTE, "grid": pkg.NN_GRID, "auto": pkg.NN_AUTO}[mode]
    got = ctx.icp_sim(src, tgt, sp=pkg.sim_params(overlap=ov), params=ctx.icp_params(nn_mode=nn), trace_cap=256)
    ref = _ref(name)
    print("%s %s: library %d it. state %d scale %.9f, restatement %d it. state %d scale %.9f, max|T - T_ref| %.2e" % (
        name, mode, got["iterations"], got["state"], got["scale"], ref["iterations"], ref["state"], ref["scale"],
        np.abs(got["T"] - ref["T"]).max()))
    _check_against_ref(got, ref)


@pytest.mark.parametrize("name", SCENES)
def test_similarity_reaches_the_truth_and_the_rigid_step_does_not(pkg, ctx, name):
    src, tgt, truth, ov = _scene(name)
    got = ctx.icp_sim(src, tgt, sp=pkg.sim_params(overlap=ov))
    rigid = ctx.icp_trimmed(src, tgt, None, overlap=ov, metric=pkg.METRIC_POINT)
    ref, ref_rigid = _ref(name), _ref_rigid(name)
    err = [np.abs(x["T"][:3].astype(F64) - truth).max() for x in (got, ref, rigid, ref_rigid)]
    print("%s: max|[sR | t] - truth| similarity %.2e (restatement %.2e) in %d passes, scale %.6f; rigid %.2e (restatement %.2e) in %d passes" % (
        name, err[0], err[1], got["iterations"], got["scale"], err[2], err[3], rigid["iterations"]))
    assert err[0] <= 1e-3 and err[1] <= 1e-3
    assert err[2] > 1e-2 and err[3] > 1e-2


@pytest.mark.parametrize("name", ["full0.9", "partial1.05"])
def test_unit_bounds_are_icp_trimmed_bit_for_bit(pkg, ctx, name):
    src, tgt, _, ov = _scene(name)
    a = ctx.icp_trimmed(src, tgt, None, overlap=ov, metric=pkg.METRIC_POINT, trace_cap=256)
    b = ctx.icp_sim(src, tgt, sp=pkg.sim_params(overlap=ov, scale_min=1.0, scale_max=1.0), trace_cap=256)
    assert a["iterations"] == b["iterations"] >= 2 and a["state"] == b["state"] and a["converged"] == b["converged"]
    assert np.array_equal(_bits(a["T"]), _bits(b["T"]))
    assert _f64_bits(a["last_mse"]) == _f64_bits(b["last_mse"])
    assert np.array_equal(_bits(a["trace_Tk"]), _bits(b["trace_Tk"]))
    assert np.array_equal(_bits(a["trace_sums"][:, :17]), _bits(b["trace_sums"][:, :17]))
    assert _f64_bits(a["fitness"]) == _f64_bits(b["fitness"])
    assert np.array_equal(_bits(a["trace_trim"]), _bits(b["trace_sim"][:, :4]))
    assert np.all(b["trace_sim"][:, 4:] == 1.0) and np.all(b["trace_sums"][:, 17] > 0.0) and np.all(b["trace_sums"][:, 18:] == 0.0)


@pytest.mark.parametrize("name,lo,hi", [("full0.9", 0.5, 1.05), ("full1.1", 0.95, 2.0)], ids=["max1.05", "min0.95"])
def test_clamp_in_the_loop(pkg, ctx, name, lo, hi):
    src, tgt, _, ov = _scene(name)
    got = ctx.icp_sim(src, tgt, sp=pkg.sim_params(overlap=ov, scale_min=lo, scale_max=hi), trace_cap=256)
    ref = _ref(name, lo, hi)
    acc = got["trace_sim"][:, 5]
    print("%s in [%g, %g]: %d passes, s_acc %s" % (name, lo, hi, got["iterations"], acc))
    assert np.all(acc <= hi) and np.all(acc >= lo)
    assert acc[-1] == (hi if name == "full0.9" else lo) and got["scale"] == acc[-1]
    _check_against_ref(got, ref)


# ---- endings: each leaves the context clean ----
class _Witness:
    def __init__(self, pkg, ctx):
        self.ctx, self.pkg = ctx, pkg
        self.src, self.tgt, _, self.ov = _scene("partial0.95")
        self.before = self.run()

    def run(self):
        return self.ctx.icp_sim(self.src, self.tgt, sp=self.pkg.sim_params(overlap=self.ov), trace_cap=64)

    def check(self):
        x, y = self.before, self.run()
        assert x["iterations"] == y["iterations"] and x["state"] == y["state"]
        for k in ("T", "trace_sums", "trace_Tk", "trace_sim"):
            assert np.array_equal(_bits(x[k]), _bits(y[k]))
        assert _f64_bits(x["fitness"]) == _f64_bits(y["fitness"])
        _check_against_ref(y, _ref("partial0.95"))


def test_ending_too_few_sources(pkg, ctx):
    w = _Witness(pkg, ctx)
    tgt = _scene("full0.9")[1]
    src = (tgt[:2] + F32(0.01)).astype(F32)
    got = ctx.icp_sim(src, tgt, params=ctx.icp_params(min_correspondences=3))
    assert got["state"] == 5 and got["iterations"] == 0 and not got["converged"]
    assert np.array_equal(got["T"], np.eye(4, dtype=F32))
    assert np.array_equal(got["sim_info"][[0, 1, 3, 4, 5]], np.array([2.0, 2.0, 2.0, 0.0, 1.0]))
    w.check()


def test_ending_identical_sources_degenerate(pkg, ctx):
    w = _Witness(pkg, ctx)
    tgt = _scene("full0.9")[1]
    src = np.tile(np.array([0.5, 0.25, -0.75], F32), (64, 1))       # dyadic: every sum is exact and var is exactly 0
    got = ctx.icp_sim(src, tgt)
    assert got["state"] == pkg.STATE_DEGENERATE and got["iterations"] == 0 and not got["converged"]
    assert np.array_equal(got["T"], np.eye(4, dtype=F32))
    assert got["sim_info"][3] == 64 and got["sim_info"][4] == 0.0 and got["sim_info"][5] == 1.0
    w.check()


def test_ending_argument_errors(pkg, ctx):
    w = _Witness(pkg, ctx)
    src, tgt = w.src[:500], w.tgt
    bad = [dict(overlap=0.0), dict(overlap=-0.5), dict(overlap=1.0000001), dict(overlap=float("nan")),
           dict(scale_min=0.0), dict(scale_min=-1.0), dict(scale_min=1.5), dict(scale_min=float("nan")),
           dict(scale_max=0.9), dict(scale_max=float("inf")), dict(scale_max=float("nan"))]
    for kw in bad:
        with pytest.raises(pkg.KssError) as e:
            ctx.icp_sim(src, tgt, sp=pkg.sim_params(**kw))
        assert e.value.status == -1, kw
    p = ctx.icp_params()
    p.allreduce = pkg.binding.ALLREDUCE_FN(lambda user, values, n: 0)
    with pytest.raises(pkg.KssError) as e:
        ctx.icp_sim(src, tgt, params=p)
    assert e.value.status == -1
    with pytest.raises(pkg.KssError) as e:
        ctx.icp_sim(src[:0], tgt)
    assert e.value.status == -1
    L = pkg.load_library()
    res = pkg.IcpResult()
    import ctypes as C
    s = np.ascontiguousarray(src)
    t = np.ascontiguousarray(tgt)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    ip = ctx.icp_params()
    assert L.kss_icp_sim(ctx.h, vp(s), len(s), vp(t), len(t), C.byref(ip), None, C.byref(res), None) == -1      # NULL sp
    assert L.kss_icp_sim(ctx.h, vp(s), len(s), vp(t), len(t), C.byref(ip), C.byref(pkg.sim_params()), None, None) == -1      # NULL res
    w.check()
