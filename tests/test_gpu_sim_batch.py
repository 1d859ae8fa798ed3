"""Batched similarity ICP on the device (kss_icp_sim_batch; include/kssicp.h): every pair's record is its
single-pair call's bit for bit -- in the batch as given, reversed, split over two calls, through a first offset that is not 0, under
the three NN engines -- a pair that ends at once leaves the others untouched, and the grid-stride wrap of the batch walk."""
import ctypes as C

import numpy as np
import pytest

import sim_ref as SR

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == F64 else np.uint32)


def _f64_bits(x):
    return int(np.array([x], F64).view(np.uint64)[0])


def _fitness_bound(ns, ref):
    # test_gpu_trim.py's bound for two summation orders of the NN engines' f64 sum of d2 over all sources (the header's "to the
    # rounding of the NN engine's own summation order"): two orders differ by less than 2 n 2^-53 relative
    return 2.0 * ns * 2.0 ** -53 * abs(ref)


def _pairs(pkg):
    """(src, tgt, overlap) of five pairs: 300, 1000, 2500 points of different true scales, the partial scene on a 3000-point model
    with its source scaled about its centroid, and a 2-point pair that ends at once (min_correspondences = 3)."""
    out = []
    for pid, n, deg, scale, ov in [(21, 300, 5.0, 0.93, 1.0), (22, 1000, 8.0, 1.08, 0.9), (23, 2500, 6.0, 0.88, 1.0)]:
        axis = pkg.synth.sphere(7000 + pid, 1)[0]
        src, tgt = pkg.synth.make_pair(pid, n, R=pkg.synth.rot_axis_angle(axis, np.deg2rad(deg)), scale=scale, t=(0.02, -0.01, 0.03),
                                       shape="bumpy")
        out.append((src, tgt, ov))
    src, tgt, R, t, ov = pkg.synth.make_partial_pair(2, 3000, 10.0, -0.35, 0.5)
    c = src.astype(F64).mean(0)
    out.append(((c + 1.05 * (src.astype(F64) - c)).astype(F32), tgt, 0.8 * ov))
    out.append(((out[0][1][:2] + F32(0.01)).astype(F32), out[0][1], 0.7))
    return out


def _pack(pairs, order, pad=0):
    """packed clouds and offsets of pairs[order]; pad: that many foreign points (and one foreign pair's worth of offset) in front"""
    srcs, tgts, so, to = [], [], [pad], [pad]
    if pad:
        junk = np.full((pad, 3), 7.5, F32)
        srcs.append(junk); tgts.append(junk)
    for i in order:
        srcs.append(pairs[i][0]); tgts.append(pairs[i][1])
        so.append(so[-1] + len(pairs[i][0])); to.append(to[-1] + len(pairs[i][1]))
    return np.concatenate(srcs), np.array(so, np.int64), np.concatenate(tgts), np.array(to, np.int64)


def _check(r, info, single, ns, pair_id):
    assert r.pair_id == pair_id
    assert r.iterations == single["iterations"] and r.state == single["state"] and bool(r.converged) == single["converged"]
    assert np.array_equal(_bits(r.matrix()), _bits(single["T"]))
    assert _f64_bits(r.last_mse) == _f64_bits(single["last_mse"])
    assert np.array_equal(_bits(info), _bits(single["sim_info"]))
    assert abs(r.fitness - single["fitness"]) <= _fitness_bound(ns, single["fitness"])


@pytest.mark.parametrize("mode", ["brute", "grid", "auto"])
def test_mixed_batch_is_the_single_calls_bit_for_bit(pkg, ctx, mode):
    nn = {"brute": pkg.NN_BRUTE, "grid": pkg.NN_GRID, "auto": pkg.NN_AUTO}[mode]
    pairs = _pairs(pkg)
    sp = pkg.sim_params(overlap=0.5)       # (every pair has its own entry in overlaps)
    singles = [ctx.icp_sim(s, t, sp=pkg.sim_params(overlap=ov), params=ctx.icp_params(nn_mode=nn), trace_cap=128) for s, t, ov in pairs]
    assert singles[4]["state"] == 5 and singles[4]["iterations"] == 0
    assert all(x["iterations"] >= 3 and x["converged"] for x in singles[:4])
    assert len({round(x["scale"], 2) for x in singles[:4]}) == 4         # four different scales were found

    def run(order, pad=0, trace=0):
        s, so, t, to = _pack(pairs, order, pad)
        ov = np.array([pairs[i][2] for i in order])
        return ctx.icp_sim_batch(s, so, t, to, overlaps=ov, sp=sp, params=ctx.icp_params(nn_mode=nn), trace_cap=trace)

    # as given (pair 0's traces), reversed, split over two calls, through a first offset that is not 0
    for order, pad, trace in [([0, 1, 2, 3, 4], 0, 128), ([4, 3, 2, 1, 0], 0, 0), ([0, 1], 0, 0), ([2, 3, 4], 0, 0), ([1, 4, 3], 11, 0)]:
        res, info, extra = run(order, pad, trace)
        for k, i in enumerate(order):
            _check(res[k], info[k], singles[i], len(pairs[i][0]), k)
        if trace:
            for key in ("trace_sums", "trace_Tk", "trace_sim"):
                assert np.array_equal(_bits(extra[key]), _bits(singles[order[0]][key])), key
    # the pair that ends at once leaves the others untouched: the batch without it gives the same records
    res_a, info_a, _ = run([0, 1, 2, 3, 4])
    res_b, info_b, _ = run([0, 1, 2, 3])
    for k in range(4):
        assert np.array_equal(_bits(res_a[k].matrix()), _bits(res_b[k].matrix())) and res_a[k].iterations == res_b[k].iterations
        assert _f64_bits(res_a[k].fitness) == _f64_bits(res_b[k].fitness)
        assert np.array_equal(_bits(info_a[k]), _bits(info_b[k]))


def test_grid_stride_wrap_of_the_batch_walk(pkg, ctx):
    # stream_blocks caps the rows of a pair at 2048: a pair of 2048 * 256 + 512 sources is the first size class whose walk wraps
    rng = np.random.default_rng(3)
    axis = pkg.synth.sphere(7031, 1)[0]
    small = pkg.synth.make_pair(31, 300, R=pkg.synth.rot_axis_angle(axis, np.deg2rad(4.0)), scale=0.95, t=(0.01, 0.0, -0.01), shape="bumpy")
    tgt = pkg.synth.bumpy(1032, 4000).astype(F32)
    n = 524800
    big = (0.97 * tgt[rng.integers(0, len(tgt), n)].astype(F64) + rng.normal(size=(n, 3)) * 2e-3 + 0.01).astype(F32)
    pairs = [(small[0], small[1], 1.0), (big, tgt, 0.9)]
    p = dict(max_iterations=2)
    singles = [ctx.icp_sim(s, t, sp=pkg.sim_params(overlap=ov), params=ctx.icp_params(**p), trace_cap=4) for s, t, ov in pairs]
    assert all(x["iterations"] == 2 for x in singles)
    for order in ([0, 1], [1, 0]):
        s, so, t, to = _pack(pairs, order)
        res, info, extra = ctx.icp_sim_batch(s, so, t, to, overlaps=np.array([pairs[i][2] for i in order]), params=ctx.icp_params(**p),
                                             trace_cap=4)
        for k, i in enumerate(order):
            _check(res[k], info[k], singles[i], len(pairs[i][0]), k)
        for key in ("trace_sums", "trace_Tk", "trace_sim"):
            assert np.array_equal(_bits(extra[key]), _bits(singles[order[0]][key])), key


def test_batch_refusals_leave_the_context_usable(pkg, ctx):
    pairs = _pairs(pkg)[:2]
    s, so, t, to = _pack(pairs, [0, 1])
    before = ctx.icp_sim_batch(s, so, t, to)
    L = pkg.load_library()
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    res = (pkg.IcpResult * 2)()
    rp = C.cast(res, C.c_void_p)
    ip = ctx.icp_params()
    good = pkg.sim_params()

    def call(so_=so, to_=to, npairs=2, p=ip, sp=good, ov=None, results=rp):
        return L.kss_icp_sim_batch(ctx.h, vp(s), vp(so_), vp(t), vp(to_), npairs, C.byref(p) if p is not None else None,
                                   C.byref(sp) if sp is not None else None, vp(ov), results, None)

    assert call(sp=None) == -1 and call(results=None) == -1 and call(so_=None) == -1 and call(to_=None) == -1 and call(p=None) == -1
    assert call(npairs=0) == -1 and call(npairs=-3) == -1
    empty = so.copy(); empty[1] = empty[0]
    assert call(so_=empty) == -1
    for bad in (0.0, 1.5, float("nan")):
        assert call(ov=np.array([0.5, bad])) == -1
        assert call(sp=pkg.sim_params(overlap=bad)) == -1
    for kw in (dict(scale_min=0.0), dict(scale_min=1.1), dict(scale_max=0.99), dict(scale_max=float("inf")), dict(scale_min=float("nan"))):
        assert call(sp=pkg.sim_params(**kw)) == -1
    pa = ctx.icp_params()
    pa.allreduce = pkg.binding.ALLREDUCE_FN(lambda user, values, n: 0)
    assert call(p=pa) == -1
    after = ctx.icp_sim_batch(s, so, t, to)
    for x, y in zip(before[0], after[0]):
        assert np.array_equal(_bits(x.matrix()), _bits(y.matrix())) and x.iterations == y.iterations
        assert _f64_bits(x.fitness) == _f64_bits(y.fitness)
    assert np.array_equal(_bits(before[1]), _bits(after[1]))
