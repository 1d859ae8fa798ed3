"""One-to-one ICP for many pairs per call (kss_o2o_filter_batch, kss_icp_o2o_batch[_dev]): every segment of the
batched filter equals the single call on it, and every pair's record of the batched loop is the single-pair call's bit for bit --
in any order, split over calls, through offsets that do not start at 0, under both NN engines -- with a pair that ends early
beside pairs that go on, and the pair above the row cap of the existing batch suites."""

import numpy as np
import pytest

import o2o_ref as OR

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
METRICS = [OR.POINT, OR.PLANE]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == F64 else np.uint32)


def _f64_bits(x):
    return int(np.array([x], F64).view(np.uint64)[0])


def _normals(ctx, tgt):
    return ctx.normals(tgt.astype(F64), 20).astype(F32)


def _bumpy(pkg, pair_id, n, deg, n_src=None, t=(0.02, -0.01, 0.03)):
    axis = pkg.synth.sphere(7000 + pair_id, 1)[0]
    return pkg.synth.make_pair(pair_id, n, R=pkg.synth.rot_axis_angle(axis, np.deg2rad(deg)), t=t, shape="bumpy", n_src=n_src)


# ---- the filter ----
def test_filter_batch_equals_single_calls(pkg, ctx):
    rng = np.random.default_rng(77)
    sizes = [1, 64, 65, 257, 4096, 300]
    nts = np.array([1, 16, 20, 64, 1000, 50], np.int64)
    idx, d2 = [], []
    for s, (n, nt) in enumerate(zip(sizes, nts)):
        i = rng.integers(-1, nt + 1, n).astype(np.int32)          # (-1 and nt: no candidates)
        d = rng.choice(np.array([0.0, -0.0, 0.125, 0.25, 0.5, 0.75, 1.5, np.nan], F32), n).astype(F32)
        if s == 3:
            i[:] = 7                                             # one segment entirely on one target
            d = rng.uniform(0.0, 1.0, n).astype(F32)
        idx.append(i); d2.append(d)
    pad = 5                                                       # offsets that do not start at 0, and a tail nobody owns
    off = (pad + np.concatenate([[0], np.cumsum(sizes)])).astype(np.int64)
    idx_all = np.concatenate([np.full(pad, 3, np.int32)] + idx + [np.full(pad, 3, np.int32)])
    d2_all = np.concatenate([np.full(pad, 0.5, F32)] + d2 + [np.full(pad, 0.5, F32)])
    got_i, got_d, info = ctx.o2o_filter_batch(idx_all, d2_all, off, nts, max_d2=1.0)
    assert np.array_equal(got_i[:pad], idx_all[:pad]) and np.array_equal(got_i[-pad:], idx_all[-pad:])
    assert np.array_equal(_bits(got_d[:pad]), _bits(d2_all[:pad])) and np.array_equal(_bits(got_d[-pad:]), _bits(d2_all[-pad:]))
    for s in range(len(sizes)):
        one_i, one_d, m, u = ctx.o2o_filter(idx[s], d2[s], int(nts[s]), 1.0)
        ref_i, ref_d, rm, ru = OR.filter(idx[s], d2[s], int(nts[s]), 1.0)
        assert (m, u) == (rm, ru) == (int(info[s, 0]), int(info[s, 1])), s
        seg = slice(int(off[s]), int(off[s + 1]))
        assert np.array_equal(got_i[seg], one_i) and np.array_equal(one_i, ref_i), s
        assert np.array_equal(_bits(got_d[seg]), _bits(one_d)) and np.array_equal(_bits(one_d), _bits(ref_d)), s
    assert info[3, 0] == sizes[3] and info[3, 1] == 1
    # any order of the segments gives every segment the same answer
    order = [4, 0, 3, 5, 1, 2]
    off2 = np.concatenate([[0], np.cumsum([sizes[s] for s in order])]).astype(np.int64)
    got_i2, got_d2, info2 = ctx.o2o_filter_batch(np.concatenate([idx[s] for s in order]), np.concatenate([d2[s] for s in order]), off2,
                                                 nts[order], max_d2=1.0)
    for q, s in enumerate(order):
        seg, seg2 = slice(int(off[s]), int(off[s + 1])), slice(int(off2[q]), int(off2[q + 1]))
        assert np.array_equal(got_i2[seg2], got_i[seg]) and np.array_equal(_bits(got_d2[seg2]), _bits(got_d[seg]))
        assert np.array_equal(info2[q], info[s])
    with pytest.raises(pkg.KssError) as e:
        ctx.o2o_filter_batch(idx_all, d2_all, off, np.array([1, 16, 20, 0, 1000, 50], np.int64))      # a segment without targets
    assert e.value.status == -1


# ---- the loop ----
class Pair:
    """One pair with its normals and, computed once and kept, the single-pair calls' results on it."""

    def __init__(self, ctx, src, tgt):
        self.ctx = ctx
        self.src, self.tgt = np.ascontiguousarray(src, F32), np.ascontiguousarray(tgt, F32)
        self.nrm = _normals(ctx, self.tgt)
        self._single = {}

    def single(self, metric, overlap, trace=False, **kw):
        key = (metric, overlap, trace, tuple(sorted(kw.items())))
        if key not in self._single:
            self._single[key] = self.ctx.icp_o2o(self.src, self.tgt, self.nrm if metric == OR.PLANE else None, overlap=overlap,
                                                 metric=metric, params=self.ctx.icp_params(**kw), trace_cap=256 if trace else 0)
        return self._single[key]


def _pack(pairs, pad=0):
    so = (pad + np.concatenate([[0], np.cumsum([len(p.src) for p in pairs])])).astype(np.int64)
    to = (2 * pad + np.concatenate([[0], np.cumsum([len(p.tgt) for p in pairs])])).astype(np.int64)
    z = lambda n: [np.full((n, 3), 9.0, F32)] if n else []
    return (np.concatenate(z(pad) + [p.src for p in pairs] + z(pad)), so, np.concatenate(z(2 * pad) + [p.tgt for p in pairs]), to,
            np.concatenate(z(2 * pad) + [p.nrm for p in pairs]))


def _run_batch(ctx, pairs, metric, overlaps, trace=False, pad=0, **kw):
    s, so, t, to, nr = _pack(pairs, pad)
    return ctx.icp_o2o_batch(s, so, t, to, nr if metric == OR.PLANE else None, overlaps=overlaps, metric=metric,
                             params=ctx.icp_params(**kw), trace_cap=256 if trace else 0)


def _check_record(r, single, ns, pair_id, info):
    assert r.pair_id == pair_id
    assert r.iterations == single["iterations"] and r.state == single["state"] and bool(r.converged) == single["converged"]
    assert np.array_equal(_bits(r.matrix()), _bits(single["T"]))
    assert _f64_bits(r.last_mse) == _f64_bits(single["last_mse"])
    # test_gpu_trim.py's bound for two summation orders of the NN engines' f64 sum of d2 over all sources
    assert abs(r.fitness - single["fitness"]) <= 2.0 * ns * 2.0 ** -53 * single["fitness"]
    assert np.array_equal(_bits(info), _bits(single["o2o_info"]))


OVERLAPS = [1.0, 0.9, 0.5, 1.0, 0.7]


@pytest.fixture(scope="module")
def five(pkg, ctx):
    """Five pairs of 300 to 3000 points: three partly overlapping ones, where sources share targets, and two full ones."""
    out = []
    for spec in ((41, 1200, 10.0, -0.35, 0.5), (42, 3600, 12.0, -0.2, 0.6), (43, 600, 8.0, -0.5, 0.3)):
        src, tgt = pkg.synth.make_partial_pair(*spec)[:2]
        out.append(Pair(ctx, src, tgt))
    out.append(Pair(ctx, *_bumpy(pkg, 44, 3000, 6.0, n_src=2100)))
    out.append(Pair(ctx, *_bumpy(pkg, 45, 900, 9.0, n_src=300)))
    assert min(len(p.src) for p in out) == 300 and max(max(len(p.src), len(p.tgt)) for p in out) <= 3000
    return out


@pytest.mark.parametrize("nn_mode", ["brute", "grid"])
@pytest.mark.parametrize("metric", METRICS, ids=["point", "plane"])
def test_o2o_batch_equals_single_calls(pkg, ctx, five, metric, nn_mode):
    mode = pkg.NN_BRUTE if nn_mode == "brute" else pkg.NN_GRID
    kw = dict(max_iterations=60, nn_mode=mode)
    ov = np.array(OVERLAPS, F64)
    singles = [p.single(metric, float(o), trace=(i == 0), max_iterations=60, nn_mode=pkg.NN_BRUTE) for i, (p, o) in enumerate(zip(five, ov))]
    assert all(s["iterations"] >= 2 for s in singles)
    assert sum(s["o2o_info"][0] < s["o2o_info"][4] for s in singles) >= 3          # the rejection is live in the batch
    # as packed, with pair 0's traces
    res, info, extra = _run_batch(ctx, five, metric, ov, trace=True, **kw)
    for i, (r, p) in enumerate(zip(res, five)):
        _check_record(r, singles[i], len(p.src), i, info[i])
    assert np.array_equal(_bits(extra["trace_sums"]), _bits(singles[0]["trace_sums"]))
    assert np.array_equal(_bits(extra["trace_Tk"]), _bits(singles[0]["trace_Tk"]))
    assert np.array_equal(_bits(extra["trace_o2o"]), _bits(singles[0]["trace_o2o"]))
    # reversed
    res, info, _ = _run_batch(ctx, five[::-1], metric, ov[::-1].copy(), **kw)
    for i, (r, p) in enumerate(zip(res, five[::-1])):
        _check_record(r, singles[4 - i], len(p.src), i, info[i])
    # split over two calls
    for lo, hi in ((0, 2), (2, 5)):
        res, info, _ = _run_batch(ctx, five[lo:hi], metric, ov[lo:hi].copy(), **kw)
        for i, (r, p) in enumerate(zip(res, five[lo:hi])):
            _check_record(r, singles[lo + i], len(p.src), i, info[i])
    # through offsets that do not start at 0
    res, info, _ = _run_batch(ctx, five, metric, ov, pad=37, **kw)
    for i, (r, p) in enumerate(zip(res, five)):
        _check_record(r, singles[i], len(p.src), i, info[i])


@pytest.mark.parametrize("metric", METRICS, ids=["point", "plane"])
def test_o2o_batch_dev_and_default_overlap(pkg, ctx, five, metric):
    import torch
    pairs = five[:3]
    s, so, t, to, nr = _pack(pairs)
    ds, dt, dn = (torch.from_numpy(x).cuda() for x in (s, t, nr))
    torch.cuda.synchronize()
    res, info = ctx.icp_o2o_batch_dev(ds.data_ptr(), so, dt.data_ptr(), to, dn.data_ptr() if metric == OR.PLANE else None,
                                      ctx.icp_params(max_iterations=60), overlaps=None, overlap=0.9, metric=metric)
    for i, (r, p) in enumerate(zip(res, pairs)):
        _check_record(r, p.single(metric, 0.9, max_iterations=60), len(p.src), i, info[i])


@pytest.mark.parametrize("metric", METRICS, ids=["point", "plane"])
def test_one_pair_ends_early_the_others_go_on(pkg, ctx, five, metric):
    far = Pair(ctx, five[4].src + np.float32(100.0), five[4].tgt)          # no candidate in its first pass
    pairs = [five[0], far, five[3]]
    ov = np.array([1.0, 1.0, 0.7], F64)
    res, info, _ = _run_batch(ctx, pairs, metric, ov, max_iterations=60)
    assert res[1].state == 5 and res[1].iterations == 0 and not res[1].converged
    assert np.array_equal(info[1], np.zeros(5)) and np.array_equal(res[1].matrix(), np.eye(4, dtype=F32))
    for i in (0, 2):
        single = pairs[i].single(metric, float(ov[i]), max_iterations=60)
        assert single["iterations"] >= 2
        _check_record(res[i], single, len(pairs[i].src), i, info[i])
    _check_record(res[1], far.single(metric, 1.0, max_iterations=60), len(far.src), 1, info[1])


def test_pair_above_the_row_cap(pkg, ctx):
    """stream_blocks saturates at 2048 rows: for a pair of more than 2048 * 256 sources the grid-stride term of the filter's walk
    and of the rows walk is live.  Two passes of both metrics against the single-pair calls; 524 800 sources on at most 3000
    targets is also the filter's contention at scale."""
    src, tgt = _bumpy(pkg, 60, 524800, 5.0)
    big = Pair(ctx, src, tgt[::175])
    small = Pair(ctx, *_bumpy(pkg, 61, 2000, 7.0, n_src=300))
    assert len(big.src) == 524800 > 2048 * 256 and len(big.tgt) <= 3000 and len(small.src) == 300
    pairs = [small, big]
    ov = np.array([0.6, 0.8], F64)
    for metric in METRICS:
        res, info, _ = _run_batch(ctx, pairs, metric, ov, max_iterations=2)
        for i, (r, pr) in enumerate(zip(res, pairs)):
            single = pr.single(metric, float(ov[i]), max_iterations=2)
            assert single["iterations"] == 2
            _check_record(r, single, len(pr.src), i, info[i])
        assert info[1, 0] <= len(big.tgt) < info[1, 4] == len(big.src)


def test_batch_argument_errors(pkg, ctx, five):
    import ctypes as C
    pairs = five[:2]
    s, so, t, to, nr = _pack(pairs)
    before = _run_batch(ctx, pairs, OR.POINT, None, max_iterations=5)
    for ov in (np.array([0.5, 0.0]), np.array([float("nan"), 1.0]), np.array([1.5, 1.0])):
        with pytest.raises(pkg.KssError) as e:
            ctx.icp_o2o_batch(s, so, t, to, None, overlaps=ov, metric=OR.POINT)
        assert e.value.status == -1
    with pytest.raises(pkg.KssError) as e:
        ctx.icp_o2o_batch(s, so, t, to, nr, metric=OR.POINT)                  # the point metric takes no normals
    assert e.value.status == -1
    bad = so.copy(); bad[1] = bad[0]                                          # an empty pair
    with pytest.raises(pkg.KssError) as e:
        ctx.icp_o2o_batch(s, bad, t, to, None, metric=OR.POINT)
    assert e.value.status == -1
    p = ctx.icp_params()
    p.allreduce = pkg.binding.ALLREDUCE_FN(lambda user, values, n: 0)
    with pytest.raises(pkg.KssError) as e:
        ctx.icp_o2o_batch(s, so, t, to, None, metric=OR.POINT, params=p)
    assert e.value.status == -1
    L, q = ctx.L, ctx.icp_params()
    res = (pkg.IcpResult * 2)()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.kss_icp_o2o_batch(ctx.h, vp(s), vp(so), vp(t), vp(to), None, 2, C.byref(q), None, None, C.cast(res, C.c_void_p), None) == -1
    op = pkg.o2o_params()
    assert L.kss_icp_o2o_batch(ctx.h, vp(s), vp(so), vp(t), vp(to), None, 0, C.byref(q), C.byref(op), None, C.cast(res, C.c_void_p), None) == -1
    assert L.kss_icp_o2o_batch(ctx.h, vp(s), vp(so), vp(t), vp(to), None, 2, C.byref(q), C.byref(op), None, None, None) == -1
    # the context is as it was
    after = _run_batch(ctx, pairs, OR.POINT, None, max_iterations=5)
    for a, b in zip(before[0], after[0]):
        assert np.array_equal(_bits(a.matrix()), _bits(b.matrix())) and _f64_bits(a.fitness) == _f64_bits(b.fitness)
    assert np.array_equal(_bits(before[1]), _bits(after[1]))
