"""Robust ICP for many pairs per call (kss_icp_robust_batch[_dev]).  The contract: every pair's record is the
single-pair call's, bit for bit -- so the reference of every comparison here is Context.icp_robust on the pair alone with the same
parameters (T, iterations, state, converged, last_mse, the info row, pair 0's traces as bit patterns; the fitness within the bound
of two summation orders, 2 ns 2^-53 relative).  The L2 loss anchors the batch to kss_icp_p2l_batch and kss_icp_trimmed_batch, and
the six outlier pairs to their true motion."""

import numpy as np
import pytest

import robust_ref as RR
from test_gpu_pairs_batch import _bits, _bumpy, _f64_bits, _fitness_bound, _normals

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
POINT, PLANE = RR.POINT, RR.PLANE
METRICS = [POINT, PLANE]
ROBUST = [RR.HUBER, RR.TUKEY, RR.CAUCHY]
OUTLIER_SPECS = RR.PAIRS + [(4, 1500, 8.0, 0.3), (5, 2000, 6.0, 0.35), (6, 1200, 7.0, 0.25), (7, 1800, 9.0, 0.3)]
BOUNDARY_NS = [37, 255, 256, 257, 511, 512, 513, 769]      # one row, a partial wavefront, the row-count boundaries


class Pair:
    """One pair with its normals and, computed once and kept, the single-pair calls' results on it."""

    def __init__(self, ctx, src, tgt, nrm=None, truth=None):
        self.ctx = ctx
        self.src, self.tgt = np.ascontiguousarray(src, F32), np.ascontiguousarray(tgt, F32)
        self.nrm = _normals(ctx, self.tgt) if nrm is None else np.ascontiguousarray(nrm, F32)
        self.truth = truth
        self._single = {}

    def single(self, pkg, loss, metric, scale=0.0, min_scale=0.0, trace=False, **kw):
        key = (loss, metric, scale, min_scale, trace, tuple(sorted(kw.items())))
        if key not in self._single:
            rp = pkg.robust_params(loss, metric, scale=scale, min_scale=min_scale)
            self._single[key] = self.ctx.icp_robust(self.src, self.tgt, self.nrm if metric == PLANE else None, rp=rp,
                                                    params=self.ctx.icp_params(**kw), trace_cap=256 if trace else 0)
        return self._single[key]


def _pack(pairs):
    so = np.concatenate([[0], np.cumsum([len(p.src) for p in pairs])]).astype(np.int64)
    to = np.concatenate([[0], np.cumsum([len(p.tgt) for p in pairs])]).astype(np.int64)
    return (np.concatenate([p.src for p in pairs]), so, np.concatenate([p.tgt for p in pairs]), to,
            np.concatenate([p.nrm for p in pairs]))


def _run(pkg, ctx, pairs, loss, metric, scales=None, scale=0.0, min_scale=0.0, trace=False, normals=True, **kw):
    """-> (list of IcpResult, info npairs x 4, extras of pair 0)"""
    s, so, t, to, nr = _pack(pairs)
    rp = pkg.robust_params(loss, metric, scale=scale, min_scale=min_scale)
    return ctx.icp_robust_batch(s, so, t, to, nr if (metric == PLANE and normals) else None, rp=rp, scales=scales,
                                params=ctx.icp_params(**kw), trace_cap=256 if trace else 0)


def _check_record(r, info, single, ns, pair_id):
    """IcpResult r and info row of a batch against the single-pair call's dictionary.  Returns whether the fitness was bit-equal."""
    assert r.pair_id == pair_id
    assert r.iterations == single["iterations"] and r.state == single["state"] and bool(r.converged) == single["converged"], (
        pair_id, r.iterations, r.state, single["iterations"], single["state"])
    assert np.array_equal(_bits(r.matrix()), _bits(single["T"])), pair_id
    assert _f64_bits(r.last_mse) == _f64_bits(single["last_mse"]), pair_id
    assert np.array_equal(_bits(info), _bits(single["robust_info"])), (pair_id, info, single["robust_info"])
    assert abs(r.fitness - single["fitness"]) <= _fitness_bound(ns, single["fitness"]), pair_id
    return _f64_bits(r.fitness) == _f64_bits(single["fitness"])


def _check_trace(extra, single):
    for k in ("trace_sums", "trace_Tk", "trace_robust"):
        assert np.array_equal(_bits(extra[k]), _bits(single[k])), k


def _key(r, info):
    return (r.iterations, r.state, r.converged, _bits(r.matrix()).tolist(), _f64_bits(r.last_mse), _bits(info).tolist())


@pytest.fixture(scope="module")
def outliers(pkg, ctx):
    out = []
    for spec in OUTLIER_SPECS:
        src, tgt, R, t = pkg.synth.make_outlier_pair(*spec)
        out.append(Pair(ctx, src, tgt, truth=(R.T, -R.T @ t)))
    return out


@pytest.fixture(scope="module")
def boundary(pkg, ctx):
    return [Pair(ctx, *_bumpy(pkg, 40 + i, 800, 5.0, n_src=ns)) for i, ns in enumerate(BOUNDARY_NS)]


@pytest.fixture(scope="module")
def fourteen(outliers, boundary):
    both = outliers + boundary
    return [both[i] for i in np.random.default_rng(14).permutation(len(both))]


def _mixed_scales(n):
    return np.array([(0.0, 0.02, 0.05)[i % 3] for i in range(n)], F64)


# ---- test 1: batch = single calls ----
CASES = [(loss, metric, "auto") for loss in ROBUST for metric in METRICS]
CASES += [(RR.HUBER, POINT, "fixed"), (RR.TUKEY, PLANE, "fixed"), (RR.CAUCHY, POINT, "mixed"), (RR.HUBER, PLANE, "mixed"),
          (RR.TUKEY, POINT, "floor"), (RR.CAUCHY, PLANE, "floor")]


@pytest.mark.parametrize("loss,metric,how", CASES, ids=lambda v: str(v))
def test_batch_equals_single_calls(pkg, ctx, fourteen, loss, metric, how):
    n = len(fourteen)
    scales = {"auto": None, "fixed": np.full(n, 0.02), "mixed": _mixed_scales(n), "floor": None}[how]
    min_scale = 0.01 if how == "floor" else 0.0
    res, info, extra = _run(pkg, ctx, fourteen, loss, metric, scales=scales, min_scale=min_scale, trace=True, max_iterations=60)
    assert len(res) == n and info.shape == (n, 4)
    same = []
    for i, (r, pr) in enumerate(zip(res, fourteen)):
        single = pr.single(pkg, loss, metric, scale=0.0 if scales is None else float(scales[i]), min_scale=min_scale, trace=(i == 0),
                           max_iterations=60)
        assert single["iterations"] >= 2, i
        same.append(_check_record(r, info[i], single, len(pr.src), i))
    _check_trace(extra, fourteen[0].single(pkg, loss, metric, scale=0.0 if scales is None else float(scales[0]), min_scale=min_scale,
                                           trace=True, max_iterations=60))
    print("icp_robust_batch loss %d metric %d %s: fitness bit-equal to the single call for %d of %d" % (loss, metric, how, sum(same), n))


# ---- test 2: the L2 anchors ----
def test_l2_plane_batch_is_p2l_batch(pkg, ctx, fourteen):
    s, so, t, to, nr = _pack(fourteen)
    a, _ = ctx.icp_p2l_batch(s, so, t, to, nr, params=ctx.icp_params(max_iterations=60))
    for kw in (dict(), dict(scale=0.05)):
        b, info, _ = _run(pkg, ctx, fourteen, RR.L2, PLANE, max_iterations=60, **kw)
        for x, y in zip(a, b):
            assert x.iterations == y.iterations >= 1 and x.state == y.state and x.converged == y.converged and x.pair_id == y.pair_id
            assert np.array_equal(_bits(x.matrix()), _bits(y.matrix()))
            assert _f64_bits(x.last_mse) == _f64_bits(y.last_mse)
        assert np.all(info[:, 0] == info[:, 3]) and np.all(info[:, 2] == info[:, 3])      # every candidate, weight 1


def test_l2_point_batch_is_trimmed_batch_overlap_one(pkg, ctx, fourteen):
    s, so, t, to, _ = _pack(fourteen)
    a, _, _ = ctx.icp_trimmed_batch(s, so, t, to, None, overlap=1.0, metric=POINT, params=ctx.icp_params(max_iterations=60))
    for kw in (dict(), dict(scale=0.05)):
        b, info, _ = _run(pkg, ctx, fourteen, RR.L2, POINT, max_iterations=60, **kw)
        for x, y in zip(a, b):
            assert x.iterations == y.iterations >= 1 and x.state == y.state and x.converged == y.converged and x.pair_id == y.pair_id
            assert np.array_equal(_bits(x.matrix()), _bits(y.matrix()))
            assert _f64_bits(x.last_mse) == _f64_bits(y.last_mse)
        assert np.all(info[:, 0] == info[:, 3]) and np.all(info[:, 2] == info[:, 3])


# ---- test 3: recovery ----
def _errors(T, truth):
    return max(np.abs(T[:3, :3] - truth[0]).max(), np.abs(T[:3, 3] - truth[1]).max())


@pytest.mark.parametrize("loss", ROBUST, ids=["huber", "tukey", "cauchy"])
@pytest.mark.parametrize("metric", METRICS, ids=["point", "plane"])
def test_batch_recovers_the_true_motion(pkg, ctx, outliers, metric, loss):
    res, _, _ = _run(pkg, ctx, outliers, loss, metric, max_iterations=200)
    errs = [_errors(r.matrix(), pr.truth) for r, pr in zip(res, outliers)]
    print("loss %d metric %d: iterations %s, max|T - truth| %s" % (loss, metric, [r.iterations for r in res], ["%.2e" % e for e in errs]))
    assert all(r.converged for r in res)
    assert max(errs) < 2e-3


def test_l2_point_batch_misses_the_bar(pkg, ctx, outliers):
    res, _, _ = _run(pkg, ctx, outliers, RR.L2, POINT, max_iterations=200)
    errs = [_errors(r.matrix(), pr.truth) for r, pr in zip(res, outliers)]
    print("L2 point: max|T - truth| %s" % ["%.2e" % e for e in errs])
    assert min(errs) >= 2e-3


# ---- test 4: endings inside a batch ----
class _Witness:
    """kss_icp, kss_icp_p2l, kss_icp_robust and a small kss_icp_batch on fixed pairs: the same bits before and after."""

    def __init__(self, pkg, ctx):
        self.pkg, self.ctx = pkg, ctx
        self.src, self.tgt = _bumpy(pkg, 11, 3000, 7.0, n_src=2500)
        self.nrm = _normals(ctx, self.tgt)
        small = [_bumpy(pkg, 30 + i, 700 + 50 * i, 6.0) for i in range(3)]
        self.bs = np.concatenate([s for s, _ in small]); self.bt = np.concatenate([t for _, t in small])
        self.bso = np.concatenate([[0], np.cumsum([len(s) for s, _ in small])])
        self.bto = np.concatenate([[0], np.cumsum([len(t) for _, t in small])])
        self.before = self.run()

    def run(self):
        a = self.ctx.icp(self.src, self.tgt, trace_cap=64)
        b = self.ctx.icp_p2l(self.src, self.tgt, self.nrm, trace_cap=64)
        c = self.ctx.icp_robust(self.src, self.tgt, self.nrm, loss=RR.TUKEY, metric=PLANE, trace_cap=64)
        d = self.ctx.icp_batch(self.bs, self.bso, self.bt, self.bto)
        return a, b, c, [(r.iterations, r.state, _bits(r.matrix()).tolist(), _f64_bits(r.fitness)) for r in d]

    def check(self):
        now = self.run()
        for x, y in zip(self.before[:3], now[:3]):
            assert x["iterations"] == y["iterations"] and x["state"] == y["state"]
            assert np.array_equal(_bits(x["T"]), _bits(y["T"]))
            assert np.array_equal(_bits(x["trace_sums"]), _bits(y["trace_sums"]))
            assert _f64_bits(x["fitness"]) == _f64_bits(y["fitness"])
        assert self.before[3] == now[3]


def _ending_pairs(pkg, ctx, metric):
    """(pair, scale, expected state or None, name)"""
    out = []
    src, tgt = _bumpy(pkg, 9, 2000, 5.0)
    out.append((Pair(ctx, src + F32(100.0), tgt), 0.0, 5, "no candidate"))
    src, tgt = _bumpy(pkg, 12, 500, 5.0)
    out.append((Pair(ctx, src, tgt), 1e-30, 5, "tiny scale"))
    out.append((Pair(ctx, *_bumpy(pkg, 40, 800, 5.0, n_src=3)), 0.0, pkg.STATE_DEGENERATE if metric == PLANE else None, "ns = 3"))
    if metric == PLANE:
        g = np.linspace(-1, 1, 40)
        tgt = np.stack(np.meshgrid(g, g), -1).reshape(-1, 2)
        tgt = np.concatenate([tgt, np.zeros((len(tgt), 1))], 1).astype(F32)
        src = (tgt[::2] + np.array([0.01, -0.02, 0.05])).astype(F32)
        out.append((Pair(ctx, src, tgt, nrm=np.tile(np.array([0, 0, 1], F32), (len(tgt), 1))), 0.0, pkg.STATE_DEGENERATE, "planar"))
    _, tgt = _bumpy(pkg, 13, 1000, 5.0)
    src = tgt.copy()
    src[:400] += F32(0.5)                       # 40 % pushed away; the others' d2 is exactly 0: the median key is 0
    out.append((Pair(ctx, src, tgt), 0.0, None, "median 0"))
    return out


@pytest.mark.parametrize("metric", METRICS, ids=["point", "plane"])
def test_endings_inside_a_batch(pkg, ctx, outliers, boundary, metric):
    w = _Witness(pkg, ctx)
    loss = RR.TUKEY
    healthy = [outliers[2], boundary[3], outliers[4], boundary[6], outliers[5]]
    ending = _ending_pairs(pkg, ctx, metric)
    pairs, scales, expect, names = [], [], [], []
    for i, hp in enumerate(healthy):                      # ending pairs between and around the healthy ones
        if i < len(ending):
            e = ending[i]
            pairs.append(e[0]); scales.append(e[1]); expect.append(e[2]); names.append(e[3])
        pairs.append(hp); scales.append(0.0); expect.append(None); names.append(None)
    assert len(ending) <= len(healthy)
    res, info, _ = _run(pkg, ctx, pairs, loss, metric, scales=np.array(scales), max_iterations=60)
    for i, (r, pr) in enumerate(zip(res, pairs)):
        single = pr.single(pkg, loss, metric, scale=scales[i], max_iterations=60)
        _check_record(r, info[i], single, len(pr.src), i)
        if expect[i] is not None:
            assert r.state == expect[i] and r.iterations == 0 and not r.converged, names[i]
            assert np.array_equal(r.matrix(), np.eye(4, dtype=F32))
        elif names[i] is None:
            assert r.iterations >= 2
        if names[i] == "no candidate":
            assert np.array_equal(info[i], np.zeros(4))
        if names[i] == "tiny scale":
            assert info[i][1] == 1e-30 * 1e-30 and info[i][0] > 0.9 * len(pr.src) and info[i][3] < 3
        if names[i] == "ns = 3" and metric == POINT:
            assert r.iterations == 3
        if names[i] == "median 0" and metric == POINT:
            assert info[i][1] == 0.0 and info[i][3] == 600 and info[i][0] >= 600
    alone, info_alone, _ = _run(pkg, ctx, healthy, loss, metric, scales=np.zeros(len(healthy)), max_iterations=60)
    with_endings = [(r, info[i], len(pairs[i].src)) for i, r in enumerate(res) if names[i] is None]
    assert len(with_endings) == len(healthy)
    for (r, inf, ns), a, ia in zip(with_endings, alone, info_alone):
        assert _key(r, inf) == _key(a, ia)
        assert abs(r.fitness - a.fitness) <= _fitness_bound(ns, a.fitness)
    w.check()


# ---- test 5: invariances ----
@pytest.mark.parametrize("metric", METRICS, ids=["point", "plane"])
def test_batch_invariances(pkg, ctx, outliers, boundary, metric):
    six = [outliers[0], boundary[0], outliers[3], boundary[2], boundary[5], outliers[1]]
    n = len(six)
    sc = _mixed_scales(n)
    loss = RR.CAUCHY
    kw = dict(max_iterations=40)

    def run(order, **more):
        res, info, _ = _run(pkg, ctx, [six[i] for i in order], loss, metric, scales=sc[list(order)], **dict(kw, **more))
        assert [r.pair_id for r in res] == list(range(len(order)))
        return {i: (res[j], info[j]) for j, i in enumerate(order)}

    base = run(range(n))
    assert all(base[i][0].iterations >= 2 for i in range(n))
    perm = run([4, 0, 5, 2, 1, 3])                                      # the order of the batch
    ones = {}
    for i in range(n):                                                  # a batch of one = the single-pair call
        ones.update(run([i]))
        _check_record(ones[i][0], ones[i][1], six[i].single(pkg, loss, metric, scale=float(sc[i]), **kw), len(six[i].src), 0)
    halves = {**run([0, 1]), **run([2, 3, 4, 5])}                       # two calls instead of one
    others = [perm, ones, halves]
    for more in (dict(nn_mode=pkg.NN_BRUTE), dict(nn_mode=pkg.NN_GRID), dict(nn_mode=pkg.NN_AUTO),
                 dict(nn_mode=pkg.NN_BRUTE, nn_sources_per_thread=1, nn_target_splits=3),
                 dict(nn_mode=pkg.NN_BRUTE, nn_sources_per_thread=8, nn_target_splits=1)):
        others.append(run(range(n), **more))
    for other in others:
        for i in range(n):
            assert _key(*other[i]) == _key(*base[i]), i
            assert abs(other[i][0].fitness - base[i][0].fitness) <= _fitness_bound(len(six[i].src), base[i][0].fitness)


# ---- test 6: more pairs than compute units ----
def test_more_pairs_than_compute_units(pkg, ctx):
    rng = np.random.default_rng(300)
    pairs = []
    for i in range(300):
        n = int(rng.integers(600, 1201))
        n_src = int(rng.integers(600, 1201))
        pairs.append(Pair(ctx, *_bumpy(pkg, 100 + i, n, float(rng.uniform(3.0, 12.0)), n_src=n_src)))
    res, info, _ = _run(pkg, ctx, pairs, RR.CAUCHY, PLANE, max_iterations=60)
    assert len(res) == 300
    same = 0
    for i, (r, pr) in enumerate(zip(res, pairs)):
        same += _check_record(r, info[i], pr.single(pkg, RR.CAUCHY, PLANE, max_iterations=60), len(pr.src), i)
    assert sum(r.iterations >= 2 for r in res) == 300
    print("300 pairs: fitness bit-equal to the single call for %d" % same)


# ---- test 7: a pair above the row cap (stream_blocks saturates at 2048 rows: the grid-stride term is live) ----
def test_pair_above_the_row_cap(pkg, ctx, boundary):
    src, tgt = _bumpy(pkg, 60, 524800, 5.0)
    big = Pair(ctx, src, tgt[::26])
    assert len(big.src) == 524800 > 2048 * 256
    pairs = [boundary[1], big, boundary[4]]
    for metric in METRICS:
        res, info, extra = _run(pkg, ctx, pairs, RR.HUBER, metric, max_iterations=3)
        for i, (r, pr) in enumerate(zip(res, pairs)):
            single = pr.single(pkg, RR.HUBER, metric, max_iterations=3)
            assert single["iterations"] >= 2
            _check_record(r, info[i], single, len(pr.src), i)


# ---- test 8: device variants, computed normals ----
def test_dev_variants_and_computed_normals(pkg, ctx, outliers, boundary):
    import torch
    pairs = [outliers[2], boundary[7], outliers[4]]
    s, so, t, to, nr = _pack(pairs)
    sc = np.array([0.0, 0.02, 0.0])
    ds, dt, dn = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (s, t, nr))
    torch.cuda.synchronize()
    p = ctx.icp_params(max_iterations=40)

    def same(a, ai, b, bi):
        for x, xi, y, yi in zip(a, ai, b, bi):
            assert _key(x, xi) == _key(y, yi) and x.pair_id == y.pair_id
            assert _f64_bits(x.fitness) == _f64_bits(y.fitness)

    for metric in METRICS:
        rp = pkg.robust_params(RR.HUBER, metric)
        h, hi, _ = _run(pkg, ctx, pairs, RR.HUBER, metric, scales=sc, max_iterations=40)
        for d_n in ((dn.data_ptr(), None) if metric == PLANE else (None,)):
            d, di = ctx.icp_robust_batch_dev(ds.data_ptr(), so, dt.data_ptr(), to, d_n, p, rp=rp, scales=sc)
            same(h, hi, d, di)
        # a sub-range of the packed arrays: offsets that do not start at 0
        d, di = ctx.icp_robust_batch_dev(ds.data_ptr(), so[1:], dt.data_ptr(), to[1:], dn.data_ptr() if metric == PLANE else None, p, rp=rp,
                                         scales=sc[1:])
        for x, xi, y, yi in zip(d, di, h[1:], hi[1:]):
            assert _key(x, xi) == _key(y, yi)
    # normals_all = None: kss_normals of each target rounded to float, which is what the pairs carry
    a, ai, _ = _run(pkg, ctx, pairs, RR.HUBER, PLANE, scales=sc, max_iterations=40)
    b, bi, _ = _run(pkg, ctx, pairs, RR.HUBER, PLANE, scales=sc, normals=False, max_iterations=40)
    same(a, ai, b, bi)
    # scales = None: rp->scale for every pair
    a, ai, _ = _run(pkg, ctx, pairs, RR.TUKEY, POINT, scales=None, scale=0.05, max_iterations=40)
    b, bi, _ = _run(pkg, ctx, pairs, RR.TUKEY, POINT, scales=np.full(3, 0.05), max_iterations=40)
    same(a, ai, b, bi)


# ---- test 9: argument errors ----
def test_argument_errors(pkg, ctx, outliers, boundary):
    import ctypes as C
    pairs = [outliers[2], boundary[3]]
    s, so, t, to, nr = _pack(pairs)

    def valid():
        out = []
        for metric in METRICS:
            res, info, _ = _run(pkg, ctx, pairs, RR.HUBER, metric, scales=np.array([0.0, 0.02]), max_iterations=40)
            out.append([_key(r, i) + (_f64_bits(r.fitness),) for r, i in zip(res, info)])
        return out

    before = valid()

    def refused(call):
        with pytest.raises(pkg.KssError) as e:
            call()
        assert e.value.status == -1

    def batch(rp, normals=None, scales=None, so_=so, to_=to, params=None):
        return ctx.icp_robust_batch(s, so_, t, to_, normals, rp=rp, scales=scales, params=params)

    p = ctx.icp_params()
    p.allreduce = pkg.binding.ALLREDUCE_FN(lambda user, values, n: 0)
    for metric in METRICS:
        refused(lambda: batch(pkg.robust_params(RR.HUBER, metric), nr if metric == PLANE else None, params=p))
    assert valid() == before
    nan, inf = float("nan"), float("inf")
    for field, values in (("loss", (-1, 4)), ("metric", (-1, 2)), ("scale", (-0.5, inf, nan)), ("tune", (0.0, -1.0, inf, nan)),
                          ("min_scale", (-0.5,))):
        for v in values:
            rp = pkg.robust_params(RR.HUBER, POINT)
            setattr(rp, field, v)
            refused(lambda: batch(rp))
    for bad in (-0.5, inf, nan):
        refused(lambda: batch(pkg.robust_params(RR.HUBER, POINT), scales=np.array([0.02, bad])))
    for tune in (0.0, -1.0, inf, nan):                    # an automatic pair needs the tune; an all-fixed batch does not read it
        rp = pkg.robust_params(RR.HUBER, POINT, scale=0.02)
        rp.tune = tune
        refused(lambda: batch(rp, scales=np.array([0.02, 0.0])))
        assert len(batch(rp, scales=np.array([0.02, 0.05]))[0]) == 2
    refused(lambda: batch(pkg.robust_params(RR.HUBER, POINT), normals=nr))               # normals with the point metric
    assert valid() == before
    so_e = np.array([so[0], so[1], so[1], so[2]]); to_e = np.array([to[0], to[1], to[1] + 5, to[2]])
    refused(lambda: batch(pkg.robust_params(RR.HUBER, POINT), so_=so_e, to_=to_e))      # an empty source
    to_e2 = np.array([to[0], to[1], to[1], to[2]]); so_e2 = np.array([so[0], so[1], so[1] + 5, so[2]])
    refused(lambda: batch(pkg.robust_params(RR.HUBER, PLANE), normals=nr, so_=so_e2, to_=to_e2))      # an empty target
    with pytest.raises(ValueError):
        batch(pkg.robust_params(RR.HUBER, POINT), scales=np.array([0.02]))
    # null results, through the C-ABI itself
    _p = pkg.binding._p
    rp = pkg.robust_params(RR.HUBER, POINT)
    pp = ctx.icp_params()
    for fn in (ctx.L.kss_icp_robust_batch, ctx.L.kss_icp_robust_batch_dev):
        assert fn(ctx.h, _p(s), _p(so), _p(t), _p(to), None, 2, C.byref(pp), C.byref(rp), None, None, None) == -1
    assert valid() == before
