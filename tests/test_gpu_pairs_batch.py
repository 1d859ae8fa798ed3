"""Point-to-plane and trimmed ICP for many pairs per call (kss_icp_p2l_batch, kss_icp_trimmed_batch, kss_trim_threshold_batch;
DESIGN.md 2.11).  The contract: every pair's numbers are the single-pair call's, bit for bit -- so nearly every check here is a
comparison of bit patterns with kss_icp_p2l / kss_icp_trimmed / kss_trim_threshold on the pair alone; the independent
restatement (tests/trim_ref.py) anchors the batch once more on its own."""

import numpy as np
import pytest

import trim_ref as TR
from test_gpu_trim import FULL_PAIRS, OVERLAPS, PAIRS, SETS

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
LENGTHS = [1, 2, 63, 64, 65, 257, 4096, 100000, 3000001]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == F64 else np.uint32)


def _f32_bits(x):
    return int(np.array([x], F32).view(np.uint32)[0])


def _f64_bits(x):
    return int(np.array([x], F64).view(np.uint64)[0])


def _normals(ctx, tgt):
    return ctx.normals(tgt.astype(F64), 20).astype(F32)


def _bumpy(pkg, pair_id, n, deg, n_src=None, t=(0.02, -0.01, 0.03)):
    axis = pkg.synth.sphere(7000 + pair_id, 1)[0]
    return pkg.synth.make_pair(pair_id, n, R=pkg.synth.rot_axis_angle(axis, np.deg2rad(deg)), t=t, shape="bumpy", n_src=n_src)


class Pair:
    """One pair with its normals and, computed once and kept, the single-pair calls' results on it."""

    def __init__(self, ctx, src, tgt, nrm=None, truth=None):
        self.ctx = ctx
        self.src, self.tgt = np.ascontiguousarray(src, F32), np.ascontiguousarray(tgt, F32)
        self.nrm = _normals(ctx, self.tgt) if nrm is None else np.ascontiguousarray(nrm, F32)
        self.truth = truth
        self._single = {}

    def single(self, kind, overlap=1.0, trace=False, **kw):
        """kind 'p2l' (kss_icp_p2l), TR.POINT / TR.PLANE (kss_icp_trimmed with that metric)."""
        key = (kind, overlap, trace, tuple(sorted(kw.items())))
        if key not in self._single:
            p = self.ctx.icp_params(**kw)
            cap = 256 if trace else 0
            if kind == "p2l":
                r = self.ctx.icp_p2l(self.src, self.tgt, self.nrm, params=p, trace_cap=cap)
            else:
                r = self.ctx.icp_trimmed(self.src, self.tgt, self.nrm if kind == TR.PLANE else None, overlap=overlap, metric=kind, params=p,
                                         trace_cap=cap)
            self._single[key] = r
        return self._single[key]


def _pack(pairs):
    so = np.concatenate([[0], np.cumsum([len(p.src) for p in pairs])]).astype(np.int64)
    to = np.concatenate([[0], np.cumsum([len(p.tgt) for p in pairs])]).astype(np.int64)
    return (np.concatenate([p.src for p in pairs]), so, np.concatenate([p.tgt for p in pairs]), to,
            np.concatenate([p.nrm for p in pairs]))


def _run_batch(ctx, pairs, kind, overlaps=None, trace=False, normals=True, **kw):
    """-> (list of IcpResult, info npairs x 4 or None, extras of pair 0)"""
    s, so, t, to, nr = _pack(pairs)
    p = ctx.icp_params(**kw)
    cap = 256 if trace else 0
    if kind == "p2l":
        res, extra = ctx.icp_p2l_batch(s, so, t, to, nr if normals else None, params=p, trace_cap=cap)
        return res, None, extra
    res, info, extra = ctx.icp_trimmed_batch(s, so, t, to, nr if (kind == TR.PLANE and normals) else None, overlaps=overlaps, metric=kind,
                                             params=p, trace_cap=cap)
    return res, info, extra


def _fitness_bound(ns, ref):
    # test_gpu_trim.py's bound for two summation orders of the NN engines' f64 sum of d2 over all sources: each order is within
    # (n - 1) 2^-53 relative of the exact sum of the non-negative terms, two orders differ by less than 2 n 2^-53 relative
    return 2.0 * ns * 2.0 ** -53 * ref


def _check_record(r, single, ns, pair_id, info=None, exact_fitness=False):
    """IcpResult r of a batch against the single-pair call's dictionary.  Returns whether the fitness was bit-equal."""
    assert r.pair_id == pair_id
    assert r.iterations == single["iterations"] and r.state == single["state"] and bool(r.converged) == single["converged"]
    assert np.array_equal(_bits(r.matrix()), _bits(single["T"]))
    assert _f64_bits(r.last_mse) == _f64_bits(single["last_mse"])
    assert abs(r.fitness - single["fitness"]) <= _fitness_bound(ns, single["fitness"])
    same = _f64_bits(r.fitness) == _f64_bits(single["fitness"])
    if exact_fitness:
        assert same
    if info is not None:
        assert np.array_equal(_bits(info), _bits(single["trim_info"]))
    return same


def _check_trace(extra, single, trimmed):
    assert np.array_equal(_bits(extra["trace_sums"]), _bits(single["trace_sums"]))
    assert np.array_equal(_bits(extra["trace_Tk"]), _bits(single["trace_Tk"]))
    if trimmed:
        assert np.array_equal(_bits(extra["trace_trim"]), _bits(single["trace_trim"]))


@pytest.fixture(scope="module")
def six(pkg, ctx):
    """The three full bumpy pairs of test_gpu_p2l.py and the three partial pairs of test_gpu_trim.py."""
    out = [Pair(ctx, *_bumpy(pkg, pid, n, deg, n_src=n_src)) for pid, n, n_src, deg in FULL_PAIRS]
    for spec in PAIRS:
        src, tgt, R, t, _ = pkg.synth.make_partial_pair(*spec)
        out.append(Pair(ctx, src, tgt, truth=(R.T, -R.T @ t)))
    return out


@pytest.fixture(scope="module")
def twelve(pkg, ctx, six):
    """... twice, the second time with other ids, in a shuffled order (ragged: 1800 to 8000 points)."""
    more = [Pair(ctx, *_bumpy(pkg, pid + 20, n, deg, n_src=n_src)) for pid, n, n_src, deg in FULL_PAIRS]
    for spec in PAIRS:
        src, tgt = pkg.synth.make_partial_pair(spec[0] + 20, *spec[1:])[:2]
        more.append(Pair(ctx, src, tgt))
    both = six + more
    order = np.random.default_rng(12).permutation(len(both))
    return [both[i] for i in order]


def _mixed_overlaps(n):
    return np.array([(1.0, 0.5, 0.25)[i % 3] for i in range(n)], F64)


# ---- test 1: the selection ----
@pytest.fixture(scope="module")
def segments():
    segs = [SETS[i % len(SETS)](n, np.random.default_rng(1000 + i))[0] for i, n in enumerate(LENGTHS)]
    off = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.int64)
    return segs, off, np.concatenate(segs)


@pytest.mark.parametrize("rot,max_d2", [(0, 2.0), (1, 2.0), (2, 2.0), (3, 2.0), (4, 2.0), (0, 1.0)])
def test_threshold_batch_bit_exact(ctx, segments, rot, max_d2):
    segs, off, d2_all = segments
    ov = np.array([OVERLAPS[(i + rot) % len(OVERLAPS)] for i in range(len(segs))], F64)
    got = ctx.trim_threshold_batch(d2_all, off, ov, max_d2)
    again = ctx.trim_threshold_batch(d2_all, off, ov, max_d2)
    assert got.shape == (len(segs), 4)
    assert np.array_equal(_bits(got), _bits(again))
    for i, d2 in enumerate(segs):
        _, m, k, tau, kept = TR.threshold(d2, max_d2, ov[i])
        g = got[i]
        assert g[0] == m and g[1] == k, (i, ov[i], g, m, k)
        assert g[2] == float(tau) and _f32_bits(g[2]) == _f32_bits(tau), (i, ov[i], g, tau)
        assert g[3] == int(kept.sum()), (i, ov[i], g, int(kept.sum()))
        assert np.array_equal(_bits(g), _bits(ctx.trim_threshold(d2, max_d2, ov[i]))), (i, ov[i])


def test_threshold_batch_subrange_and_dev(ctx, segments):
    """Offsets that do not start at 0, and the device variant."""
    import torch
    segs, off, d2_all = segments
    ov = np.array([OVERLAPS[i % len(OVERLAPS)] for i in range(len(segs))], F64)
    full = ctx.trim_threshold_batch(d2_all, off, ov, 2.0)
    part = ctx.trim_threshold_batch(d2_all, off[3:8], ov[3:7], 2.0)
    assert np.array_equal(_bits(part), _bits(full[3:7]))
    d = torch.from_numpy(d2_all).cuda()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(ctx.trim_threshold_batch_dev(d.data_ptr(), off, ov, 2.0)), _bits(full))
    assert np.array_equal(_bits(ctx.trim_threshold_batch_dev(d.data_ptr(), off[3:8], ov[3:7], 2.0)), _bits(full[3:7]))


# ---- test 2: batch = single calls, plane, untrimmed ----
def test_p2l_batch_equals_single_calls(ctx, twelve):
    res, _, extra = _run_batch(ctx, twelve, "p2l", trace=True, max_iterations=60)
    assert len(res) == 12
    same = []
    for i, (r, pr) in enumerate(zip(res, twelve)):
        single = pr.single("p2l", trace=(i == 0), max_iterations=60)
        assert single["iterations"] >= 1
        same.append(_check_record(r, single, len(pr.src), i))
    _check_trace(extra, twelve[0].single("p2l", trace=True, max_iterations=60), False)
    print("icp_p2l_batch, 12 pairs: fitness bit-equal to the single call for %d of 12 (%s)" % (sum(same), same))


# ---- test 3: batch = single calls, trimmed, both metrics ----
@pytest.mark.parametrize("metric", [TR.POINT, TR.PLANE], ids=["point", "plane"])
def test_trimmed_batch_equals_single_calls(ctx, twelve, metric):
    ov = _mixed_overlaps(12)
    res, info, extra = _run_batch(ctx, twelve, metric, overlaps=ov, trace=True, max_iterations=60)
    same = []
    for i, (r, pr) in enumerate(zip(res, twelve)):
        single = pr.single(metric, overlap=float(ov[i]), trace=(i == 0), max_iterations=60)
        same.append(_check_record(r, single, len(pr.src), i, info[i]))
    _check_trace(extra, twelve[0].single(metric, overlap=float(ov[0]), trace=True, max_iterations=60), True)
    print("icp_trimmed_batch metric %d: fitness bit-equal for %d of 12" % (metric, sum(same)))


def test_trimmed_plane_overlap_one_is_p2l_batch(ctx, twelve):
    """DESIGN 2.10's anchor, batched."""
    a, _, ea = _run_batch(ctx, twelve, "p2l", trace=True, max_iterations=60)
    b, info, eb = _run_batch(ctx, twelve, TR.PLANE, overlaps=np.ones(12), trace=True, max_iterations=60)
    for x, y in zip(a, b):
        assert x.iterations == y.iterations >= 1 and x.state == y.state and x.converged == y.converged and x.pair_id == y.pair_id
        assert np.array_equal(_bits(x.matrix()), _bits(y.matrix()))
        assert _f64_bits(x.last_mse) == _f64_bits(y.last_mse)
        assert _f64_bits(x.fitness) == _f64_bits(y.fitness)
    assert np.array_equal(_bits(ea["trace_sums"]), _bits(eb["trace_sums"]))
    assert np.array_equal(_bits(ea["trace_Tk"]), _bits(eb["trace_Tk"]))
    assert np.all(info[:, 1] == info[:, 0])      # every candidate kept


# ---- test 4: against the independent restatement ----
@pytest.mark.parametrize("metric", [TR.POINT, TR.PLANE], ids=["point", "plane"])
def test_trimmed_batch_matches_restatement_and_recovers(ctx, O, six, metric):
    part = six[3:]
    res, info, _ = _run_batch(ctx, part, metric, overlaps=np.full(3, 0.5), max_iterations=200)
    for r, pr, spec in zip(res, part, PAIRS):
        ref = TR.icp_trimmed(O, pr.src, pr.tgt, pr.nrm if metric == TR.PLANE else None, 0.5, metric, max_iterations=200)
        T = r.matrix()
        R_true, t_true = pr.truth
        print("pair %d metric %d: batch %d it. state %d, restatement %d it. state %d, max|T - T_ref| %.2e, vs truth %.2e / %.2e" % (
            spec[0], metric, r.iterations, r.state, ref["iterations"], ref["state"], np.abs(T - ref["T"]).max(),
            np.abs(T[:3, :3] - R_true).max(), np.abs(T[:3, 3] - t_true).max()))
        assert r.iterations == ref["iterations"] >= 1
        assert r.state == ref["state"] and bool(r.converged) == ref["converged"]
        assert np.abs(T - ref["T"]).max() <= 5e-6
        assert np.abs(T[:3, :3] - R_true).max() < 2e-3
        assert np.abs(T[:3, 3] - t_true).max() < 2e-3


# ---- test 5: endings inside a batch ----
class _Witness:
    """kss_icp, kss_icp_p2l and a small kss_icp_batch on fixed pairs: what the context gave before must be what it gives afterwards."""

    def __init__(self, pkg, ctx):
        self.ctx = ctx
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
        c = self.ctx.icp_batch(self.bs, self.bso, self.bt, self.bto)
        return a, b, [(r.iterations, r.state, _bits(r.matrix()).tolist(), _f64_bits(r.fitness)) for r in c]

    def check(self):
        now = self.run()
        for x, y in zip(self.before[:2], now[:2]):
            assert x["iterations"] == y["iterations"] and x["state"] == y["state"]
            assert np.array_equal(_bits(x["T"]), _bits(y["T"]))
            assert np.array_equal(_bits(x["trace_sums"]), _bits(y["trace_sums"]))
            assert _f64_bits(x["fitness"]) == _f64_bits(y["fitness"])
        assert self.before[2] == now[2]


def _ending_pairs(pkg, ctx, metric):
    """(pair, overlap, expected state) as test_gpu_trim.py's ending tests build them."""
    out = []
    src, tgt = _bumpy(pkg, 9, 2000, 5.0)
    out.append((Pair(ctx, src + np.float32(100.0), tgt), 0.5, 5))                      # no candidate
    if metric == TR.PLANE:
        g = np.linspace(-1, 1, 40)
        tgt = np.stack(np.meshgrid(g, g), -1).reshape(-1, 2)
        tgt = np.concatenate([tgt, np.zeros((len(tgt), 1))], 1).astype(F32)
        src = (tgt[::2] + np.array([0.01, -0.02, 0.05])).astype(F32)
        out.append((Pair(ctx, src, tgt, nrm=np.tile(np.array([0, 0, 1], F32), (len(tgt), 1))), 0.5, pkg.STATE_DEGENERATE))
    src, tgt = _bumpy(pkg, 12, 500, 5.0)
    out.append((Pair(ctx, src, tgt), 0.001, 5))                                        # k = 1 < min_correspondences = 3
    return out


@pytest.mark.parametrize("metric", [TR.POINT, TR.PLANE], ids=["point", "plane"])
def test_endings_inside_a_batch(pkg, ctx, six, metric):
    w = _Witness(pkg, ctx)
    healthy = [six[0], six[3], six[1]]
    h_ov = [0.8, 0.5, 1.0]
    ending = _ending_pairs(pkg, ctx, metric)
    # ending pairs between and around the healthy ones
    pairs, ov, expect = [], [], []
    for i, hp in enumerate(healthy):
        if i < len(ending):
            pairs.append(ending[i][0]); ov.append(ending[i][1]); expect.append(ending[i][2])
        pairs.append(hp); ov.append(h_ov[i]); expect.append(None)
    for e in ending[len(healthy):]:
        pairs.append(e[0]); ov.append(e[1]); expect.append(e[2])
    res, info, _ = _run_batch(ctx, pairs, metric, overlaps=np.array(ov))
    for i, (r, pr) in enumerate(zip(res, pairs)):
        single = pr.single(metric, overlap=ov[i])
        _check_record(r, single, len(pr.src), i, info[i])
        if expect[i] is not None:
            assert r.state == expect[i] and r.iterations == 0 and not r.converged
            assert np.array_equal(r.matrix(), np.eye(4, dtype=F32))
        else:
            assert r.iterations >= 2
    alone, info_alone, _ = _run_batch(ctx, healthy, metric, overlaps=np.array(h_ov))
    with_endings = [(r, info[i], len(pairs[i].src)) for i, r in enumerate(res) if expect[i] is None]
    for (r, inf, ns), a, ia in zip(with_endings, alone, info_alone):
        assert r.iterations == a.iterations and r.state == a.state and r.converged == a.converged
        assert np.array_equal(_bits(r.matrix()), _bits(a.matrix()))
        assert _f64_bits(r.last_mse) == _f64_bits(a.last_mse)
        assert abs(r.fitness - a.fitness) <= _fitness_bound(ns, a.fitness)
        assert np.array_equal(_bits(inf), _bits(ia))
    w.check()


# ---- test 6: invariances ----
def _key(r, info):
    return (r.iterations, r.state, r.converged, _bits(r.matrix()).tolist(), _f64_bits(r.last_mse), None if info is None else _bits(info).tolist())


@pytest.mark.parametrize("kind", ["p2l", TR.POINT, TR.PLANE], ids=["p2l", "point", "plane"])
def test_batch_invariances(pkg, ctx, six, kind):
    n = len(six)
    ov = _mixed_overlaps(n)
    kw = dict(max_iterations=40)

    def run(order, **more):
        res, info, _ = _run_batch(ctx, [six[i] for i in order], kind, overlaps=ov[list(order)], **dict(kw, **more))
        assert [r.pair_id for r in res] == list(range(len(order)))
        return {i: (res[j], None if info is None else info[j]) for j, i in enumerate(order)}

    base = run(range(n))
    assert all(base[i][0].iterations >= 1 for i in range(n))
    # the order of the batch
    perm = run([4, 0, 5, 2, 1, 3])
    # a batch of one = the single-pair call; one call = the same pairs over two calls
    ones = {}
    for i in range(n):
        ones.update(run([i]))
        single = six[i].single(kind, overlap=float(ov[i]), **kw)
        _check_record(ones[i][0], single, len(six[i].src), 0, ones[i][1])
    halves = {**run([0, 1]), **run([2, 3, 4, 5])}
    for other in (perm, ones, halves):
        for i in range(n):
            assert _key(*other[i]) == _key(*base[i]), i
            assert abs(other[i][0].fitness - base[i][0].fitness) <= _fitness_bound(len(six[i].src), base[i][0].fitness)
    # the NN engine
    for mode in (pkg.NN_BRUTE, pkg.NN_GRID, pkg.NN_AUTO):
        eng = run(range(n), nn_mode=mode)
        for i in range(n):
            assert _key(*eng[i]) == _key(*base[i]), (mode, i)
            assert abs(eng[i][0].fitness - base[i][0].fitness) <= _fitness_bound(len(six[i].src), base[i][0].fitness)


# ---- test 7: more pairs than compute units ----
def test_more_pairs_than_compute_units(pkg, ctx):
    rng = np.random.default_rng(320)
    pairs = []
    for i in range(320):
        n = int(rng.integers(1200, 2001))
        n_src = int(rng.integers(1200, 2001))
        pairs.append(Pair(ctx, *_bumpy(pkg, 100 + i, n, float(rng.uniform(3.0, 12.0)), n_src=n_src)))
    res, info, _ = _run_batch(ctx, pairs, TR.PLANE, overlaps=np.full(320, 0.8), max_iterations=60)
    assert len(res) == 320
    same = 0
    for i, (r, pr) in enumerate(zip(res, pairs)):
        same += _check_record(r, pr.single(TR.PLANE, overlap=0.8, max_iterations=60), len(pr.src), i, info[i])
    assert sum(r.iterations >= 2 for r in res) == 320
    print("320 pairs: fitness bit-equal to the single call for %d" % same)


# ---- test 8: device variants, computed normals ----
def test_pair_above_the_row_cap(pkg, ctx):
    """stream_blocks saturates at 2048 rows: for a pair of more than 2048 * 256 sources the grid-stride term of the walk is live.
    Two passes each of the plane metric, the trimmed point metric and the trimmed plane metric, against the single-pair calls."""
    src, tgt = _bumpy(pkg, 60, 524800, 5.0)
    big = Pair(ctx, src, tgt[::175])
    small = Pair(ctx, *_bumpy(pkg, 61, 2000, 7.0, n_src=300))
    assert len(big.src) == 524800 > 2048 * 256 and len(big.tgt) <= 3000 and len(small.src) == 300
    pairs = [small, big]
    for kind in ("p2l", TR.POINT, TR.PLANE):
        ov = None if kind == "p2l" else np.array([0.6, 0.8], F64)
        res, info, _ = _run_batch(ctx, pairs, kind, overlaps=ov, max_iterations=2)
        for i, (r, pr) in enumerate(zip(res, pairs)):
            single = pr.single(kind, overlap=1.0 if ov is None else float(ov[i]), max_iterations=2)
            assert single["iterations"] == 2
            _check_record(r, single, len(pr.src), i, None if info is None else info[i])


def test_dev_variants_and_computed_normals(ctx, six):
    import torch
    pairs = [six[1], six[4], six[2]]
    s, so, t, to, nr = _pack(pairs)
    ov = np.array([0.5, 1.0, 0.25])
    ds, dt, dn = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (s, t, nr))
    torch.cuda.synchronize()
    p = ctx.icp_params(max_iterations=40)

    def same(a, b):
        for x, y in zip(a, b):
            assert _key(x, None) == _key(y, None) and x.pair_id == y.pair_id
            assert _f64_bits(x.fitness) == _f64_bits(y.fitness)

    h, _, _ = _run_batch(ctx, pairs, "p2l", max_iterations=40)
    same(h, ctx.icp_p2l_batch_dev(ds.data_ptr(), so, dt.data_ptr(), to, dn.data_ptr(), p))
    # NULL normals: kss_normals of each target rounded to float, which is what the pairs carry
    same(h, ctx.icp_p2l_batch_dev(ds.data_ptr(), so, dt.data_ptr(), to, None, p))
    same(h, _run_batch(ctx, pairs, "p2l", normals=False, max_iterations=40)[0])
    for metric in (TR.POINT, TR.PLANE):
        h, hi, _ = _run_batch(ctx, pairs, metric, overlaps=ov, max_iterations=40)
        for d_n in ((dn.data_ptr(), None) if metric == TR.PLANE else (None,)):
            d, di = ctx.icp_trimmed_batch_dev(ds.data_ptr(), so, dt.data_ptr(), to, d_n, p, overlaps=ov, metric=metric)
            same(h, d)
            assert np.array_equal(_bits(hi), _bits(di))
        # a sub-range of the packed arrays: offsets that do not start at 0
        d, di = ctx.icp_trimmed_batch_dev(ds.data_ptr(), so[1:], dt.data_ptr(), to[1:], dn.data_ptr() if metric == TR.PLANE else None, p,
                                          overlaps=ov[1:], metric=metric)
        for x, y in zip(d, h[1:]):
            assert _key(x, None) == _key(y, None)
        assert np.array_equal(_bits(di), _bits(hi[1:]))
    # overlaps = NULL: tp->overlap for every pair
    a, ai, _ = ctx.icp_trimmed_batch(s, so, t, to, None, overlaps=None, overlap=0.5, metric=TR.POINT, params=p)
    b, bi, _ = ctx.icp_trimmed_batch(s, so, t, to, None, overlaps=np.full(3, 0.5), metric=TR.POINT, params=p)
    same(a, b)
    assert np.array_equal(_bits(ai), _bits(bi))


# ---- test 9: argument errors ----
def test_argument_errors(pkg, ctx, six):
    w = _Witness(pkg, ctx)
    pairs = [six[1], six[2]]
    s, so, t, to, nr = _pack(pairs)

    def refused(call):
        with pytest.raises(pkg.KssError) as e:
            call()
        assert e.value.status == -1

    p = ctx.icp_params()
    p.allreduce = pkg.binding.ALLREDUCE_FN(lambda user, values, n: 0)
    refused(lambda: ctx.icp_p2l_batch(s, so, t, to, nr, params=p))
    refused(lambda: ctx.icp_trimmed_batch(s, so, t, to, nr, overlaps=np.array([0.5, 0.5]), metric=TR.PLANE, params=p))
    w.check()
    for bad in (0.0, -0.5, 1.0000001, float("nan")):
        refused(lambda: ctx.icp_trimmed_batch(s, so, t, to, None, overlaps=np.array([0.5, bad]), metric=TR.POINT))
        refused(lambda: ctx.icp_trimmed_batch(s, so, t, to, None, overlaps=None, overlap=bad, metric=TR.POINT))
        refused(lambda: ctx.trim_threshold_batch(np.ones(10, F32), [0, 4, 10], np.array([bad, 0.5])))
    refused(lambda: ctx.icp_trimmed_batch(s, so, t, to, nr, overlaps=np.array([0.5, 0.5]), metric=TR.POINT))      # normals with the point metric
    w.check()
    # an empty pair (source or target), an empty segment
    so_e = np.array([so[0], so[1], so[1], so[2]]); to_e = np.array([to[0], to[1], to[1] + 5, to[2]])
    refused(lambda: ctx.icp_p2l_batch(s, so_e, t, to_e, nr))
    to_e2 = np.array([to[0], to[1], to[1], to[2]]); so_e2 = np.array([so[0], so[1], so[1] + 5, so[2]])
    refused(lambda: ctx.icp_trimmed_batch(s, so_e2, t, to_e2, None, overlaps=np.full(3, 0.5), metric=TR.POINT))
    refused(lambda: ctx.trim_threshold_batch(np.ones(10, F32), [0, 4, 4, 10], np.full(3, 0.5)))
    w.check()
