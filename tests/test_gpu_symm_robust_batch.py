"""Robust symmetric ICP for many pairs per call (kss_icp_symm_robust_batch[_dev]).  The contract: every pair's
record -- T, iterations, state, converged, last_mse, its info, pair 0's traces -- is the single-pair kss_icp_symm_robust call's, bit
for bit; so nearly every check here compares bit patterns with that call on the pair alone (computed once per pair and setting, and
kept).  The independent restatement (tests/symm_robust_ref.py) anchors one pair inside a batch once more on its own.  The pairs are
symm_ref.halves_pair pairs and symm_robust_ref's scenes and outliers, their normals ctx.normals(cloud, 20) per cloud.  Every test
states what keeps it from passing vacuously: both per-pair tables are read from the second pass on, so the pairs must run it and end
at rotations of their own.  The conditions were checked with the restatement alone (on the oracle's NN and normals) when the seeds
and angles were chosen."""

import os

import numpy as np
import pytest

import robust_ref as RR
import symm_ref as S
import symm_robust_ref as SR

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
KW = dict(max_iterations=40)
FIXED = 0.05


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == F64 else np.uint32)


def _f64_bits(x):
    return int(np.array([x], F64).view(np.uint64)[0])


def _normals(ctx, cloud, k=20):
    return ctx.normals(cloud.astype(F64), k).astype(F32)


def _rp(pkg, loss, **kw):
    return pkg.robust_params(loss, RR.PLANE, **kw)


# ---- the clouds: functions of synth alone, so that the restatement can be run on them without a device ----
# (seed, n, n_src, degrees): DESIGN.md 2.15's eight pairs -- ragged, 1800 to 4000 points, every pair its own angle and axis
EIGHT = [(11, 2000, None, 5.0), (12, 2500, 1800, 8.0), (13, 1800, None, 12.0), (14, 4000, 3500, 15.0), (15, 3000, 2600, 6.5),
         (16, 2200, None, 10.0), (17, 3600, 2000, 13.5), (18, 2800, None, 7.0)]
SIZES = [1, 3, 63, 64, 65, 256, 257, 513, 20000]


def build_halves(synth, seed, n, deg, n_src=None, share=0.2, **kw):
    """(src, tgt, R_true, t_true): a halves_pair with the first `share` of the source pushed off the surface"""
    src, tgt, R, t = S.halves_pair(synth, seed, n, deg, n_src=n_src, **kw)
    if share > 0.0 and int(share * len(src)) > 0:
        src = SR.outliers(synth, src, seed, share)
    return src, tgt, R, t


def build_eight(synth):
    return [build_halves(synth, seed, n, deg, n_src=n_src) for seed, n, n_src, deg in EIGHT]


def build_sizes(synth):
    return [build_halves(synth, 40 + i, max(ns, 300), 6.0 + i, n_src=ns) for i, ns in enumerate(SIZES)]


def build_sixty_six(synth):
    rng = np.random.default_rng(66)
    out = []
    for i in range(66):
        n = int(rng.integers(500, 901))
        out.append(build_halves(synth, 100 + i, n, float(rng.uniform(3.0, 14.0)), n_src=int(rng.integers(500, n + 1))))
    return out


def build_narrow(synth):
    """the two narrow pairs of the headline batch: 10 degrees, 30 % outliers"""
    return [build_halves(synth, seed, 2000, 10.0, share=0.3) for seed in (21, 22)]


def build_endings(synth):
    """{name: (src, tgt)} of the four pairs of test_endings_do_not_leak; 'blind' gets NaN source normals from the test"""
    src, tgt, _, _ = build_halves(synth, 32, 2000, 5.0)
    away = (src + F32(100.0), tgt)
    blind = build_halves(synth, 33, 1500, 7.0, n_src=1200)[:2]
    _, tgt, _, _ = S.halves_pair(synth, 31, 1000, 5.0)
    src = tgt.copy()
    src[:400] += F32(0.5)                         # 40 % pushed away; the others lie on their targets
    early = (src, tgt)
    slow = build_halves(synth, 34, 1500, 60.0, n_src=1300)[:2]
    return {"away": away, "blind": blind, "early": early, "slow": slow}


def flip_quarter(sn, seed):
    out = sn.copy()
    out[np.random.default_rng(seed).random(len(out)) < 0.25] *= F32(-1.0)
    return out


# ---- pairs with their cached single-pair results ----
class Pair:
    """One pair with both clouds' normals and, computed once and kept, kss_icp_symm_robust's results on it."""

    def __init__(self, ctx, src, tgt, sn=None, tn=None, truth=None, seed=None):
        self.ctx = ctx
        self.src, self.tgt = np.ascontiguousarray(src, F32), np.ascontiguousarray(tgt, F32)
        self.sn = _normals(ctx, self.src) if sn is None else np.ascontiguousarray(sn, F32)
        self.tn = _normals(ctx, self.tgt) if tn is None else np.ascontiguousarray(tn, F32)
        self.truth = truth
        self.seed = seed
        self._single = {}

    def single(self, pkg, loss, scale=0.0, align=1, **kw):
        key = (loss, float(scale), align, tuple(sorted(kw.items())))
        if key not in self._single:
            self._single[key] = self.ctx.icp_symm_robust(self.src, self.tgt, self.sn, self.tn, sp=pkg.symm_params(align_normals=align),
                                                         rp=_rp(pkg, loss, scale=scale), params=self.ctx.icp_params(**kw), trace_cap=64)
        return self._single[key]


def _pairs(ctx, built, seeds=None):
    return [Pair(ctx, b[0], b[1], truth=(b[2], b[3]) if len(b) > 2 else None, seed=None if seeds is None else seeds[i])
            for i, b in enumerate(built)]


def _pack(pairs):
    so = np.concatenate([[0], np.cumsum([len(p.src) for p in pairs])]).astype(np.int64)
    to = np.concatenate([[0], np.cumsum([len(p.tgt) for p in pairs])]).astype(np.int64)
    return (np.concatenate([p.src for p in pairs]), so, np.concatenate([p.sn for p in pairs]),
            np.concatenate([p.tgt for p in pairs]), to, np.concatenate([p.tn for p in pairs]))


def _run(pkg, ctx, pairs, loss, scales=None, scale=0.0, aligns=None, sp=None, sn=True, tn=True, trace=False, **kw):
    """-> (list of IcpResult, info npairs x 4, extras of pair 0)"""
    s, so, ns_, t, to, nt_ = _pack(pairs)
    return ctx.icp_symm_robust_batch(s, so, t, to, ns_ if sn else None, nt_ if tn else None, aligns=aligns, scales=scales, sp=sp,
                                     rp=_rp(pkg, loss, scale=scale), params=ctx.icp_params(**kw), trace_cap=64 if trace else 0)


def _fitness_bound(ns, ref):
    # two summation orders of the NN engines' f64 sum of d2 over all sources differ by less than 2 n 2^-53 relative
    return 2.0 * ns * 2.0 ** -53 * ref


def _key(r, info):
    return (r.iterations, r.state, bool(r.converged), _bits(r.matrix()).tobytes(), _f64_bits(r.last_mse), _bits(info).tobytes())


def _check_record(r, info, single, ns, pair_id):
    """IcpResult r and its info row of a batch against kss_icp_symm_robust's dictionary."""
    assert r.pair_id == pair_id
    assert r.iterations == single["iterations"] and r.state == single["state"] and bool(r.converged) == single["converged"]
    assert np.array_equal(_bits(r.matrix()), _bits(single["T"]))
    assert _f64_bits(r.last_mse) == _f64_bits(single["last_mse"])
    assert np.array_equal(_bits(info), _bits(single["robust_info"]))
    assert abs(r.fitness - single["fitness"]) <= _fitness_bound(ns, single["fitness"])


def _check_trace(extra, single):
    assert np.array_equal(_bits(extra["trace_sums"]), _bits(single["trace_sums"]))
    assert np.array_equal(_bits(extra["trace_Tk"]), _bits(single["trace_Tk"]))
    assert np.array_equal(_bits(extra["trace_robust"]), _bits(single["trace_robust"]))


def _check_same(pairs, got, ginfo, want, winfo):
    """two batches' records of the same pairs"""
    for pr, a, ai, b, bi in zip(pairs, got, ginfo, want, winfo):
        assert _key(a, ai) == _key(b, bi)
        assert abs(a.fitness - b.fitness) <= _fitness_bound(len(pr.src), b.fitness)


def _own_rotations(res, at_least):
    """The records with two passes or more -- at_least of them -- end at pairwise different rotation bits, none the identity: one
    pair's rotation, or the identity, used for every pair could not give them."""
    later = [r for r in res if r.iterations >= 2]
    assert len(later) >= at_least
    rots = [_bits(r.matrix()[:3, :3]).tobytes() for r in later]
    assert len(set(rots)) == len(rots)
    assert all(not np.array_equal(r.matrix()[:3, :3], np.eye(3, dtype=F32)) for r in later)


@pytest.fixture(scope="module")
def eight(pkg, ctx):
    return _pairs(ctx, build_eight(pkg.synth), seeds=[e[0] for e in EIGHT])


@pytest.fixture(scope="module")
def flipped(ctx, eight):
    """the eight pairs with a quarter of each pair's source normals negated"""
    out = []
    for pr in eight:
        sn = flip_quarter(pr.sn, pr.seed)
        assert not np.array_equal(sn, pr.sn)
        out.append(Pair(ctx, pr.src, pr.tgt, sn, pr.tn, truth=pr.truth, seed=pr.seed))
    return out


def _scales_of(mode, n):
    """(scales argument, rp.scale, the scale of every pair)"""
    if mode == "fixed":
        return None, FIXED, [FIXED] * n
    if mode == "auto":
        return None, 0.0, [0.0] * n
    sc = [FIXED if i % 2 == 0 else 0.0 for i in range(n)]
    return np.array(sc), 0.0, sc


# ---- test 1: a ragged batch ----
@pytest.mark.parametrize("mode", ["fixed", "auto", "mixed"])
@pytest.mark.parametrize("loss", [RR.HUBER, RR.TUKEY, RR.CAUCHY, RR.L2], ids=["huber", "tukey", "cauchy", "l2"])
def test_ragged_batch_equals_single_calls(pkg, ctx, eight, loss, mode):
    scales, scale, per_pair = _scales_of(mode, len(eight))
    res, info, extra = _run(pkg, ctx, eight, loss, scales=scales, scale=scale, trace=True, **KW)
    assert len(res) == len(eight)
    print("passes", [r.iterations for r in res], "c2", [float(i[1]) for i in info])
    for i, (r, pr) in enumerate(zip(res, eight)):
        _check_record(r, info[i], pr.single(pkg, loss, scale=per_pair[i], **KW), len(pr.src), i)
    _check_trace(extra, eight[0].single(pkg, loss, scale=per_pair[0], **KW))
    _own_rotations(res, 6)
    if mode == "mixed":          # the fixed pairs took the fixed scale and the automatic ones a scale of their own
        for i, row in enumerate(info):
            assert (row[1] == FIXED * FIXED) == (per_pair[i] == FIXED), i


# ---- test 2: sizes ----
def test_sizes(pkg, ctx):
    """one, two and many partial rows in one launch (stream_blocks(ns) is 1 up to 256 sources), and pairs too small to run a pass"""
    pairs = _pairs(ctx, build_sizes(pkg.synth))
    assert [len(p.src) for p in pairs] == SIZES and all(len(p.tgt) >= 30 for p in pairs)
    order = [8, 0, 5, 1, 6, 2, 7, 3, 4]                   # the large pair first: the small ones' row_base is not their index
    res, info, _ = _run(pkg, ctx, [pairs[i] for i in order], RR.TUKEY, **KW)
    zero_pass = 0
    for j, i in enumerate(order):
        single = pairs[i].single(pkg, RR.TUKEY, **KW)
        print("ns %d: %d passes, state %d, info %s" % (SIZES[i], single["iterations"], single["state"], single["robust_info"]))
        _check_record(res[j], info[j], single, SIZES[i], j)
        if single["iterations"] == 0:
            assert single["state"] in (5, pkg.STATE_DEGENERATE)
            zero_pass += 1
    assert zero_pass >= 1
    assert sum(r.iterations >= 2 for r in res) >= 5


# ---- test 3: invariances ----
def test_order_split_subrange_and_one_pair(pkg, ctx, eight):
    n = len(eight)
    sc = np.array([FIXED if i % 2 == 0 else 0.0 for i in range(n)])
    base, binfo, _ = _run(pkg, ctx, eight, RR.TUKEY, scales=sc, **KW)
    rev, rinfo, _ = _run(pkg, ctx, eight[::-1], RR.TUKEY, scales=sc[::-1].copy(), **KW)
    assert [r.pair_id for r in rev] == list(range(n))
    _check_same(eight, rev[::-1], rinfo[::-1], base, binfo)
    a, ai, _ = _run(pkg, ctx, eight[:3], RR.TUKEY, scales=sc[:3], **KW)
    b, bi, _ = _run(pkg, ctx, eight[3:], RR.TUKEY, scales=sc[3:], **KW)
    _check_same(eight, a + b, np.concatenate([ai, bi]), base, binfo)
    # one call on a sub-range of the packed arrays: offsets whose first entry is not 0
    s, so, sn, t, to, tn = _pack(eight)
    sub, sinfo, _ = ctx.icp_symm_robust_batch(s, so[2:7], t, to[2:7], sn, tn, scales=sc[2:6], rp=_rp(pkg, RR.TUKEY), params=ctx.icp_params(**KW))
    assert [r.pair_id for r in sub] == list(range(4))
    _check_same(eight[2:6], sub, sinfo, base[2:6], binfo[2:6])
    for r, inf, pr, c in zip(sub, sinfo, eight[2:6], sc[2:6]):
        _check_record(r, inf, pr.single(pkg, RR.TUKEY, scale=c, **KW), len(pr.src), r.pair_id)
    # a batch of one
    for i in (3, 0):
        one, oinfo, extra = _run(pkg, ctx, [eight[i]], RR.TUKEY, scales=sc[i:i + 1], trace=True, **KW)
        single = eight[i].single(pkg, RR.TUKEY, scale=sc[i], **KW)
        assert len(one) == 1 and single["iterations"] >= 2
        _check_record(one[0], oinfo[0], single, len(eight[i].src), 0)
        _check_trace(extra, single)
    _own_rotations(base, 6)


# ---- test 4: the L2 batch is the symmetric batch ----
def test_l2_batch_is_the_symmetric_batch(pkg, ctx, eight):
    s, so, sn, t, to, tn = _pack(eight)
    want, _ = ctx.icp_symm_batch(s, so, t, to, sn, tn, params=ctx.icp_params(**KW))
    for scale in (FIXED, 0.0):
        res, _, _ = _run(pkg, ctx, eight, RR.L2, scale=scale, **KW)
        for r, q in zip(res, want):
            assert (r.iterations, r.state, _bits(r.matrix()).tobytes(), _f64_bits(r.last_mse)) == (
                q.iterations, q.state, _bits(q.matrix()).tobytes(), _f64_bits(q.last_mse))
    _own_rotations(want, 6)


# ---- test 5: the headline inside a batch ----
def test_headline_scenes_inside_a_batch(pkg, ctx):
    """DESIGN.md 2.19's two scenes and bars beside two narrow pairs: only the combination registers A and B"""
    kw = dict(max_iterations=100)
    a, b = SR.scene_a(pkg.synth), SR.scene_b(pkg.synth)
    pairs = _pairs(ctx, [a, b] + build_narrow(pkg.synth))
    res, info, _ = _run(pkg, ctx, pairs, RR.TUKEY, **kw)
    for i, (r, pr) in enumerate(zip(res, pairs)):
        _check_record(r, info[i], pr.single(pkg, RR.TUKEY, **kw), len(pr.src), i)
    s, so, sn, t, to, tn = _pack(pairs)
    plain, _ = ctx.icp_symm_batch(s, so, t, to, sn, tn, params=ctx.icp_params(**kw))
    p2l, _, _ = ctx.icp_robust_batch(s, so, t, to, tn, rp=_rp(pkg, RR.TUKEY), params=ctx.icp_params(**kw))
    for r, q, w, pr, bar, name in zip(res[:2], plain[:2], p2l[:2], pairs[:2], (3e-3, 2e-2), "AB"):
        eR, et = SR.errors(r.matrix(), *pr.truth)
        eS, eP = SR.errors(q.matrix(), *pr.truth)[0], SR.errors(w.matrix(), *pr.truth)[0]
        print("scene %s: %d passes, state %d, |R - R_true| %.2e, |t - t_true| %.2e; plain symmetric %.2e, Tukey point-to-plane %.2e" % (
            name, r.iterations, r.state, eR, et, eS, eP))
        assert r.converged and r.state in (2, 3, 4)
        assert eR <= 1e-3
        assert eS >= bar
        assert eP >= 0.5


# ---- test 6: the align_normals of every pair ----
def test_per_pair_align(pkg, ctx, eight, flipped):
    """a quarter of each pair's source normals are negated: without the flips one pair gives the same bits at align 0 and 1"""
    n = len(flipped)
    aligns = np.array([1 - i % 2 for i in range(n)], np.int32)      # 1, 0, 1, 0, ...
    res, info, extra = _run(pkg, ctx, flipped, RR.TUKEY, aligns=aligns, trace=True, **KW)
    for i, (r, pr) in enumerate(zip(res, flipped)):
        _check_record(r, info[i], pr.single(pkg, RR.TUKEY, align=int(aligns[i]), **KW), len(pr.src), i)
    _check_trace(extra, flipped[0].single(pkg, RR.TUKEY, align=1, **KW))
    # no table: sp->align_normals for every pair
    res0, info0, _ = _run(pkg, ctx, flipped, RR.TUKEY, sp=pkg.symm_params(align_normals=0), **KW)
    for i, (r, pr) in enumerate(zip(res0, flipped)):
        _check_record(r, info0[i], pr.single(pkg, RR.TUKEY, align=0, **KW), len(pr.src), i)
    # the sign invariance at align 1: the record with the flips is the record without them, bit for bit, the keys-derived c2 and
    # the info included
    res1, info1, _ = _run(pkg, ctx, flipped, RR.TUKEY, aligns=np.ones(n, np.int32), sp=pkg.symm_params(align_normals=0), **KW)
    plain, pinfo, _ = _run(pkg, ctx, eight, RR.TUKEY, **KW)
    for i, (r, q, pr) in enumerate(zip(res1, plain, eight)):
        assert _key(r, info1[i]) == _key(q, pinfo[i])
        _check_record(r, info1[i], pr.single(pkg, RR.TUKEY, align=1, **KW), len(pr.src), i)
    assert all(row[1] > 0.0 and row[1] != FIXED * FIXED for row in info1)
    # (void otherwise) the two settings give different matrices
    differ = sum(_bits(a.matrix()).tobytes() != _bits(b.matrix()).tobytes() for a, b in zip(res0, res1))
    print("align 0 and 1 differ for %d of %d pairs" % (differ, n))
    assert differ >= 6


# ---- test 7: endings ----
def test_endings_do_not_leak(pkg, ctx, eight):
    kw = dict(max_iterations=6)
    e = build_endings(pkg.synth)
    away, early, slow = Pair(ctx, *e["away"]), Pair(ctx, *e["early"]), Pair(ctx, *e["slow"])
    blind = Pair(ctx, *e["blind"], sn=np.full((len(e["blind"][0]), 3), np.nan, F32))
    healthy = [eight[1], eight[4], eight[6]]
    pairs = [eight[1], away, early, eight[4], blind, slow, eight[6]]
    ending = (1, 2, 4, 5)
    res, info, _ = _run(pkg, ctx, pairs, RR.TUKEY, **kw)
    print("passes", [r.iterations for r in res], "states", [r.state for r in res])
    for i, (r, pr) in enumerate(zip(res, pairs)):
        _check_record(r, info[i], pr.single(pkg, RR.TUKEY, **kw), len(pr.src), i)
    for i in (1, 4):             # no candidate at all: no pass, the identity, an all-zero info row
        assert res[i].state == 5 and res[i].iterations == 0 and not res[i].converged
        assert np.array_equal(res[i].matrix(), np.eye(4, dtype=F32))
        assert np.array_equal(info[i], np.zeros(4))
    one = early.single(pkg, RR.TUKEY, **kw)                # (what "early" means is the single call's record)
    assert one["iterations"] < 6 and res[2].iterations == one["iterations"] and bool(res[2].converged) == one["converged"]
    assert res[5].iterations == 6 and res[5].state == 1      # (PCL's criteria count the iteration limit as converged)
    assert slow.single(pkg, RR.TUKEY, max_iterations=100)["iterations"] > 6
    assert all(res[i].iterations >= 2 for i in (0, 3, 6))
    alone, ainfo, _ = _run(pkg, ctx, healthy, RR.TUKEY, **kw)
    keep = [i for i in range(len(pairs)) if i not in ending]
    _check_same(healthy, [res[i] for i in keep], [info[i] for i in keep], alone, ainfo)


# ---- test 8: NN engines, tuning knobs and the table's transport ----
def test_engines_and_knobs_bit_identical(pkg, ctx, eight):
    sc = np.array([FIXED if i % 2 == 0 else 0.0 for i in range(len(eight))])
    base, binfo, _ = _run(pkg, ctx, eight, RR.TUKEY, scales=sc, **KW)
    for i, (r, pr) in enumerate(zip(base, eight)):
        _check_record(r, binfo[i], pr.single(pkg, RR.TUKEY, scale=sc[i], **KW), len(pr.src), i)
    for more in (dict(nn_mode=pkg.NN_BRUTE), dict(nn_mode=pkg.NN_GRID), dict(nn_mode=pkg.NN_AUTO),
                 dict(nn_mode=pkg.NN_BRUTE, nn_sources_per_thread=1, nn_target_splits=3),
                 dict(nn_mode=pkg.NN_BRUTE, nn_sources_per_thread=8, nn_target_splits=1)):
        res, info, _ = _run(pkg, ctx, eight, RR.TUKEY, scales=sc, **dict(KW, **more))
        _check_same(eight, res, info, base, binfo)
    old = os.environ.get("KSS_GICP_TABLE_MAPPED")
    os.environ["KSS_GICP_TABLE_MAPPED"] = "1"             # the kernels read the pinned table across the bus: the same bits
    try:
        res, info, _ = _run(pkg, ctx, eight, RR.TUKEY, scales=sc, **KW)
    finally:
        if old is None:
            del os.environ["KSS_GICP_TABLE_MAPPED"]
        else:
            os.environ["KSS_GICP_TABLE_MAPPED"] = old
    _check_same(eight, res, info, base, binfo)
    _own_rotations(base, 6)


# ---- test 9: the host pool does the solves from 64 pairs up ----
def test_host_pool_path(pkg, ctx):
    pairs = _pairs(ctx, build_sixty_six(pkg.synth))
    sc = np.array([FIXED if i % 3 == 0 else 0.0 for i in range(66)])
    res, info, extra = _run(pkg, ctx, pairs, RR.TUKEY, scales=sc, trace=True, **KW)
    assert len(res) == 66
    for i, (r, pr) in enumerate(zip(res, pairs)):
        _check_record(r, info[i], pr.single(pkg, RR.TUKEY, scale=sc[i], **KW), len(pr.src), i)
    _check_trace(extra, pairs[0].single(pkg, RR.TUKEY, scale=sc[0], **KW))
    assert sum(r.iterations >= 2 for r in res) >= 60
    _own_rotations(res, 60)


# ---- test 10: device pointers ----
def test_dev_matches_host(pkg, ctx, eight, flipped):
    import torch
    pairs = flipped[2:6]
    s, so, sn, t, to, tn = _pack(pairs)
    ds, dsn, dt, dtn = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (s, sn, t, tn))
    torch.cuda.synchronize()
    aligns = np.array([1, 0, 0, 1], np.int32)
    sc = np.array([0.0, FIXED, 0.0, FIXED])
    rp = _rp(pkg, RR.TUKEY)
    host, hinfo, hextra = _run(pkg, ctx, pairs, RR.TUKEY, scales=sc, aligns=aligns, trace=True, **KW)
    for i, (r, pr) in enumerate(zip(host, pairs)):
        _check_record(r, hinfo[i], pr.single(pkg, RR.TUKEY, scale=sc[i], align=int(aligns[i]), **KW), len(pr.src), i)
    assert all(r.iterations >= 2 for r in host)
    # computed source normals carry no flips: at align 0 they give other records, so each combination has its own host run
    for has_s, has_t in ((True, True), (False, True), (True, False), (False, False)):
        want, winfo, wextra = (host, hinfo, hextra) if has_s and has_t else _run(pkg, ctx, pairs, RR.TUKEY, scales=sc, aligns=aligns,
                                                                                 sn=has_s, tn=has_t, trace=True, **KW)
        dev, dinfo, dextra = ctx.icp_symm_robust_batch_dev(ds.data_ptr(), so, dsn.data_ptr() if has_s else None, dt.data_ptr(), to,
                                                           dtn.data_ptr() if has_t else None, params=ctx.icp_params(**KW), aligns=aligns,
                                                           scales=sc, rp=rp, trace_cap=64)
        assert [r.pair_id for r in dev] == list(range(len(pairs)))
        assert [_key(r, i) for r, i in zip(dev, dinfo)] == [_key(r, i) for r, i in zip(want, winfo)]
        assert [_f64_bits(r.fitness) for r in dev] == [_f64_bits(r.fitness) for r in want]
        _check_trace(dextra, wextra)
    # a sub-range of the device arrays
    dev, dinfo, _ = ctx.icp_symm_robust_batch_dev(ds.data_ptr(), so[1:], dsn.data_ptr(), dt.data_ptr(), to[1:], dtn.data_ptr(),
                                                  params=ctx.icp_params(**KW), aligns=aligns[1:], scales=sc[1:], rp=rp)
    assert [_key(r, i) for r, i in zip(dev, dinfo)] == [_key(r, i) for r, i in zip(host[1:], hinfo[1:])]
    # normals_k is read where a set is computed
    four = eight[:4]
    at12 = [Pair(ctx, p.src, p.tgt, _normals(ctx, p.src, 12), _normals(ctx, p.tgt, 12)) for p in four]
    given, ginfo, _ = _run(pkg, ctx, at12, RR.TUKEY, **KW)
    computed, cinfo, _ = _run(pkg, ctx, four, RR.TUKEY, sn=False, tn=False, sp=pkg.symm_params(normals_k=12), **KW)
    _check_same(four, computed, cinfo, given, ginfo)
    at20, info20, _ = _run(pkg, ctx, four, RR.TUKEY, **KW)
    assert [_key(r, i) for r, i in zip(given, ginfo)] != [_key(r, i) for r, i in zip(at20, info20)]


# ---- test 11: the independent restatement ----
def test_pair_in_a_batch_matches_restatement(pkg, ctx, O, eight):
    """scene A inside a batch of three against symm_robust_ref.icp_symm_robust at test_gpu_symm_robust.py's tolerances"""
    src, tgt, R_true, t_true = SR.scene_a(pkg.synth)
    pr = Pair(ctx, src, tgt, truth=(R_true, t_true))
    res, info, extra = _run(pkg, ctx, [pr, eight[2], eight[5]], RR.TUKEY, trace=True, max_iterations=100)
    got = res[0]
    ref = SR.icp_symm_robust(O, pr.src, pr.sn, pr.tgt, pr.tn, RR.TUKEY, max_iterations=100)
    s0, r0 = extra["trace_sums"][0], ref["trace_sums"][0]
    print("%d / %d passes, |trace_Tk| %.2e  |T| %.2e  |fitness| %.2e  first sums %.2e" % (
        got.iterations, ref["iterations"],
        np.abs(extra["trace_Tk"] - ref["trace_Tk"]).max() if got.iterations == ref["iterations"] else -1.0,
        np.abs(got.matrix() - ref["T"]).max(), abs(got.fitness - ref["fitness"]), (np.abs(s0 - r0) / np.maximum(np.abs(r0), 1.0)).max()))
    assert got.iterations == ref["iterations"] >= 2
    assert got.state == ref["state"] and bool(got.converged) == ref["converged"]
    assert np.abs(extra["trace_Tk"] - ref["trace_Tk"]).max() <= 1e-6
    assert np.abs(got.matrix() - ref["T"]).max() <= 5e-6
    assert abs(got.fitness - ref["fitness"]) <= 1e-9 * max(1.0, ref["fitness"])
    i0, j0 = extra["trace_robust"][0], ref["trace_robust"][0]
    assert i0[0] == j0[0] and i0[3] == j0[3]
    assert _bits(i0[1:2])[0] == _bits(j0[1:2])[0]
    assert np.all(np.abs(s0 - r0) <= 1e-9 * np.maximum(np.abs(r0), 1.0))
    assert np.array_equal(_bits(info[0]), _bits(extra["trace_robust"][-1]))
    eR, et = SR.errors(got.matrix(), R_true, t_true)
    print("|R - R_true| %.2e, |t - t_true| %.2e" % (eR, et))
    assert eR <= 1e-3 and et <= 1e-3


# ---- test 12: bad arguments ----
def test_bad_arguments(pkg, ctx, eight):
    pairs = eight[:2]
    s, so, sn, t, to, tn = _pack(pairs)
    tukey = lambda: _rp(pkg, RR.TUKEY)                      # noqa: E731
    before = (ctx.icp_symm_batch(s, so, t, to, sn, tn)[0], ctx.icp_robust_batch(s, so, t, to, tn, rp=tukey())[:2],
              ctx.icp_symm_robust(pairs[0].src, pairs[0].tgt, pairs[0].sn, pairs[0].tn, rp=tukey()))

    def refused(call):
        with pytest.raises(pkg.KssError) as e:
            call()
        assert e.value.status == -1

    def batch(**kw):
        kw.setdefault("rp", tukey())
        return ctx.icp_symm_robust_batch(s, so, t, to, kw.pop("sn", sn), kw.pop("tn", tn), **kw)

    batch(params=ctx.icp_params(max_iterations=2))        # (the call the refusals below vary is accepted)
    nan, inf = float("nan"), float("inf")
    # what kss_icp_symm_batch refuses
    for bad in (2, -1):
        refused(lambda: batch(aligns=np.array([1, bad])))
        refused(lambda: batch(aligns=np.array([bad, 0])))
        refused(lambda: batch(sp=pkg.symm_params(align_normals=bad)))
    p = ctx.icp_params()
    p.allreduce = pkg.binding.ALLREDUCE_FN(lambda user, values, n: 0)
    refused(lambda: batch(params=p))
    refused(lambda: ctx.icp_symm_robust_batch(s, np.array([0, so[1], so[1]]), t, to, sn, tn, rp=tukey()))          # an empty pair
    refused(lambda: ctx.icp_symm_robust_batch(s, so, t, np.array([0, 0, to[2]]), sn, tn, rp=tukey()))
    for k in (2, 65):                                      # normals_k is checked where a set of normals has to be computed
        refused(lambda: batch(sn=None, sp=pkg.symm_params(normals_k=k)))
        refused(lambda: batch(tn=None, sp=pkg.symm_params(normals_k=k)))
        batch(sp=pkg.symm_params(normals_k=k), params=ctx.icp_params(max_iterations=2))
    # what kss_icp_symm_robust refuses in rp
    refused(lambda: batch(rp=pkg.robust_params(RR.TUKEY, RR.POINT)))
    for field, values in (("loss", (-1, 4)), ("metric", (-1, 2)), ("scale", (-0.5, inf, nan)), ("tune", (0.0, -1.0, inf, nan)),
                          ("min_scale", (-0.5,))):
        for v in values:
            rp = tukey()
            setattr(rp, field, v)
            refused(lambda: batch(rp=rp))
    # the per-pair scales
    for v in (-0.5, -inf, inf, nan):
        refused(lambda: batch(scales=np.array([FIXED, v])))
        refused(lambda: batch(scales=np.array([v, 0.0])))
    for v in (0.0, -1.0, inf, nan):                        # an automatic pair needs a tune; a batch of fixed pairs does not read it
        rp = _rp(pkg, RR.TUKEY, scale=FIXED)
        rp.tune = v
        refused(lambda: batch(rp=rp, scales=np.array([FIXED, 0.0])))
        batch(rp=rp, scales=np.array([FIXED, FIXED]), params=ctx.icp_params(max_iterations=2))
    # the context still works, and everything gives what it gave
    res, info, _ = _run(pkg, ctx, pairs, RR.TUKEY, **KW)
    for i, (r, pr) in enumerate(zip(res, pairs)):
        _check_record(r, info[i], pr.single(pkg, RR.TUKEY, **KW), len(pr.src), i)
    assert all(r.iterations >= 2 for r in res)
    after = (ctx.icp_symm_batch(s, so, t, to, sn, tn)[0], ctx.icp_robust_batch(s, so, t, to, tn, rp=tukey())[:2],
             ctx.icp_symm_robust(pairs[0].src, pairs[0].tgt, pairs[0].sn, pairs[0].tn, rp=tukey()))
    for x, y in zip(before[0], after[0]):
        assert (x.iterations, x.state, _bits(x.matrix()).tobytes(), _f64_bits(x.fitness)) == (
            y.iterations, y.state, _bits(y.matrix()).tobytes(), _f64_bits(y.fitness))
    for (x, xi), (y, yi) in zip(zip(*before[1]), zip(*after[1])):
        assert _key(x, xi) == _key(y, yi) and _f64_bits(x.fitness) == _f64_bits(y.fitness)
    assert np.array_equal(_bits(before[2]["T"]), _bits(after[2]["T"])) and before[2]["iterations"] == after[2]["iterations"]
    assert np.array_equal(_bits(before[2]["robust_info"]), _bits(after[2]["robust_info"]))
