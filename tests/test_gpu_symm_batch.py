"""Symmetric ICP for many pairs per call (kss_icp_symm_batch[_dev]).  The contract: every pair's record is the
single-pair call's, bit for bit -- so nearly every check here is a comparison of bit patterns with kss_icp_symm on the pair alone;
the independent restatement (tests/symm_ref.py) anchors one pair inside a batch once more on its own.  The pairs are two
independent samplings of one surface (symm_ref.halves_pair), their normals ctx.normals(cloud, 20) per cloud.  Every test states
what keeps it from passing vacuously: the per-pair rotation table is read from the second pass on, so the pairs must run it and
end at rotations of their own."""

import numpy as np
import pytest

import symm_ref as S

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
KW = dict(max_iterations=40)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == F64 else np.uint32)


def _f64_bits(x):
    return int(np.array([x], F64).view(np.uint64)[0])


def _normals(ctx, cloud, k=20):
    return ctx.normals(cloud.astype(F64), k).astype(F32)


class Pair:
    """One pair with both clouds' normals and, computed once and kept, kss_icp_symm's results on it."""

    def __init__(self, ctx, src, tgt, sn=None, tn=None, truth=None, seed=None):
        self.ctx = ctx
        self.src, self.tgt = np.ascontiguousarray(src, F32), np.ascontiguousarray(tgt, F32)
        self.sn = _normals(ctx, self.src) if sn is None else np.ascontiguousarray(sn, F32)
        self.tn = _normals(ctx, self.tgt) if tn is None else np.ascontiguousarray(tn, F32)
        self.truth = truth
        self.seed = seed
        self._single = {}

    def single(self, pkg, align=1, **kw):
        key = (align, tuple(sorted(kw.items())))
        if key not in self._single:
            self._single[key] = self.ctx.icp_symm(self.src, self.tgt, self.sn, self.tn, sp=pkg.symm_params(align_normals=align),
                                                  params=self.ctx.icp_params(**kw), trace_cap=64)
        return self._single[key]


def _halves(pkg, ctx, seed, n, deg, n_src=None, **kw):
    src, tgt, R, t = S.halves_pair(pkg.synth, seed, n, deg, n_src=n_src, **kw)
    return Pair(ctx, src, tgt, truth=(R, t), seed=seed)


def _pack(pairs):
    so = np.concatenate([[0], np.cumsum([len(p.src) for p in pairs])]).astype(np.int64)
    to = np.concatenate([[0], np.cumsum([len(p.tgt) for p in pairs])]).astype(np.int64)
    return (np.concatenate([p.src for p in pairs]), so, np.concatenate([p.sn for p in pairs]),
            np.concatenate([p.tgt for p in pairs]), to, np.concatenate([p.tn for p in pairs]))


def _run(pkg, ctx, pairs, aligns=None, sp=None, sn=True, tn=True, trace=False, **kw):
    """-> (list of IcpResult, extras of pair 0)"""
    s, so, ns_, t, to, nt_ = _pack(pairs)
    return ctx.icp_symm_batch(s, so, t, to, ns_ if sn else None, nt_ if tn else None, aligns=aligns, sp=sp,
                              params=ctx.icp_params(**kw), trace_cap=64 if trace else 0)


def _fitness_bound(ns, ref):
    # test_gpu_pairs_batch.py's bound for two summation orders of the NN engines' f64 sum of d2 over all sources: each order is
    # within (n - 1) 2^-53 relative of the exact sum of the non-negative terms, two orders differ by less than 2 n 2^-53 relative
    return 2.0 * ns * 2.0 ** -53 * ref


def _key(r):
    return (r.iterations, r.state, bool(r.converged), _bits(r.matrix()).tobytes(), _f64_bits(r.last_mse))


def _check_record(r, single, ns, pair_id):
    """IcpResult r of a batch against kss_icp_symm's dictionary."""
    assert r.pair_id == pair_id
    assert r.iterations == single["iterations"] and r.state == single["state"] and bool(r.converged) == single["converged"]
    assert np.array_equal(_bits(r.matrix()), _bits(single["T"]))
    assert _f64_bits(r.last_mse) == _f64_bits(single["last_mse"])
    assert abs(r.fitness - single["fitness"]) <= _fitness_bound(ns, single["fitness"])


def _check_trace(extra, single):
    assert np.array_equal(_bits(extra["trace_sums"]), _bits(single["trace_sums"]))
    assert np.array_equal(_bits(extra["trace_Tk"]), _bits(single["trace_Tk"]))


def _check_same(pairs, got, want):
    """two batches' records of the same pairs"""
    for pr, a, b in zip(pairs, got, want):
        assert _key(a) == _key(b)
        assert abs(a.fitness - b.fitness) <= _fitness_bound(len(pr.src), b.fitness)


def _own_rotations(res, at_least):
    """The records with two passes or more -- at_least of them -- end at pairwise different rotation bits, none the identity: one
    pair's rotation, or the identity, used for every pair could not give them."""
    later = [r for r in res if r.iterations >= 2]
    assert len(later) >= at_least
    rots = [_bits(r.matrix()[:3, :3]).tobytes() for r in later]
    assert len(set(rots)) == len(rots)
    assert all(not np.array_equal(r.matrix()[:3, :3], np.eye(3, dtype=F32)) for r in later)


# (seed, n, n_src, degrees): test_gpu_gicp_batch.py's list -- ragged, 1800 to 4000 points, every pair its own angle and axis
EIGHT = [(11, 2000, None, 5.0), (12, 2500, 1800, 8.0), (13, 1800, None, 12.0), (14, 4000, 3500, 15.0), (15, 3000, 2600, 6.5),
         (16, 2200, None, 10.0), (17, 3600, 2000, 13.5), (18, 2800, None, 7.0)]


@pytest.fixture(scope="module")
def eight(pkg, ctx):
    return [_halves(pkg, ctx, seed, n, deg, n_src=n_src) for seed, n, n_src, deg in EIGHT]


@pytest.fixture(scope="module")
def flipped(ctx, eight):
    """the eight pairs with a quarter of each pair's source normals negated"""
    out = []
    for pr in eight:
        sn = pr.sn.copy()
        sn[np.random.default_rng(pr.seed).random(len(sn)) < 0.25] *= F32(-1.0)
        assert not np.array_equal(sn, pr.sn)
        out.append(Pair(ctx, pr.src, pr.tgt, sn, pr.tn, truth=pr.truth, seed=pr.seed))
    return out


# ---- test 1: a ragged batch ----
def test_ragged_batch_equals_single_calls(pkg, ctx, eight):
    """the restatement runs every one of the eight pairs 3 or 4 passes"""
    res, extra = _run(pkg, ctx, eight, trace=True, **KW)
    assert len(res) == len(eight)
    print("passes", [r.iterations for r in res])
    for i, (r, pr) in enumerate(zip(res, eight)):
        _check_record(r, pr.single(pkg, **KW), len(pr.src), i)
    _check_trace(extra, eight[0].single(pkg, **KW))
    _own_rotations(res, 6)


# ---- test 2: row boundaries ----
def test_row_boundary_sizes(pkg, ctx):
    """one, two and many partial rows in one launch: stream_blocks(ns) is 1 up to 256 sources.  The restatement: ns = 1 ends with
    state 5 and ns = 3 with state 6, both at 0 passes; ns = 63, 64, 65 run all 40 passes (the table is rewritten 39 times); the
    rest run 5."""
    sizes = [1, 3, 63, 64, 65, 256, 257, 513, 20000]
    pairs = [_halves(pkg, ctx, 40 + i, max(ns, 300), 6.0 + i, n_src=ns) for i, ns in enumerate(sizes)]
    assert [len(p.src) for p in pairs] == sizes and all(len(p.tgt) >= 30 for p in pairs)
    order = [8, 0, 5, 1, 6, 2, 7, 3, 4]                   # the large pair first: the small ones' row_base is not their index
    res, _ = _run(pkg, ctx, [pairs[i] for i in order], **KW)
    for j, i in enumerate(order):
        single = pairs[i].single(pkg, **KW)
        print("ns %d: %d passes, state %d" % (sizes[i], single["iterations"], single["state"]))
        _check_record(res[j], single, sizes[i], j)
    assert sum(r.iterations >= 2 for r in res) >= 5


def test_pair_above_the_row_cap(pkg, ctx):
    """stream_blocks saturates at 2048 rows: for a pair of more than 2048 * 256 sources the grid-stride term of the walk is live.
    Two passes of a batch {300 sources, 524 800 sources} against the single-pair calls.  (The large pair's source normals are the
    radial directions -- the surface is star-shaped --, not 524 800 computed ones: the comparison is of bits, whatever the normals.)"""
    Sy = pkg.synth
    src, tgt = Sy.make_pair(60, 524800, R=Sy.rot_axis_angle(Sy.sphere(7060, 1)[0], np.deg2rad(5.0)), t=(0.02, -0.01, 0.03), shape="bumpy")
    sn = (src / np.sqrt((src.astype(F64) ** 2).sum(axis=1, keepdims=True))).astype(F32)
    big = Pair(ctx, src, tgt[::175], sn=sn)
    small = _halves(pkg, ctx, 61, 300, 7.0)
    assert len(big.src) == 524800 > 2048 * 256 and len(big.tgt) <= 3000 and len(small.src) == 300
    pairs = [small, big]
    res, _ = _run(pkg, ctx, pairs, max_iterations=2)
    for i, (r, pr) in enumerate(zip(res, pairs)):
        single = pr.single(pkg, max_iterations=2)
        assert single["iterations"] == 2
        _check_record(r, single, len(pr.src), i)


# ---- test 3: order and split ----
def test_order_and_split(pkg, ctx, eight):
    n = len(eight)
    base, _ = _run(pkg, ctx, eight, **KW)
    rev, _ = _run(pkg, ctx, eight[::-1], **KW)
    assert [r.pair_id for r in rev] == list(range(n))
    _check_same(eight, rev[::-1], base)
    a, _ = _run(pkg, ctx, eight[:3], **KW)
    b, _ = _run(pkg, ctx, eight[3:], **KW)
    _check_same(eight, a + b, base)
    # one call on a sub-range of the packed arrays: offsets whose first entry is not 0
    s, so, sn, t, to, tn = _pack(eight)
    sub, _ = ctx.icp_symm_batch(s, so[2:7], t, to[2:7], sn, tn, params=ctx.icp_params(**KW))
    assert [r.pair_id for r in sub] == list(range(4))
    _check_same(eight[2:6], sub, base[2:6])
    for r, pr in zip(sub, eight[2:6]):
        _check_record(r, pr.single(pkg, **KW), len(pr.src), r.pair_id)


# ---- test 4: wide angles ----
def test_wide_angles_where_point_to_plane_fails(pkg, ctx, eight):
    """two pairs of 2 x 2000 points 65 degrees apart about (0.3, -0.5, 1) beside two narrow ones.  The restatement gives the wide
    pairs 7 passes each and 2.9e-4 / 1.4e-4 in R; its point-to-plane ends 1.21 / 1.17 away."""
    wide = [_halves(pkg, ctx, seed, 2000, 65.0, axis=[0.3, -0.5, 1.0]) for seed in (8, 21)]
    pairs = wide + [eight[0], eight[3]]
    res, _ = _run(pkg, ctx, pairs, **KW)
    for i, (r, pr) in enumerate(zip(res, pairs)):
        _check_record(r, pr.single(pkg, **KW), len(pr.src), i)
    s, so, _, t, to, tn = _pack(pairs)
    p2l, _ = ctx.icp_p2l_batch(s, so, t, to, tn, params=ctx.icp_params(**KW))
    for r, q, pr in zip(res[:2], p2l[:2], wide):
        eR, et = S.errors(r.matrix(), *pr.truth)
        pR, _ = S.errors(q.matrix(), *pr.truth)
        print("symmetric: %d passes, state %d, |R - R_true| %.2e, |t - t_true| %.2e;  point-to-plane: %d passes, %.2e" % (
            r.iterations, r.state, eR, et, q.iterations, pR))
        assert r.converged and r.state in (2, 3, 4)
        assert eR <= 1e-3
        assert pR >= 0.5


# ---- test 5: the align_normals of every pair ----
def test_per_pair_align(pkg, ctx, eight, flipped):
    """a quarter of each pair's source normals are negated: without the flips one pair gives the same bits at align 0 and 1"""
    n = len(flipped)
    aligns = np.array([1 - i % 2 for i in range(n)], np.int32)      # 1, 0, 1, 0, ...
    res, extra = _run(pkg, ctx, flipped, aligns=aligns, trace=True, **KW)
    for i, (r, pr) in enumerate(zip(res, flipped)):
        _check_record(r, pr.single(pkg, align=int(aligns[i]), **KW), len(pr.src), i)
    _check_trace(extra, flipped[0].single(pkg, align=1, **KW))
    # no table: sp->align_normals for every pair
    res0, _ = _run(pkg, ctx, flipped, sp=pkg.symm_params(align_normals=0), **KW)
    for i, (r, pr) in enumerate(zip(res0, flipped)):
        _check_record(r, pr.single(pkg, align=0, **KW), len(pr.src), i)
    # the sign invariance at align 1: the record with the flips is the record without them, bit for bit
    res1, _ = _run(pkg, ctx, flipped, aligns=np.ones(n, np.int32), sp=pkg.symm_params(align_normals=0), **KW)
    plain, _ = _run(pkg, ctx, eight, **KW)
    for i, (r, q, pr) in enumerate(zip(res1, plain, eight)):
        assert _key(r) == _key(q)
        _check_record(r, pr.single(pkg, align=1, **KW), len(pr.src), i)
    # (void otherwise) the two settings give different matrices
    differ = sum(_bits(a.matrix()).tobytes() != _bits(b.matrix()).tobytes() for a, b in zip(res0, res1))
    print("align 0 and 1 differ for %d of %d pairs" % (differ, n))
    assert differ >= 6


# ---- test 6: NN engines and tuning knobs ----
def test_engines_and_knobs_bit_identical(pkg, ctx, eight):
    base, _ = _run(pkg, ctx, eight, **KW)
    for i, (r, pr) in enumerate(zip(base, eight)):
        _check_record(r, pr.single(pkg, **KW), len(pr.src), i)
    for more in (dict(nn_mode=pkg.NN_BRUTE), dict(nn_mode=pkg.NN_GRID), dict(nn_mode=pkg.NN_AUTO),
                 dict(nn_mode=pkg.NN_BRUTE, nn_sources_per_thread=1, nn_target_splits=3),
                 dict(nn_mode=pkg.NN_BRUTE, nn_sources_per_thread=8, nn_target_splits=1)):
        res, _ = _run(pkg, ctx, eight, **dict(KW, **more))
        _check_same(eight, res, base)


# ---- test 7: computed normals ----
def test_computed_normals_equal_given(pkg, ctx, eight):
    pairs = eight[:4]
    base, _ = _run(pkg, ctx, pairs, **KW)
    for sn, tn in ((False, True), (True, False), (False, False)):
        res, _ = _run(pkg, ctx, pairs, sn=sn, tn=tn, **KW)
        _check_same(pairs, res, base)
        assert [_f64_bits(r.fitness) for r in res] == [_f64_bits(r.fitness) for r in base]
    # normals_k is read where a set is computed
    at12 = [Pair(ctx, p.src, p.tgt, _normals(ctx, p.src, 12), _normals(ctx, p.tgt, 12)) for p in pairs]
    given, _ = _run(pkg, ctx, at12, **KW)
    computed, _ = _run(pkg, ctx, pairs, sn=False, tn=False, sp=pkg.symm_params(normals_k=12), **KW)
    _check_same(pairs, computed, given)
    assert [_key(r) for r in given] != [_key(r) for r in base]


# ---- test 8: endings ----
def test_endings_do_not_leak(pkg, ctx, eight):
    """max_iterations = 6: the restatement gives the pair at 0.5 degrees 3 passes and the pair at 60 degrees 10"""
    kw = dict(max_iterations=6)
    early = _halves(pkg, ctx, 31, 1500, 0.5)
    src, tgt, _, _ = S.halves_pair(pkg.synth, 32, 2000, 5.0)
    away = Pair(ctx, src + F32(100.0), tgt)
    src, tgt, _, _ = S.halves_pair(pkg.synth, 33, 1500, 7.0, n_src=1200)
    blind = Pair(ctx, src, tgt, sn=np.full((len(src), 3), np.nan, F32))
    slow = _halves(pkg, ctx, 34, 1500, 60.0, n_src=1300)
    healthy = [eight[1], early, eight[4], slow, eight[6]]
    pairs = [eight[1], away, early, eight[4], blind, slow, eight[6]]
    failing = (1, 4)
    res, _ = _run(pkg, ctx, pairs, **kw)
    print("passes", [r.iterations for r in res], "states", [r.state for r in res])
    for i, (r, pr) in enumerate(zip(res, pairs)):
        _check_record(r, pr.single(pkg, **kw), len(pr.src), i)
    for i in failing:
        assert res[i].state == 5 and res[i].iterations == 0 and not res[i].converged
        assert np.array_equal(res[i].matrix(), np.eye(4, dtype=F32))
    assert res[2].converged and res[2].iterations == 3
    assert res[5].iterations == 6 and res[5].state == 1      # (PCL's criteria count the iteration limit as converged)
    assert slow.single(pkg, max_iterations=100)["iterations"] > 6
    alone, _ = _run(pkg, ctx, healthy, **kw)
    _check_same(healthy, [r for i, r in enumerate(res) if i not in failing], alone)


# ---- test 9: the host pool does the solves from 64 pairs up ----
def test_host_pool_path(pkg, ctx):
    """the restatement gives all 66 pairs 3 passes or more"""
    rng = np.random.default_rng(66)
    pairs = []
    for i in range(66):
        n = int(rng.integers(500, 901))
        pairs.append(_halves(pkg, ctx, 100 + i, n, float(rng.uniform(3.0, 14.0)), n_src=int(rng.integers(500, n + 1))))
    res, extra = _run(pkg, ctx, pairs, trace=True, **KW)
    assert len(res) == 66
    for i, (r, pr) in enumerate(zip(res, pairs)):
        _check_record(r, pr.single(pkg, **KW), len(pr.src), i)
    _check_trace(extra, pairs[0].single(pkg, **KW))
    assert sum(r.iterations >= 2 for r in res) >= 60


# ---- test 10: device pointers ----
def test_dev_matches_host(pkg, ctx, flipped):
    import torch
    pairs = flipped[2:6]
    s, so, sn, t, to, tn = _pack(pairs)
    ds, dsn, dt, dtn = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (s, sn, t, tn))
    torch.cuda.synchronize()
    aligns = np.array([1, 0, 0, 1], np.int32)
    host, hextra = _run(pkg, ctx, pairs, aligns=aligns, trace=True, **KW)
    for i, (r, pr) in enumerate(zip(host, pairs)):
        _check_record(r, pr.single(pkg, align=int(aligns[i]), **KW), len(pr.src), i)
    # computed source normals carry no flips: at align 0 they give other records, so each combination has its own host run
    for has_s, has_t in ((True, True), (False, True), (True, False), (False, False)):
        want, wextra = (host, hextra) if has_s and has_t else _run(pkg, ctx, pairs, aligns=aligns, sn=has_s, tn=has_t, trace=True, **KW)
        dev, dextra = ctx.icp_symm_batch_dev(ds.data_ptr(), so, dsn.data_ptr() if has_s else None, dt.data_ptr(), to,
                                             dtn.data_ptr() if has_t else None, params=ctx.icp_params(**KW), aligns=aligns, trace_cap=64)
        assert [r.pair_id for r in dev] == list(range(len(pairs)))
        assert [_key(r) for r in dev] == [_key(r) for r in want]
        assert [_f64_bits(r.fitness) for r in dev] == [_f64_bits(r.fitness) for r in want]
        _check_trace(dextra, wextra)
    # a sub-range of the device arrays
    dev, _ = ctx.icp_symm_batch_dev(ds.data_ptr(), so[1:], dsn.data_ptr(), dt.data_ptr(), to[1:], dtn.data_ptr(), params=ctx.icp_params(**KW),
                                    aligns=aligns[1:])
    assert [_key(r) for r in dev] == [_key(r) for r in host[1:]]


# ---- test 11: a batch of one ----
def test_one_pair_is_the_single_call(pkg, ctx, eight):
    for pr in (eight[3], eight[0]):
        res, extra = _run(pkg, ctx, [pr], trace=True, **KW)
        single = pr.single(pkg, **KW)
        assert len(res) == 1 and single["iterations"] >= 2
        _check_record(res[0], single, len(pr.src), 0)
        _check_trace(extra, single)


# ---- test 12: the independent restatement ----
def test_pair_in_a_batch_matches_restatement(pkg, ctx, O, eight):
    """test_icp_symm_matches_restatement's first pair and tolerances, inside a batch of three"""
    pr = _halves(pkg, ctx, 1, 3000, 5.0)
    res, extra = _run(pkg, ctx, [pr, eight[2], eight[5]], trace=True, max_iterations=60)
    got = res[0]
    ref = S.icp_symm(O, pr.src, pr.sn, pr.tgt, pr.tn, max_iterations=60)
    print("|trace_Tk| %.2e  |T| %.2e  |fitness| %.2e" % (np.abs(extra["trace_Tk"] - ref["trace_Tk"]).max(),
                                                         np.abs(got.matrix() - ref["T"]).max(), abs(got.fitness - ref["fitness"])))
    assert got.iterations == ref["iterations"] >= 1
    assert got.state == ref["state"] and bool(got.converged) == ref["converged"]
    assert np.abs(extra["trace_Tk"] - ref["trace_Tk"]).max() <= 1e-6
    assert np.abs(got.matrix() - ref["T"]).max() <= 5e-6
    assert abs(got.fitness - ref["fitness"]) <= 1e-9 * max(1.0, ref["fitness"])
    eR, et = S.errors(got.matrix(), *pr.truth)
    print("|R - R_true| %.2e, |t - t_true| %.2e" % (eR, et))
    assert eR <= 1e-3 and et <= 1e-3


# ---- test 13: bad arguments ----
def test_bad_arguments(pkg, ctx, eight):
    pairs = eight[:2]
    s, so, sn, t, to, tn = _pack(pairs)

    def refused(call):
        with pytest.raises(pkg.KssError) as e:
            call()
        assert e.value.status == -1

    for bad in (2, -1):
        refused(lambda: ctx.icp_symm_batch(s, so, t, to, sn, tn, aligns=np.array([1, bad])))
        refused(lambda: ctx.icp_symm_batch(s, so, t, to, sn, tn, aligns=np.array([bad, 0])))
    refused(lambda: ctx.icp_symm_batch(s, so, t, to, sn, tn, sp=pkg.symm_params(align_normals=2)))
    p = ctx.icp_params()
    p.allreduce = pkg.binding.ALLREDUCE_FN(lambda user, values, n: 0)
    refused(lambda: ctx.icp_symm_batch(s, so, t, to, sn, tn, params=p))
    refused(lambda: ctx.icp_symm_batch(s, np.array([0, so[1], so[1]]), t, to, sn, tn))          # an empty pair
    refused(lambda: ctx.icp_symm_batch(s, so, t, np.array([0, 0, to[2]]), sn, tn))
    for k in (2, 65):                                      # normals_k is checked where a set of normals has to be computed
        refused(lambda: ctx.icp_symm_batch(s, so, t, to, None, tn, sp=pkg.symm_params(normals_k=k)))
        refused(lambda: ctx.icp_symm_batch(s, so, t, to, sn, None, sp=pkg.symm_params(normals_k=k)))
        ctx.icp_symm_batch(s, so, t, to, sn, tn, sp=pkg.symm_params(normals_k=k), params=ctx.icp_params(max_iterations=2))
    # the context still works, and gives what it gave
    res, _ = _run(pkg, ctx, pairs, **KW)
    for i, (r, pr) in enumerate(zip(res, pairs)):
        _check_record(r, pr.single(pkg, **KW), len(pr.src), i)
