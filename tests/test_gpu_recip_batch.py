"""Reciprocal ICP for many pairs per call (kss_recip_filter_batch[_dev], kss_icp_recip_pairs[_dev]): every segment of
the batched filter equals the single call on it and the restatement in tests/recip_ref.py, bit for bit, on maps that exercise every
path of the reverse search; pairs of one batch do not see each other's sources; every pair's record of the batched loop is the
single-pair call's bit for bit -- in any order, split over calls, through offsets that do not start at 0, under both NN engines and
either nn_fma -- with the anchor to kss_icp_o2o_batch, a pair that ends early beside pairs that go on, the pair above the row cap
and the argument errors."""

import numpy as np
import pytest

import recip_ref as RR

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
METRICS = [RR.POINT, RR.PLANE]
QNAN = 0x7FC00000


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
SIZES = [1, 64, 65, 257, 4096, 300]
MAX_D2 = 1e12


def _segments(O):
    """One (src, tgt, idx int32, d2 float32) per entry of SIZES, each with its own target:
    0  nt = 1;
    1  every source at one point: one cell holds them all, the one-add-per-wave path;
    2  a planar target (an axis with one cell), d2 replaced by -0.0f, +0.0f, denormals and the true value in turn, one NaN row;
    3  a random map that is not the NN map: large balls, the escape;
    4  the exact map with 200 sources on one spot: a row of more than 128 sources, the wave hand-over;
    5  sources far outside the target's box, and three source rows that are not finite (their d2 a NaN: not binned, no candidate)."""
    rng = np.random.default_rng(2028)
    u = lambda n: rng.uniform(-1, 1, (n, 3)).astype(F32)
    out = []
    src, tgt = u(1), np.array([[0.1, 0.2, -0.3]], F32)
    out.append((src, tgt) + tuple(O.nn_brute(src, tgt)))
    src, tgt = np.tile(np.array([[0.3, -0.2, 0.1]], F32), (64, 1)), u(48)
    out.append((src, tgt) + tuple(O.nn_brute(src, tgt)))
    src, tgt = u(65), u(40)
    src[:, 2] = 0.0
    tgt[:, 2] = 0.0
    idx, d2 = O.nn_brute(src, tgt)
    pick = rng.integers(0, 4, 65)
    den = rng.integers(1, 0x800000, 65).astype(np.uint32).view(F32)
    d2 = np.where(pick == 0, F32(-0.0), np.where(pick == 1, F32(0.0), np.where(pick == 2, den, d2))).astype(F32)
    d2[32] = np.nan
    out.append((src, tgt, idx, d2))
    src, tgt = u(257), u(190)
    idx = rng.integers(0, 190, 257).astype(np.int32)
    out.append((src, tgt, idx, RR.dist2(src, tgt[idx])))
    src, tgt = u(4096), u(3000)
    src[1000:1200] = src[1000]
    out.append((src, tgt) + tuple(O.nn_brute(src, tgt)))
    tgt = u(220)
    src = (rng.uniform(-1, 1, (300, 3)) * np.array([40.0, 3.0, 1.0]) + np.array([60.0, -20.0, 0.0])).astype(F32)
    src[::3] = u(100)
    idx, d2 = O.nn_brute(src, tgt)
    src[10] = np.nan
    src[20, 1] = np.inf
    src[30, 2] = -np.inf
    d2[[10, 20, 30]] = np.nan
    out.append((src, tgt, idx, d2))
    assert [len(s[0]) for s in out] == SIZES
    return out


def _pack_segments(segs, order, pad_s=0, pad_t=0):
    so = (pad_s + np.concatenate([[0], np.cumsum([len(segs[s][0]) for s in order])])).astype(np.int64)
    to = (pad_t + np.concatenate([[0], np.cumsum([len(segs[s][1]) for s in order])])).astype(np.int64)
    z3 = lambda n: [np.full((n, 3), 9.0, F32)] if n else []
    src = np.concatenate(z3(pad_s) + [segs[s][0] for s in order] + z3(pad_s))
    tgt = np.concatenate(z3(pad_t) + [segs[s][1] for s in order] + z3(pad_t))
    idx = np.concatenate([np.full(pad_s, 3, np.int32)] + [segs[s][2] for s in order] + [np.full(pad_s, 3, np.int32)])
    d2 = np.concatenate([np.full(pad_s, 0.5, F32)] + [segs[s][3] for s in order] + [np.full(pad_s, 0.5, F32)])
    return src, so, tgt, to, idx, d2


@pytest.fixture(scope="module")
def segments(O):
    segs = _segments(O)
    with np.errstate(invalid="ignore", over="ignore"):
        refs = [RR.filter_direct(s, t, i, d, MAX_D2) for s, t, i, d in segs]
    return segs, refs


def _check_segments(got_i, got_d, info, so, order, want):
    for q, s in enumerate(order):
        wi, wd, m, u, r = want[s]
        seg = slice(int(so[q]), int(so[q + 1]))
        assert (int(info[q, 0]), int(info[q, 1]), int(info[q, 2])) == (m, u, r), s
        assert np.array_equal(got_i[seg], wi), s
        assert np.array_equal(_bits(got_d[seg]), _bits(wd)), s


def test_filter_batch_equals_single_calls_and_the_restatement(ctx, segments):
    import torch
    segs, refs = segments
    singles = [ctx.recip_filter(s, t, i, d, MAX_D2) for s, t, i, d in segs]
    for s, (one, ref) in enumerate(zip(singles, refs)):
        print("segment %d (%d x %d): m %d u %d r %d (restatement %d %d %d)" % ((s, len(segs[s][0]), len(segs[s][1])) + one[2:] + ref[2:]))
        assert one[2:] == ref[2:] and np.array_equal(one[0], ref[0]) and np.array_equal(_bits(one[1]), _bits(ref[1])), s
    assert refs[1][2:] == (64, 1, 1)                                   # one point: the lowest index survives
    assert refs[3][4] < refs[3][3]                                     # the check is live on the large balls
    assert refs[4][4] >= 1 and refs[0][2:] == (1, 1, 1)
    order = list(range(len(SIZES)))
    # as packed, through offsets that do not start at 0, with rows in front and behind that nobody owns
    pad_s, pad_t = 5, 7
    src, so, tgt, to, idx, d2 = _pack_segments(segs, order, pad_s, pad_t)
    got_i, got_d, info = ctx.recip_filter_batch(src, so, tgt, to, idx, d2, MAX_D2)
    _check_segments(got_i, got_d, info, so, order, refs)
    assert np.array_equal(got_i[:pad_s], idx[:pad_s]) and np.array_equal(got_i[-pad_s:], idx[-pad_s:])
    assert np.array_equal(_bits(got_d[:pad_s]), _bits(d2[:pad_s])) and np.array_equal(_bits(got_d[-pad_s:]), _bits(d2[-pad_s:]))
    # the device form on separate outputs: the rows nobody owns come back untouched, the inputs are read only; then on its own inputs
    ds, dt, di, dd = (torch.from_numpy(x).cuda() for x in (src, tgt, idx, d2))
    oi, od = torch.full_like(di, -77), torch.full_like(dd, -77.0)
    torch.cuda.synchronize()
    args = (ds.data_ptr(), so, dt.data_ptr(), to, di.data_ptr(), dd.data_ptr(), MAX_D2, 0)
    info_d = ctx.recip_filter_batch_dev(*args, oi.data_ptr(), od.data_ptr())
    assert np.array_equal(info_d, info)
    assert np.array_equal(di.cpu().numpy(), idx) and np.array_equal(_bits(dd.cpu().numpy()), _bits(d2))
    hi, hd = oi.cpu().numpy(), od.cpu().numpy()
    _check_segments(hi, hd, info_d, so, order, refs)
    assert np.all(hi[:pad_s] == -77) and np.all(hi[-pad_s:] == -77) and np.all(hd[:pad_s] == -77.0) and np.all(hd[-pad_s:] == -77.0)
    assert np.array_equal(ctx.recip_filter_batch_dev(*args, di.data_ptr(), dd.data_ptr()), info)
    _check_segments(di.cpu().numpy(), dd.cpu().numpy(), info, so, order, refs)
    assert np.array_equal(di.cpu().numpy()[:pad_s], idx[:pad_s]) and np.array_equal(di.cpu().numpy()[-pad_s:], idx[-pad_s:])
    # any order of the segments gives every segment the same answer
    order = [4, 0, 3, 5, 1, 2]
    src, so, tgt, to, idx, d2 = _pack_segments(segs, order)
    got_i, got_d, info = ctx.recip_filter_batch(src, so, tgt, to, idx, d2, MAX_D2)
    _check_segments(got_i, got_d, info, so, order, refs)
    # the reverse distances by the fma form: against the single calls at nn_fma = 1
    fma = [ctx.recip_filter(s, t, i, d, MAX_D2, nn_fma=1) for s, t, i, d in segs]
    got_i, got_d, info = ctx.recip_filter_batch(src, so, tgt, to, idx, d2, MAX_D2, nn_fma=1)
    _check_segments(got_i, got_d, info, so, order, fma)


def test_pairs_of_a_batch_do_not_see_each_other(ctx, O):
    """Two segments on the SAME 257 targets T: A's sources are T itself, B's are T + N(0, 1e-2).  Alone, B has {m, u, r} = {257, 255,
    254}; could B's winners see A's sources (each at distance 0 from its target), none of them would stay mutual."""
    rng = np.random.default_rng(5)
    T = rng.uniform(0, 1, (257, 3)).astype(F32)
    A = T.copy()
    B = (T + rng.normal(0, 1e-2, (257, 3))).astype(F32)
    ia, da = O.nn_brute(A, T)
    ib, db = O.nn_brute(B, T)
    alone = RR.filter_direct(B, T, ib, db, 4.0)
    assert alone[2:] == (257, 255, 254)
    seen = RR.filter_direct(np.concatenate([A, B]), T, np.concatenate([ia, ib]), np.concatenate([da, db]), 4.0)
    assert not np.any(seen[0][257:] >= 0)                              # with A's sources visible no row of B stays mutual
    one = ctx.recip_filter(B, T, ib, db, 4.0)
    assert one[2:] == alone[2:] and np.array_equal(one[0], alone[0]) and np.array_equal(_bits(one[1]), _bits(alone[1]))
    off = np.array([0, 257, 514], np.int64)
    for b_at in (1, 0):
        parts = [(A, ia, da), (B, ib, db)] if b_at == 1 else [(B, ib, db), (A, ia, da)]
        got_i, got_d, info = ctx.recip_filter_batch(np.concatenate([p[0] for p in parts]), off, np.concatenate([T, T]), off,
                                                    np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts]), 4.0)
        seg = slice(257 * b_at, 257 * (b_at + 1))
        assert tuple(int(x) for x in info[b_at]) == alone[2:] and info[b_at, 2] >= 200
        assert np.array_equal(got_i[seg], alone[0]) and np.array_equal(_bits(got_d[seg]), _bits(alone[1]))
        assert tuple(int(x) for x in info[1 - b_at]) == (257, 257, 257)


@pytest.mark.parametrize("s", [0, 1, 2, 3], ids=["n%d" % n for n in SIZES[:4]])
def test_one_segment_through_the_batch_entry(ctx, segments, s):
    """nseg = 1 at n = 1, 64, 65, 257 through offsets that do not start at 0, with rows in front and behind that nobody owns: the
    restatement is the witness (the single call runs the same kernels), and the padding comes back untouched."""
    segs, refs = segments
    assert len(segs[s][0]) == SIZES[s]
    pad_s, pad_t = 5, 7
    src, so, tgt, to, idx, d2 = _pack_segments(segs, [s], pad_s, pad_t)
    assert so[0] == pad_s and to[0] == pad_t and len(so) == 2
    got_i, got_d, info = ctx.recip_filter_batch(src, so, tgt, to, idx, d2, MAX_D2)
    assert info.shape == (1, 3)
    _check_segments(got_i, got_d, info, so, [s], refs)
    for part in (slice(0, pad_s), slice(len(idx) - pad_s, len(idx))):
        assert np.array_equal(got_i[part], idx[part]) and np.array_equal(_bits(got_d[part]), _bits(d2[part]))


# ---- above the row cap, the filter alone ----
CAP_N = 2048 * 256 + 257


@pytest.fixture(scope="module")
def capped(O):
    """More sources than stream_blocks' 2048 rows of 256 hold: the grid-stride term of the walks and of the resolve is live.  128
    targets -- 64 random points and a twin of each at distance 1.7e-3 -- tiled CAP_N / 128 times plus N(0, 0.05) jitter: every target
    has thousands of candidates and one winner, and of two twins the winner of the one is often nearer to the other than that one's
    own winner, which then is not mutual.  The restatement visits 128 x CAP_N pairs: about three seconds, computed once."""
    rng = np.random.default_rng(2029)
    half = rng.uniform(-1, 1, (64, 3)).astype(F32)
    tgt = np.concatenate([half, half + F32(1e-3)]).astype(F32)
    src = (np.tile(tgt, (CAP_N // 128 + 1, 1))[:CAP_N] + rng.normal(0, 0.05, (CAP_N, 3))).astype(F32)
    idx, d2 = O.nn_brute(src, tgt)
    ref = RR.filter_direct(src, tgt, idx, d2, 4.0, chunk=16)
    return (src, tgt, idx, d2), ref


def test_filter_above_the_row_cap(ctx, capped):
    (src, tgt, idx, d2), ref = capped
    m, u, r = ref[2:]
    print("above the row cap: m %d u %d r %d" % (m, u, r))
    assert m == CAP_N and u == 128 and 1 <= r < u              # winners and mutual winners both exist and differ
    one = ctx.recip_filter(src, tgt, idx, d2, 4.0)
    assert one[2:] == ref[2:] and np.array_equal(one[0], ref[0]) and np.array_equal(_bits(one[1]), _bits(ref[1]))
    # as the second of two segments: its rows start behind the small segment's
    rng = np.random.default_rng(7)
    s_src, s_tgt = rng.uniform(-1, 1, (300, 3)).astype(F32), rng.uniform(-1, 1, (220, 3)).astype(F32)
    s_idx = rng.integers(0, 220, 300).astype(np.int32)
    small = (s_src, s_tgt, s_idx, RR.dist2(s_src, s_tgt[s_idx]))
    s_ref = RR.filter_direct(*small, 4.0)
    segs = [small, (src, tgt, idx, d2)]
    p_src, so, p_tgt, to, p_idx, p_d2 = _pack_segments(segs, [0, 1])
    got_i, got_d, info = ctx.recip_filter_batch(p_src, so, p_tgt, to, p_idx, p_d2, 4.0)
    _check_segments(got_i, got_d, info, so, [0, 1], [s_ref, ref])


# ---- stale tables on a shared context ----
def _same_filter(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and np.array_equal(_bits(x) if x.dtype in (F32, F64) else x, _bits(y) if y.dtype in (F32, F64) else y)
        else:
            assert x == y


def _same_icp(a, b):
    assert a["iterations"] == b["iterations"] and a["state"] == b["state"] and a["converged"] == b["converged"]
    for k in ("T", "trace_Tk", "trace_sums"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    for k in ("trace_recip", "recip_info", "trace_o2o", "o2o_info"):
        if k in a:
            assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    assert _f64_bits(a["fitness"]) == _f64_bits(b["fitness"]) and _f64_bits(a["last_mse"]) == _f64_bits(b["last_mse"])


def _same_batch(a, b):
    for x, y in zip(a[0], b[0]):
        assert x.iterations == y.iterations and x.state == y.state and x.pair_id == y.pair_id
        assert np.array_equal(_bits(x.matrix()), _bits(y.matrix()))
        assert _f64_bits(x.fitness) == _f64_bits(y.fitness) and _f64_bits(x.last_mse) == _f64_bits(y.last_mse)
    assert np.array_equal(_bits(a[1]), _bits(b[1]))
    assert np.array_equal(_bits(a[2]["trace_recip"]), _bits(b[2]["trace_recip"]))


def test_stale_tables_on_a_shared_context(pkg, ctx, segments):
    """The single pair reads the staged descriptor, the staged grids and the cell total that the batch also writes, and one-to-one
    shares the descriptors and the claim table's buffer: eight calls in a row on ONE context, each of which must give what it gives
    on a context that has run nothing before it -- and, for the filters, what the restatement gives."""
    segs, refs = segments
    rng = np.random.default_rng(11)
    o_idx, o_d2 = rng.integers(0, 190, 300).astype(np.int32), rng.uniform(0, 1, 300).astype(F32)
    a_src, a_tgt = _bumpy(pkg, 71, 1500, 6.0, n_src=900)
    b_src, b_tgt = _bumpy(pkg, 72, 700, 8.0, n_src=333)
    so, to = np.array([0, 900, 1233], np.int64), np.array([0, 1500, 2200], np.int64)
    p3 = lambda c: c.icp_params(max_iterations=3, fixed_iterations=1)
    order_a, order_b = list(range(len(SIZES))), [4, 0, 3, 5, 1, 2]
    pack_a, pack_b = _pack_segments(segs, order_a), _pack_segments(segs, order_b)
    calls = [
        ("filter_batch", lambda c: c.recip_filter_batch(*pack_a, MAX_D2)),
        ("filter", lambda c: c.recip_filter(*segs[3], MAX_D2)),
        ("o2o_filter", lambda c: c.o2o_filter(o_idx, o_d2, 190, 1.0)),
        ("icp", lambda c: c.icp_recip(a_src, a_tgt, None, overlap=0.9, metric=RR.POINT, params=p3(c), trace_cap=8)),
        ("icp", lambda c: c.icp_o2o(a_src, a_tgt, None, overlap=0.9, metric=RR.POINT, params=p3(c), trace_cap=8)),
        ("batch", lambda c: c.icp_recip_batch(np.concatenate([a_src, b_src]), so, np.concatenate([a_tgt, b_tgt]), to, None,
                                              overlaps=np.array([0.9, 0.8]), metric=RR.POINT, params=p3(c), trace_cap=8)),
        ("filter", lambda c: c.recip_filter(*segs[2], MAX_D2)),
        ("filter_batch", lambda c: c.recip_filter_batch(*pack_b, MAX_D2)),
    ]
    shared = [fn(ctx) for _, fn in calls]
    for q, ((kind, fn), got) in enumerate(zip(calls, shared)):
        fresh_ctx = pkg.Context(0)
        try:
            want = fn(fresh_ctx)
        finally:
            fresh_ctx.close()
        if kind == "icp":
            assert want["iterations"] == 3
            _same_icp(got, want)
        elif kind == "batch":
            assert [r.iterations for r in want[0]] == [3, 3]
            _same_batch(got, want)
        else:
            _same_filter(got, want)
    # the filters against the restatement
    _check_segments(shared[0][0], shared[0][1], shared[0][2], pack_a[1], order_a, refs)
    _check_segments(shared[7][0], shared[7][1], shared[7][2], pack_b[1], order_b, refs)
    for got, s in ((shared[1], 3), (shared[6], 2)):
        assert got[2:] == refs[s][2:] and np.array_equal(got[0], refs[s][0]) and np.array_equal(_bits(got[1]), _bits(refs[s][1]))
    assert len(segs[3][0]) == 257 and len(segs[2][0]) == 65


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
            self._single[key] = self.ctx.icp_recip(self.src, self.tgt, self.nrm if metric == RR.PLANE else None, overlap=overlap,
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
    return ctx.icp_recip_batch(s, so, t, to, nr if metric == RR.PLANE else None, overlaps=overlaps, metric=metric,
                               params=ctx.icp_params(**kw), trace_cap=256 if trace else 0)


def _check_record(r, single, ns, pair_id, info):
    assert r.pair_id == pair_id
    assert r.iterations == single["iterations"] and r.state == single["state"] and bool(r.converged) == single["converged"]
    assert np.array_equal(_bits(r.matrix()), _bits(single["T"]))
    assert _f64_bits(r.last_mse) == _f64_bits(single["last_mse"])
    # test_gpu_trim.py's bound for two summation orders of the NN engines' f64 sum of d2 over all sources
    assert abs(r.fitness - single["fitness"]) <= 2.0 * ns * 2.0 ** -53 * single["fitness"]
    assert np.array_equal(_bits(info), _bits(single["recip_info"]))


OVERLAPS = [1.0, 0.9, 0.5, 1.0, 0.7]
# tests/recip_ref.py's icp_recip, point metric, on the five pairs (run on the CPU): iterations and pass 0's (r, u)
RESTATED = [(12, 574, 728), (26, 552, 862), (8, 57, 59), (9, 1315, 1513), (14, 231, 254)]


@pytest.fixture(scope="module")
def five(pkg, ctx):
    """Five pairs of 97 to 3000 points on which the reciprocal check rejects winners in pass 0: a fifth of the sources pushed off the
    surface, a partly overlapping pair with such outliers, a sparse source, and two pairs whose source is a part of the target."""
    S = pkg.synth
    out = [Pair(ctx, *S.make_outlier_pair(51, 1200, 10.0, 0.2)[:2])]
    src, tgt = S.make_partial_pair(52, 3600, 12.0, -0.2, 0.6)[:2]
    k = len(src) // 5                                                  # test_gpu_recip.py's _with_outliers(pkg, src, 52)
    u = np.stack([S.u01(9100 + 52, k, j * k) for j in range(3)], axis=1)
    moved = src.astype(F64)
    moved[:k] += (u - 0.5) * 1.2
    out.append(Pair(ctx, moved.astype(F32), tgt))
    src, tgt = S.make_partial_pair(53, 600, 8.0, -0.5, 0.3)[:2]
    out.append(Pair(ctx, src[::4], tgt))
    out.append(Pair(ctx, *_bumpy(pkg, 54, 3000, 6.0, n_src=2100)))
    out.append(Pair(ctx, *_bumpy(pkg, 55, 900, 9.0, n_src=300)))
    assert [len(p.src) for p in out] == [1200, 2804, 97, 2100, 300]
    return out


@pytest.mark.parametrize("nn_mode", ["brute", "grid"])
@pytest.mark.parametrize("metric", METRICS, ids=["point", "plane"])
def test_recip_batch_equals_single_calls(pkg, ctx, five, metric, nn_mode):
    mode = pkg.NN_BRUTE if nn_mode == "brute" else pkg.NN_GRID
    kw = dict(max_iterations=60, nn_mode=mode)
    ov = np.array(OVERLAPS, F64)
    singles = [p.single(metric, float(o), trace=True, max_iterations=60, nn_mode=pkg.NN_BRUTE) for p, o in zip(five, ov)]
    for s, (its, r0, u0) in zip(singles, RESTATED):
        t0 = s["trace_recip"][0]
        print("single: %d iterations, pass 0 r %d u %d m %d (restatement, point metric: %d iterations, r %d u %d)"
              % (s["iterations"], t0[0], t0[5], t0[4], its, r0, u0))
        assert s["iterations"] >= 2 and t0[0] < t0[5]                  # the check is live in every pair of the batch
        assert (t0[0], t0[5]) == (r0, u0)                              # pass 0 sees the same positions under either metric
    # as packed, with pair 0's traces
    res, info, extra = _run_batch(ctx, five, metric, ov, trace=True, **kw)
    for i, (r, p) in enumerate(zip(res, five)):
        _check_record(r, singles[i], len(p.src), i, info[i])
    assert np.array_equal(_bits(extra["trace_sums"]), _bits(singles[0]["trace_sums"]))
    assert np.array_equal(_bits(extra["trace_Tk"]), _bits(singles[0]["trace_Tk"]))
    assert np.array_equal(_bits(extra["trace_recip"]), _bits(singles[0]["trace_recip"]))
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
def test_recip_batch_dev_and_default_overlap(pkg, ctx, five, metric):
    import torch
    pairs = five[:3]
    s, so, t, to, nr = _pack(pairs)
    ds, dt, dn = (torch.from_numpy(x).cuda() for x in (s, t, nr))
    torch.cuda.synchronize()
    res, info = ctx.icp_recip_batch_dev(ds.data_ptr(), so, dt.data_ptr(), to, dn.data_ptr() if metric == RR.PLANE else None,
                                        ctx.icp_params(max_iterations=60), overlaps=None, overlap=0.9, metric=metric)
    for i, (r, p) in enumerate(zip(res, pairs)):
        _check_record(r, p.single(metric, 0.9, max_iterations=60), len(p.src), i, info[i])


def test_recip_batch_nn_fma(pkg, ctx, five):
    ov = np.array(OVERLAPS, F64)
    res, info, extra = _run_batch(ctx, five, RR.POINT, ov, trace=True, max_iterations=60, nn_fma=1)
    for i, (r, p) in enumerate(zip(res, five)):
        single = p.single(RR.POINT, float(ov[i]), trace=True, max_iterations=60, nn_fma=1)
        assert single["iterations"] >= 2
        _check_record(r, single, len(p.src), i, info[i])
    assert np.array_equal(_bits(extra["trace_recip"]), _bits(five[0].single(RR.POINT, 1.0, trace=True, max_iterations=60, nn_fma=1)["trace_recip"]))


def _lattice_pair(pkg):
    """tests/test_gpu_recip.py's scene: 1000 sources on a 40 x 40 lattice target, every source the nearest source of its nearest
    target in every pass."""
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


@pytest.mark.parametrize("metric", METRICS, ids=["point", "plane"])
def test_anchor_mutual_scene_is_icp_o2o_batch_bit_for_bit(pkg, ctx, metric):
    pair = Pair(ctx, *_lattice_pair(pkg))
    s, so, t, to, nr = _pack([pair] * 3)
    nr = nr if metric == RR.PLANE else None
    ov = np.array([1.0, 0.5, 0.8], F64)
    kw = dict(max_iterations=10, fixed_iterations=1)
    a_res, a_info, a_extra = ctx.icp_o2o_batch(s, so, t, to, nr, overlaps=ov, metric=metric, params=ctx.icp_params(**kw), trace_cap=16)
    b_res, b_info, b_extra = ctx.icp_recip_batch(s, so, t, to, nr, overlaps=ov, metric=metric, params=ctx.icp_params(**kw), trace_cap=16)
    tt = b_extra["trace_recip"]
    assert len(tt) == 10
    assert np.all(tt[:, 0] == 1000) and np.all(tt[:, 4] == 1000) and np.all(tt[:, 5] == 1000)      # r == u == m in every traced pass
    assert np.array_equal(_bits(a_extra["trace_o2o"]), _bits(tt[:, :5]))
    assert np.array_equal(_bits(a_extra["trace_sums"]), _bits(b_extra["trace_sums"]))
    for i, (a, b) in enumerate(zip(a_res, b_res)):
        assert a.iterations == b.iterations == 10 and a.state == b.state and a.pair_id == b.pair_id == i
        assert np.array_equal(_bits(a.matrix()), _bits(b.matrix()))
        assert _f64_bits(a.last_mse) == _f64_bits(b.last_mse)
        assert np.array_equal(_bits(a_info[i]), _bits(b_info[i, :5]))
        assert b_info[i, 0] == b_info[i, 5] == b_info[i, 4] == 1000


@pytest.mark.parametrize("metric", METRICS, ids=["point", "plane"])
def test_one_pair_ends_early_the_others_go_on(pkg, ctx, five, metric):
    far = Pair(ctx, five[4].src + np.float32(100.0), five[4].tgt)          # no candidate in its first pass
    pairs = [five[0], far, five[3]]
    ov = np.array([1.0, 1.0, 0.7], F64)
    res, info, _ = _run_batch(ctx, pairs, metric, ov, max_iterations=60)
    assert res[1].state == 5 and res[1].iterations == 0 and not res[1].converged
    assert np.array_equal(info[1], np.zeros(6)) and np.array_equal(res[1].matrix(), np.eye(4, dtype=F32))
    for i in (0, 2):
        single = pairs[i].single(metric, float(ov[i]), max_iterations=60)
        assert single["iterations"] >= 2
        _check_record(res[i], single, len(pairs[i].src), i, info[i])
    _check_record(res[1], far.single(metric, 1.0, max_iterations=60), len(far.src), 1, info[1])


def test_pair_above_the_row_cap(pkg, ctx):
    """stream_blocks saturates at 2048 rows: for a pair of more than 2048 * 256 sources the grid-stride term of the batched walks and
    of the batched resolve is live.  Two passes of the point metric against the single-pair calls."""
    src, tgt = _bumpy(pkg, 60, 524800, 5.0)
    big = Pair(ctx, src, tgt[::175])
    small = Pair(ctx, *_bumpy(pkg, 61, 2000, 7.0, n_src=300))
    assert len(big.src) == 524800 > 2048 * 256 and len(big.tgt) <= 3000 and len(small.src) == 300
    pairs = [small, big]
    ov = np.array([0.6, 0.8], F64)
    res, info, _ = _run_batch(ctx, pairs, RR.POINT, ov, max_iterations=2)
    for i, (r, pr) in enumerate(zip(res, pairs)):
        single = pr.single(RR.POINT, float(ov[i]), max_iterations=2)
        assert single["iterations"] == 2
        _check_record(r, single, len(pr.src), i, info[i])
    assert info[1, 0] <= info[1, 5] <= len(big.tgt) < info[1, 4] == len(big.src)


def test_batch_argument_errors(pkg, ctx, five, segments):
    import ctypes as C
    pairs = five[:2]
    s, so, t, to, nr = _pack(pairs)
    before = _run_batch(ctx, pairs, RR.POINT, None, max_iterations=5)
    for ov in (np.array([0.5, 0.0]), np.array([float("nan"), 1.0]), np.array([1.5, 1.0])):
        with pytest.raises(pkg.KssError) as e:
            ctx.icp_recip_batch(s, so, t, to, None, overlaps=ov, metric=RR.POINT)
        assert e.value.status == -1
    with pytest.raises(pkg.KssError) as e:
        ctx.icp_recip_batch(s, so, t, to, nr, metric=RR.POINT)                # the point metric takes no normals
    assert e.value.status == -1
    bad = so.copy(); bad[1] = bad[0]                                          # an empty pair
    with pytest.raises(pkg.KssError) as e:
        ctx.icp_recip_batch(s, bad, t, to, None, metric=RR.POINT)
    assert e.value.status == -1
    p = ctx.icp_params()
    p.allreduce = pkg.binding.ALLREDUCE_FN(lambda user, values, n: 0)
    with pytest.raises(pkg.KssError) as e:
        ctx.icp_recip_batch(s, so, t, to, None, metric=RR.POINT, params=p)
    assert e.value.status == -1
    L, q = ctx.L, ctx.icp_params()
    res = (pkg.IcpResult * 2)()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.kss_icp_recip_pairs(ctx.h, vp(s), vp(so), vp(t), vp(to), None, 2, C.byref(q), None, None, C.cast(res, C.c_void_p), None) == -1
    assert ctx.L.kss_last_error(ctx.h).decode().startswith("icp_recip_pairs: ")
    rp = pkg.recip_params()
    assert L.kss_icp_recip_pairs(ctx.h, vp(s), vp(so), vp(t), vp(to), None, 0, C.byref(q), C.byref(rp), None, C.cast(res, C.c_void_p), None) == -1
    assert L.kss_icp_recip_pairs(ctx.h, vp(s), vp(so), vp(t), vp(to), None, 2, C.byref(q), C.byref(rp), None, None, None) == -1
    # the filter: an empty segment, a segment without targets, no segment, a NULL array
    segs = segments[0]
    fs, fso, ft, fto, fi, fd = _pack_segments(segs, [1, 2])
    for which in ("src", "tgt"):
        o1, o2 = fso.copy(), fto.copy()
        (o1 if which == "src" else o2)[1] = 0
        with pytest.raises(pkg.KssError) as e:
            ctx.recip_filter_batch(fs, o1, ft, o2, fi, fd, MAX_D2)
        assert e.value.status == -1 and ctx.L.kss_last_error(ctx.h).decode().startswith("recip_filter_batch: ")
    info = np.zeros(6)
    assert L.kss_recip_filter_batch(ctx.h, vp(fs), vp(fso), vp(ft), vp(fto), 0, vp(fi), vp(fd), MAX_D2, 0, None, None, vp(info)) == -1
    assert L.kss_recip_filter_batch(ctx.h, vp(fs), vp(fso), vp(ft), vp(fto), 2, None, vp(fd), MAX_D2, 0, None, None, vp(info)) == -1
    assert L.kss_recip_filter_batch(ctx.h, vp(fs), vp(fso), vp(ft), vp(fto), 2, vp(fi), vp(fd), MAX_D2, 0, None, None, None) == -1
    # the context is as it was
    after = _run_batch(ctx, pairs, RR.POINT, None, max_iterations=5)
    for a, b in zip(before[0], after[0]):
        assert np.array_equal(_bits(a.matrix()), _bits(b.matrix())) and _f64_bits(a.fitness) == _f64_bits(b.fitness)
    assert np.array_equal(_bits(before[1]), _bits(after[1]))
