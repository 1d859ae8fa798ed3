"""Batched voxelized generalized ICP on the device (kss_icp_vgicp_batch[_dev]).  The yardstick everywhere is
Context.icp_vgicp -- the single-scan call, code the batch does not touch -- on the same scan and the same map: every scan of a batch
has to come back with that call's bits, in any order, any split over calls, beside scans that end early, with non-finite input
next to it, and whatever the context's workspace held before.
One target serves every scan: vgicp_ref.halves_pair(synth, 8, 4000, deg, axis=[0.3, -0.5, 1], n_src=...) gives the same target for
every deg; its map is at leaf 0.1 with given normals."""
import ctypes as C

import numpy as np
import pytest

import vgicp_ref as V

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
AXIS = [0.3, -0.5, 1.0]
WRAP = 2048 * 256 + 300   # the first source count at which the rows kernel's grid-stride walk wraps (test_gpu_pair_bits.py)
# (deg, n_src): 1, 3, 255 and 257 sit around one workgroup of 256, 1000 and 4000 span several rows
RAGGED = [(10, 4000), (25, 1000), (40, 257), (5, 255), (2, 3), (10, 1), (25, 4000), (40, 4000)]
KEYS = ("T", "iterations", "state", "converged", "last_mse", "fitness", "info")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)


def _same(got, want, what=""):
    """Every field of the single call's record, in bits (NaN equals NaN)."""
    for k in KEYS:
        if k in ("iterations", "state", "converged"):
            assert got[k] == want[k], (what, k, got[k], want[k])
        else:
            a, b = (np.atleast_1d(np.asarray(x[k], dtype=F32 if k == "T" else F64)) for x in (got, want))
            assert np.array_equal(_bits(a), _bits(b)), (what, k, got[k], want[k])


def _pack(scans):
    off = np.zeros(len(scans) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s, _ in scans])
    return np.concatenate([s for s, _ in scans]), off, np.concatenate([n for _, n in scans])


def _batch(ctx, m, scans, **kw):
    src_all, off, sn_all = _pack(scans)
    return ctx.icp_vgicp_batch(src_all, off, m, src_normals_all=sn_all, **kw)


class Scene:
    pass


@pytest.fixture(scope="module")
def scene(pkg, ctx):
    """The target's map, the ragged scans with their normals and the single call's result for each, computed once."""
    sc = Scene()
    sc.scans = []
    for k, (deg, n) in enumerate(RAGGED):
        src, tgt, _, _ = V.halves_pair(pkg.synth, 8, 4000, float(deg), axis=AXIS, n_src=n)
        sn = ctx.normals(src.astype(F64), min(20, n)).astype(F32) if n >= 255 else _unit(np.random.default_rng(100 + k), n)
        sc.scans.append((src, sn))
    far = V.halves_pair(pkg.synth, 8, 4000, 10.0, axis=AXIS, n_src=300)[0] + np.array([50.0, 0.0, 0.0], F32)
    sc.scans.append((far.astype(F32), ctx.normals(far.astype(F64), 20).astype(F32)))
    sc.tgt = tgt
    sc.tn = ctx.normals(tgt.astype(F64), 20).astype(F32)
    sc.map = ctx.vmap(sc.tgt, 0.1, normals=sc.tn)
    sc.single = [ctx.icp_vgicp(s, sc.map, n, trace_cap=64) for s, n in sc.scans]
    yield sc
    sc.map.close()


def test_ragged_batch_bit_for_bit(ctx, scene):
    one = scene.single
    print("single calls: passes %s states %s" % ([r["iterations"] for r in one], [r["state"] for r in one]))
    # the input is fair: the scans end after different pass counts, some without correspondences (a condition on the yardstick)
    assert len({r["iterations"] for r in one}) >= 4
    assert sum(r["state"] == 5 for r in one) >= 1
    assert np.isnan(one[-1]["fitness"]) and one[-1]["iterations"] == 0
    got = _batch(ctx, scene.map, scene.scans, trace_cap=64)
    assert len(got) == len(one)
    for i, (g, w) in enumerate(zip(got, one)):
        _same(g, w, i)
        assert g["pair_id"] == i
        assert g["info"][1] == len(scene.scans[i][0])
    for k in ("trace_sums", "trace_Tk"):
        assert np.array_equal(_bits(got[0][k]), _bits(one[0][k])), k
        assert all(k not in g for g in got[1:])


def test_order_and_split(ctx, scene):
    scans, one, m = scene.scans, scene.single, scene.map
    n = len(scans)
    for g, w in zip(_batch(ctx, m, scans[::-1]), one[::-1]):
        _same(g, w, "reversed")
    got = _batch(ctx, m, scans[:4]) + _batch(ctx, m, scans[4:])
    assert [g["pair_id"] for g in got] == list(range(4)) + list(range(n - 4))
    for g, w in zip(got, one):
        _same(g, w, "split")
    # offsets whose first entry is not 0 into a longer packed array: scans 1 .. n - 2 of the full pack
    src_all, off, sn_all = _pack(scans)
    got = ctx.icp_vgicp_batch(src_all, off[1:-1], m, src_normals_all=sn_all)
    assert len(got) == n - 2
    for g, w in zip(got, one[1:-1]):
        _same(g, w, "sub-range")


def test_grid_stride_wrap(pkg, ctx, scene):
    """A scan of more than 2048 * 256 points -- the target's own points tiled and jittered, given normals -- behind a scan of 257."""
    rng = np.random.default_rng(9)
    big = (scene.tgt[np.arange(WRAP) % len(scene.tgt)] + rng.normal(scale=0.005, size=(WRAP, 3))).astype(F32)
    bn = _unit(rng, WRAP)
    p = ctx.icp_params(max_iterations=2)
    scans = [scene.scans[2], (big, bn)]
    assert len(scans[0][0]) == 257
    want = [ctx.icp_vgicp(s, scene.map, n, params=p) for s, n in scans]
    assert want[1]["iterations"] == 2 and want[1]["info"][0] > 0.5 * WRAP
    for g, w in zip(_batch(ctx, scene.map, scans, params=p), want):
        _same(g, w, "wrap")


def test_per_scan_epsilon(pkg, ctx, scene):
    eps = [1e-3, 1e-2, 1.0]
    s, n = scene.scans[0]
    want = [ctx.icp_vgicp(s, scene.map, n, gp=pkg.gicp_params(epsilon=e)) for e in eps]
    got = _batch(ctx, scene.map, [(s, n)] * 3, epsilons=eps)
    for g, w in zip(got, want):
        _same(g, w, "epsilon")
    assert not np.array_equal(_bits(got[0]["T"]), _bits(got[1]["T"]))
    # no per-scan array: gp.epsilon everywhere
    for g in _batch(ctx, scene.map, [(s, n)] * 2, gp=pkg.gicp_params(epsilon=1e-2)):
        _same(g, want[1], "gp.epsilon")


def test_non_finite_input_inside_a_batch(ctx, scene):
    rng = np.random.default_rng(3)
    s, n = scene.scans[1][0].copy(), scene.scans[1][1].copy()
    s[rng.random(len(s)) < 0.05, 1] = np.nan
    s[rng.random(len(s)) < 0.02, 0] = np.inf
    n[rng.random(len(n)) < 0.05] = np.nan
    s[0] = np.nan
    n[-1, 2] = -np.inf
    want = ctx.icp_vgicp(s, scene.map, n)
    assert want["iterations"] >= 1 and 0 < want["info"][0] < len(s)
    got = _batch(ctx, scene.map, [scene.scans[0], (s, n), scene.scans[2]])
    _same(got[0], scene.single[0], "left neighbour")
    _same(got[1], want, "non-finite scan")
    _same(got[2], scene.single[2], "right neighbour")


def test_computed_normals_and_dev_entry(ctx, scene):
    import torch
    idx = [i for i, (s, _) in enumerate(scene.scans) if len(s) >= 255]
    scans = [scene.scans[i] for i in idx]
    src_all, off, sn_all = _pack(scans)
    host = ctx.icp_vgicp_batch(src_all, off, scene.map, src_normals_all=None)
    for g, i in zip(host, idx):
        _same(g, scene.single[i], "computed normals")
    ds, dn = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (src_all, sn_all))
    torch.cuda.synchronize()
    for d_n in (dn.data_ptr(), None):
        res, info = ctx.icp_vgicp_batch_dev(ds.data_ptr(), off, d_n, scene.map, ctx.icp_params())
        assert info.shape == (len(scans), 4)
        for k, (r, h) in enumerate(zip(res, host)):
            assert (r.iterations, r.state, bool(r.converged), r.pair_id) == (h["iterations"], h["state"], h["converged"], k)
            assert np.array_equal(_bits(r.matrix()), _bits(h["T"]))
            assert np.array_equal(_bits(np.array([r.fitness, r.last_mse])), _bits(np.array([h["fitness"], h["last_mse"]])))
            assert np.array_equal(_bits(info[k]), _bits(h["info"]))


def test_deterministic_whatever_the_workspace_held(pkg, ctx, scene):
    lin0, st0 = scene.map.read()
    a = _batch(ctx, scene.map, scene.scans, trace_cap=64)
    b = _batch(ctx, scene.map, scene.scans, trace_cap=64)
    big_s, big_t = pkg.synth.make_pair(3, 60000, R=pkg.synth.rot_axis_angle([0, 0, 1], 0.1), shape="bumpy")
    assert ctx.icp(big_s, big_t, ctx.icp_params(max_iterations=3))["iterations"] == 3
    c = _batch(ctx, scene.map, scene.scans, trace_cap=64)
    for x, y, z in zip(a, b, c):
        _same(y, x, "again")
        _same(z, x, "after another call")
    for k in ("trace_sums", "trace_Tk"):
        assert np.array_equal(_bits(a[0][k]), _bits(b[0][k])) and np.array_equal(_bits(a[0][k]), _bits(c[0][k]))
    lin1, st1 = scene.map.read()
    assert np.array_equal(lin0, lin1) and np.array_equal(_bits(st0), _bits(st1))


def test_states(ctx, scene):
    """test_gpu_vgicp.py's test_vgicp_states in one batch: a scan wholly outside the box and a scan of NaNs (NO_CORRESPONDENCES), a
    scan of one point repeated with one normal (its normal equations have no spread: whatever state the single call gives it),
    beside a converging scan; then the same batch cut off by max_iterations (ITERATIONS)."""
    s, n = scene.scans[0]
    flat = (np.repeat(scene.tgt[:1], 64, axis=0).astype(F32), np.repeat(scene.tn[:1], 64, axis=0).astype(F32))
    scans = [(s + F32(100.0), n), (s, n), (np.full_like(s, np.nan), n), flat, scene.scans[3]]
    for kw in ({}, {"max_iterations": 2}):
        want = [ctx.icp_vgicp(a, scene.map, b, params=ctx.icp_params(**kw)) for a, b in scans]
        print("states %s passes %s" % ([w["state"] for w in want], [w["iterations"] for w in want]))
        assert want[0]["state"] == 5 and want[2]["state"] == 5 and np.isnan(want[0]["fitness"])
        if kw:
            assert want[1]["state"] == 1 and want[1]["iterations"] == 2
        else:
            assert want[1]["converged"] and want[1]["state"] in (2, 3, 4)
        for g, w in zip(_batch(ctx, scene.map, scans, params=ctx.icp_params(**kw)), want):
            _same(g, w, "states")


def test_fixed_iterations_no_fitness_no_passes(ctx, scene):
    idx = [0, 1, 2, 3, 6, 7]
    scans = [scene.scans[i] for i in idx]
    p = ctx.icp_params(fixed_iterations=1, max_iterations=5)
    got = _batch(ctx, scene.map, scans, params=p)
    assert [g["iterations"] for g in got] == [5] * len(scans)
    for g, (a, b) in zip(got, scans):
        _same(g, ctx.icp_vgicp(a, scene.map, b, params=p), "fixed iterations")
    p = ctx.icp_params(compute_fitness=0)
    got = _batch(ctx, scene.map, scene.scans, params=p)
    for g, (a, b) in zip(got, scene.scans):
        _same(g, ctx.icp_vgicp(a, scene.map, b, params=p), "no fitness")
        assert g["fitness"] == 0.0
    p = ctx.icp_params(max_iterations=0)
    got = _batch(ctx, scene.map, scene.scans, params=p)
    for g, (a, b) in zip(got, scene.scans):
        _same(g, ctx.icp_vgicp(a, scene.map, b, params=p), "no passes")
        assert g["iterations"] == 0 and np.array_equal(g["T"], np.eye(4, dtype=F32)) and g["info"][0] == 0.0


def test_bad_arguments(pkg, ctx, scene):
    """Every refusal is KSS_ERR_ARG and is followed by a good call whose bits are what they were."""
    m = scene.map
    scans = [scene.scans[2], scene.scans[3], scene.scans[4]]
    src_all, off, sn_all = _pack(scans)
    want = [scene.single[2], scene.single[3], scene.single[4]]
    L, B = ctx.L, pkg.binding
    count = [0]

    def good():
        for g, w in zip(ctx.icp_vgicp_batch(src_all, off, m, src_normals_all=sn_all), want):
            _same(g, w, "after refusal %d" % count[0])

    def refused(call):
        count[0] += 1
        with pytest.raises(pkg.KssError) as e:
            call()
        assert e.value.status == -1
        good()

    def raw(name="kss_icp_vgicp_batch", **kw):
        """The C entry with one argument replaced."""
        res = (B.IcpResult * 3)()
        info = np.zeros((3, 4), F64)
        a = dict(src=B._p(src_all), off=B._p(off), sn=B._p(sn_all), n=3, map=m.h, p=C.byref(ctx.icp_params()), gp=C.byref(pkg.gicp_params()),
                 eps=None, res=C.cast(res, C.c_void_p), info=B._p(info))
        a.update(kw)
        rc = getattr(L, name)(ctx.h, a["src"], a["off"], a["sn"], a["n"], a["map"], a["p"], a["gp"], a["eps"], a["res"], a["info"])
        return rc, list(res), info

    good()
    for k in ("src", "off", "p", "gp", "res"):
        refused(lambda: ctx._chk(raw(**{k: None})[0], "kss_icp_vgicp_batch"))
    for n in (0, -1):
        refused(lambda: ctx._chk(raw(n=n)[0], "kss_icp_vgicp_batch"))
    refused(lambda: ctx.icp_vgicp_batch(src_all, off[:1], m, src_normals_all=sn_all))                    # nscans = 0 through the binding
    refused(lambda: ctx.icp_vgicp_batch(src_all, [0, 257, 257, 515], m, src_normals_all=sn_all))        # an empty scan
    refused(lambda: ctx.icp_vgicp_batch(src_all, [0, 300, 257, 515], m, src_normals_all=sn_all))        # decreasing offsets
    refused(lambda: ctx.icp_vgicp_batch(src_all, off, None, src_normals_all=sn_all))                    # a NULL map
    other = pkg.Context(0)
    try:
        theirs = other.vmap(scene.tgt, 0.1, normals=scene.tn)
        refused(lambda: ctx.icp_vgicp_batch(src_all, off, theirs, src_normals_all=sn_all))              # a map of another context
        for g, w in zip(other.icp_vgicp_batch(src_all, off, theirs, src_normals_all=sn_all), want):
            _same(g, w, "on its own context")
        theirs.close()
    finally:
        other.close()
    gone = ctx.vmap(scene.tgt, 0.1, normals=scene.tn)
    gone.close()
    gone.h = C.c_void_p(0x1234560)                                                                       # a handle that is no live map
    refused(lambda: ctx.icp_vgicp_batch(src_all, off, gone, src_normals_all=sn_all))
    for eps in (0.0, -1.0, 2.0, float("nan")):
        refused(lambda: ctx.icp_vgicp_batch(src_all, off, m, src_normals_all=sn_all, gp=pkg.gicp_params(epsilon=eps)))
        refused(lambda: ctx.icp_vgicp_batch(src_all, off, m, src_normals_all=sn_all, epsilons=[1e-3, eps, 1e-3]))
    for k in (2, 65):
        refused(lambda: ctx.icp_vgicp_batch(src_all, off, m, gp=pkg.gicp_params(normals_k=k)))          # the normals are to be computed
    _same(ctx.icp_vgicp_batch(src_all, off, m, src_normals_all=sn_all, gp=pkg.gicp_params(normals_k=2))[0], want[0], "normals_k unread")
    p = ctx.icp_params()
    cb = B.ALLREDUCE_FN(lambda user, values, n: 0)
    p.allreduce = cb
    refused(lambda: ctx.icp_vgicp_batch(src_all, off, m, src_normals_all=sn_all, params=p))
    idx, d2 = np.zeros(len(src_all), np.int32), np.zeros(len(src_all), F32)
    p = ctx.icp_params()
    p.fitness_idx = idx.ctypes.data_as(C.POINTER(C.c_int32))
    refused(lambda: ctx.icp_vgicp_batch(src_all, off, m, src_normals_all=sn_all, params=p))
    p = ctx.icp_params()
    p.fitness_d2 = d2.ctypes.data_as(C.POINTER(C.c_float))
    refused(lambda: ctx.icp_vgicp_batch(src_all, off, m, src_normals_all=sn_all, params=p))
    assert not idx.any() and not d2.any()
    # more partial rows than 32-bit indexing takes: refused from the offsets alone, before a scan is read
    nbig = 0x7fff0000 // 2048 + 1
    big_off = np.arange(nbig + 1, dtype=np.int64) * (2048 * 256)
    for name in ("kss_icp_vgicp_batch", "kss_icp_vgicp_batch_dev"):
        refused(lambda: ctx._chk(raw(name, off=B._p(big_off), n=nbig)[0], name))
        assert raw(name, off=B._p(big_off), n=nbig)[0] == -1 and "32-bit" in L.kss_last_error(ctx.h).decode()
    rc, res, info = raw("kss_icp_vgicp_batch", off=B._p(big_off[:nbig]), n=nbig - 1, map=None)           # one scan fewer passes that check
    assert rc == -1 and "map" in L.kss_last_error(ctx.h).decode()
    # last_info = NULL is accepted
    rc, res, _ = raw(info=None)
    assert rc == 0
    for r, w in zip(res, want):
        assert np.array_equal(_bits(r.matrix()), _bits(w["T"])) and r.iterations == w["iterations"] and r.state == w["state"]
    good()
