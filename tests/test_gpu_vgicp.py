"""Voxelized generalized ICP on the device (kss_vmap_*, kss_vgicp_sums, kss_icp_vgicp[_dev]) against the independent restatement in
tests/vgicp_ref.py: the map bit for bit, the record and the loop within test_gpu_gicp's bars, the anchor to kss_gicp_sums on a map
of one point per voxel, and what a map is for: it outlives every other call on its context.  The scenes are generalized ICP's
(gicp_ref.halves_pair): two independent samplings of one surface, no source point is a target point.
There is one source form, packed float triples: the loop keeps its positions that way, so no float4 form exists to compare."""
import ctypes as C

import numpy as np
import pytest

import vgicp_ref as V

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
WRAP = 2048 * 256 + 300   # the first source count at which the rows kernel's grid-stride walk wraps (test_gpu_pair_bits.py)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)


def _normals(ctx, cloud):
    return ctx.normals(cloud.astype(F64), 20).astype(F32)


def _same_map(m, ref):
    lin, stats = m.read()
    assert np.array_equal(lin, ref.lin)
    assert np.array_equal(_bits(stats), _bits(ref.stats))
    assert np.array_equal(_bits(m.info()), _bits(ref.info()))


def _same_run(a, b):
    assert b["iterations"] == a["iterations"] and b["state"] == a["state"] and b["converged"] == a["converged"]
    for k in ("trace_Tk", "trace_sums", "T", "info"):
        if k in a:
            assert np.array_equal(_bits(b[k]), _bits(a[k])), k
    assert np.array_equal(_bits(np.array([b["fitness"]])), _bits(np.array([a["fitness"]])))


@pytest.fixture(scope="module")
def bumpy_map(pkg, ctx):
    """5000 points of the bumpy surface with unit normals, its map at leaf 0.1 on the device and restated."""
    tgt = pkg.synth.bumpy(21, 5000).astype(F32)
    tn = _unit(np.random.default_rng(21), 5000)
    m = ctx.vmap(tgt, 0.1, normals=tn)
    yield tgt, tn, m, V.build(tgt, tn, 0.1)
    m.close()


@pytest.mark.parametrize("leaf", [1e3, 0.1, 1e-2, 1e-3])
@pytest.mark.parametrize("nt", [1, 255, 257, 1000, 5000])
def test_map_bit_for_bit(pkg, ctx, nt, leaf):
    """One voxel that holds everything (1e3), a few points per voxel (0.1), nearly every point alone (1e-2).  At 1e-3 the bumpy
    surface's box has 2.7e10 cells, far over the definition's 2^26: from two points on that is KSS_ERR_ARG by the definition,
    which the restatement applies (None) and the library must apply the same; 1e-2 is the finest leaf here that is a map."""
    tgt = pkg.synth.bumpy(nt, nt).astype(F32)
    tn = _unit(np.random.default_rng(nt), nt)
    ref = V.build(tgt, tn, leaf)
    if ref is None:
        assert leaf == 1e-3 and nt > 1
        with pytest.raises(pkg.KssError) as e:
            ctx.vmap(tgt, leaf, normals=tn)
        assert e.value.status == -1
        return
    m = ctx.vmap(tgt, leaf, normals=tn)
    try:
        print("nt %d leaf %g: dims %s, %d voxels, largest %d" % (nt, leaf, ref.dims, len(ref.lin), int(ref.stats[:, 0].max())))
        _same_map(m, ref)
        assert ref.stats[:, 0].sum() == nt == ref.mapped
        if leaf == 1e3:
            assert len(ref.lin) == 1
        if leaf == 1e-2:
            assert len(ref.lin) >= 0.9 * nt
        again = ctx.vmap(tgt, leaf, normals=tn)       # two builds of one cloud: the same bits whatever the atomics did
        _same_map(again, ref)
        again.close()
    finally:
        m.close()


def test_map_leaves_out_non_finite_targets(pkg, ctx):
    rng = np.random.default_rng(5)
    tgt = pkg.synth.bumpy(31, 1000).astype(F32)
    tn = _unit(rng, 1000)
    tgt[rng.random(1000) < 0.03, 0] = np.nan
    tgt[rng.random(1000) < 0.02, 2] = np.inf
    tgt[rng.random(1000) < 0.02, 1] = -np.inf
    tn[rng.random(1000) < 0.03] = np.nan
    tn[rng.random(1000) < 0.02, 1] = np.inf
    tgt[0] = np.nan                                   # the first and the last target too
    tn[999, 2] = -np.inf
    ref = V.build(tgt, tn, 0.1)
    assert 800 < ref.mapped < 960
    m = ctx.vmap(tgt, 0.1, normals=tn)
    _same_map(m, ref)
    m.close()


def test_map_entries_and_normals(pkg, ctx):
    """The host entry against the _dev entry, given normals against computed ones."""
    import torch
    tgt = pkg.synth.bumpy(41, 1000).astype(F32)
    tn = _normals(ctx, tgt)
    ref = V.build(tgt, tn, 0.1)
    maps = [ctx.vmap(tgt, 0.1, normals=tn), ctx.vmap(tgt, 0.1)]
    dt, dn = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (tgt, tn))
    torch.cuda.synchronize()
    maps += [ctx.vmap_dev(dt.data_ptr(), len(tgt), 0.1, dn.data_ptr()), ctx.vmap_dev(dt.data_ptr(), len(tgt), 0.1)]
    for m in maps:
        _same_map(m, ref)
        m.close()
    tn12 = ctx.normals(tgt.astype(F64), 12).astype(F32)   # normals_k is read when the normals are computed
    m = ctx.vmap(tgt, 0.1, normals_k=12)
    _same_map(m, V.build(tgt, tn12, 0.1))
    m.close()


@pytest.mark.parametrize("n", [1, 255, 257, 1000, WRAP])
def test_vgicp_sums_match_restatement(pkg, ctx, bumpy_map, n):
    """test_gicp_sums_match_restatement's tolerance: both sides are the same f64 cofactor form, 1e-12 * sum|term| leaves two
    decades.  The sources: on the surface (most have a voxel), uniform in a box that overhangs the map's (empty cells, outside),
    far outside, with non-finite positions and normals; max_d2 cuts the farther ones off."""
    tgt, tn, m, ref = bumpy_map
    rng = np.random.default_rng(n)
    src = (pkg.synth.bumpy(100 + n % 7, n) + rng.normal(scale=0.01, size=(n, 3))).astype(F32)
    kind = rng.random(n)
    box = kind < 0.15
    src[box] = rng.uniform(-1.8, 1.8, size=(int(box.sum()), 3)).astype(F32)
    src[(kind >= 0.15) & (kind < 0.18)] += F32(100.0)
    src[(kind >= 0.18) & (kind < 0.20), 1] = np.nan
    src[(kind >= 0.20) & (kind < 0.21), 0] = -np.inf
    sn = _unit(rng, n)
    sn[rng.random(n) < 0.05] = np.nan
    sn[rng.random(n) < 0.02, 2] = np.inf
    max_d2 = 0.002
    Rn = pkg.synth.rot_axis_angle(rng.normal(size=3), rng.uniform(0.1, 3.0)).astype(F32)
    gp = pkg.gicp_params(epsilon=1e-3)
    got = ctx.vgicp_sums(src, sn, m, max_d2, Rn=Rn, gp=gp)
    want, absc = V.sums(src, sn, ref, max_d2, Rn=Rn, eps=1e-3)
    err = np.abs(got - want) / np.maximum(absc, 1e-300)
    has, _ = V.lookup(ref, src)
    print("n %d: %d with a voxel, kept %d, max |got - ref| / sum|term| %.2e" % (n, int(has.sum()), int(got[0]), err.max()))
    if n >= 255:
        assert 0 < got[0] < has.sum() < n             # every way of not being kept occurs
    assert got[0] == want[0]
    assert np.all(np.abs(got - want) <= 1e-12 * absc), err
    assert got[29] == 0.0 and got[31] == 0.0
    assert np.array_equal(_bits(got), _bits(ctx.vgicp_sums(src, sn, m, max_d2, Rn=Rn, gp=gp)))
    if n == 257:                                      # no Rn is the identity
        a = ctx.vgicp_sums(src, sn, m, max_d2, gp=gp)
        assert np.array_equal(_bits(a), _bits(ctx.vgicp_sums(src, sn, m, max_d2, Rn=np.eye(3), gp=gp)))
        wi, ai = V.sums(src, sn, ref, max_d2, eps=1e-3)
        assert a[0] == wi[0] and np.all(np.abs(a - wi) <= 1e-12 * ai)


def test_vgicp_sums_anchor_to_gicp(pkg, ctx):
    """A jittered lattice with one target per cell of the map: N = 1 gives mean = q and S = nq nq^T exactly, so with idx the target
    of the source's cell the record is kss_gicp_sums' bit for bit in [0..27] and [30] ([28] sums an f64 distance here, a float
    one there).  The target of cell (0, 0, 0) sits on the cell's corner so that the map's origin is the lattice's."""
    rng = np.random.default_rng(77)
    h, g = 0.1, 12
    o = np.array([-0.55, 0.2, 1.05])
    c = np.stack(np.meshgrid(np.arange(g), np.arange(g), np.arange(g), indexing="ij"), -1).reshape(-1, 3)
    u = rng.uniform(0.2, 0.8, size=c.shape)
    u[(c == 0).all(1)] = 0.0
    tgt = (o + (c + u) * h).astype(F32)
    tn = _unit(rng, len(tgt))
    m = ctx.vmap(tgt, h, normals=tn)
    lin, stats = m.read()
    assert len(lin) == len(tgt) == g ** 3 and (stats[:, 0] == 1.0).all()
    n = 4000
    idx = rng.integers(0, len(tgt), size=n).astype(np.int32)
    src = (o + (c[idx] + rng.uniform(0.1, 0.9, size=(n, 3))) * h).astype(F32)
    ref = V.build(tgt, tn, h)
    has, v = V.lookup(ref, src)
    _, tv = V.lookup(ref, tgt)
    assert has.all() and np.array_equal(v, tv[idx])   # every source sits in the cell of its target
    sn = _unit(rng, n)
    Rn = pkg.synth.rot_axis_angle([0.2, -1.0, 0.4], 0.7).astype(F32)
    a = ctx.vgicp_sums(src, sn, m, 1.0, Rn=Rn)
    b = ctx.gicp_sums(src, sn, tgt, tn, idx, 1.0, Rn=Rn)
    m.close()
    assert a[0] == n
    keep = list(range(28)) + [30]
    assert np.array_equal(_bits(a[keep]), _bits(b[keep]))
    assert abs(a[28] - b[28]) <= 1e-6 * b[28]


SCENES = [(8, 4000, None, 10.0, [0.3, -0.5, 1.0]), (5, 20000, 2000, 10.0, None), (3, 4000, None, 5.0, None)]


@pytest.fixture(scope="module")
def scene0(pkg, ctx):
    src, tgt, R_true, t_true = V.halves_pair(pkg.synth, 8, 4000, 10.0, axis=[0.3, -0.5, 1.0])
    return src, tgt, _normals(ctx, src), _normals(ctx, tgt), R_true, t_true


@pytest.mark.parametrize("seed,n,n_src,deg,axis", SCENES)
def test_icp_vgicp_matches_restatement(pkg, ctx, O, seed, n, n_src, deg, axis):
    """test_icp_gicp_matches_restatement's bars.  Pass 0 works on the positions passed in, so its cells are the restatement's and
    its record agrees within the sums tolerance; later passes see positions that differ by the steps' float roundings."""
    src, tgt, _, _ = V.halves_pair(pkg.synth, seed, n, deg, axis=axis, n_src=n_src)
    sn, tn = _normals(ctx, src), _normals(ctx, tgt)
    m = ctx.vmap(tgt, 0.1, normals=tn)
    vm = V.build(tgt, tn, 0.1)
    _same_map(m, vm)
    got = ctx.icp_vgicp(src, m, sn, params=ctx.icp_params(max_iterations=60), trace_cap=64)
    m.close()
    ref = V.icp_vgicp(O, src, sn, vm, max_iterations=60)
    print("pair %d: %d / %d passes, state %d / %d, kept %d of %d" % (seed, got["iterations"], ref["iterations"], got["state"], ref["state"],
                                                                  int(got["info"][0]), len(src)))
    assert got["iterations"] == ref["iterations"] >= 1
    assert got["state"] == ref["state"] and got["converged"] == ref["converged"]
    s0, r0 = got["trace_sums"][0], ref["trace_sums"][0]
    _, a0 = V.sums(src, sn, vm, 1.0)
    print("  |trace_Tk| %.2e  |T| %.2e  |fitness| %.2e rel  first sums %.2e of sum|term|" % (
        np.abs(got["trace_Tk"] - ref["trace_Tk"]).max(), np.abs(got["T"] - ref["T"]).max(),
        abs(got["fitness"] - ref["fitness"]) / ref["fitness"], (np.abs(s0 - r0) / np.maximum(a0, 1e-300)).max()))
    assert s0[0] == r0[0]
    assert np.all(np.abs(s0 - r0) <= 1e-12 * a0)
    assert np.abs(got["trace_Tk"] - ref["trace_Tk"]).max() <= 1e-6
    assert np.abs(got["T"] - ref["T"]).max() <= 5e-6
    assert abs(got["fitness"] - ref["fitness"]) <= 1e-9 * ref["fitness"]
    assert got["info"][1] == len(src) and got["info"][3] == len(vm.lin)


def test_icp_vgicp_recovers_known_motion(pkg, ctx, scene0):
    src, tgt, sn, tn, R_true, t_true = scene0
    m = ctx.vmap(tgt, 0.1, normals=tn)
    got = ctx.icp_vgicp(src, m, sn)
    m.close()
    eR, et = V.errors(got["T"], R_true, t_true)
    print("%d passes, state %d, |R - R_true| %.2e, |t - t_true| %.2e" % (got["iterations"], got["state"], eR, et))
    assert got["converged"] and got["state"] in (2, 3, 4)
    assert eR <= 1e-3 and et <= 1e-3


def test_icp_vgicp_deterministic_and_dev_matches_host(pkg, ctx, scene0):
    import torch
    src, tgt, sn, tn, _, _ = scene0
    m = ctx.vmap(tgt, 0.1, normals=tn)
    a = ctx.icp_vgicp(src, m, sn, trace_cap=64)
    assert a["iterations"] >= 2
    _same_run(a, ctx.icp_vgicp(src, m, sn, trace_cap=64))
    _same_run(a, ctx.icp_vgicp(src, m, None, trace_cap=64))          # computed source normals are the given ones
    s, dsn = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (src, sn))
    torch.cuda.synchronize()
    for d_n in (dsn.data_ptr(), None):
        r, info = ctx.icp_vgicp_dev(s.data_ptr(), len(src), d_n, m, ctx.icp_params())
        assert r.iterations == a["iterations"] and r.state == a["state"]
        assert np.array_equal(_bits(r.matrix()), _bits(a["T"])) and r.fitness == a["fitness"]
        assert np.array_equal(_bits(info), _bits(a["info"]))
    x = ctx.vgicp_sums(src, sn, m)
    assert np.array_equal(_bits(x), _bits(ctx.vgicp_sums_dev(s.data_ptr(), dsn.data_ptr(), len(src), m)))
    assert np.array_equal(_bits(x), _bits(a["trace_sums"][0]))       # pass 0 of the loop is the record at the positions passed in
    m.close()


def test_map_outlives_other_calls(pkg, scene0):
    """On a context of its own, whose workspace is empty when the map is built: a point-to-point registration that has to
    allocate all of it, two sources against the map, the map destroyed and built again -- nothing moves a bit."""
    src, tgt, sn, tn, _, _ = scene0
    src2, sn2 = src[::2] + F32(0.01), sn[::2]
    c = pkg.Context(0)
    try:
        fresh = []
        for s_, n_ in ((src, sn), (src2, sn2)):
            f = c.vmap(tgt, 0.1, normals=tn)
            fresh.append(c.icp_vgicp(s_, f, n_, trace_cap=64))
            f.close()
        m = c.vmap(tgt, 0.1, normals=tn)
        lin0, st0 = m.read()
        big_s, big_t = pkg.synth.make_pair(3, 60000, R=pkg.synth.rot_axis_angle([0, 0, 1], 0.1), shape="bumpy")
        assert c.icp(big_s, big_t, c.icp_params(max_iterations=3))["iterations"] == 3
        c.icp_gicp(src, tgt, sn, tn, params=c.icp_params(max_iterations=2))
        lin1, st1 = m.read()
        assert np.array_equal(lin0, lin1) and np.array_equal(_bits(st0), _bits(st1))
        _same_run(fresh[0], c.icp_vgicp(src, m, sn, trace_cap=64))
        _same_run(fresh[1], c.icp_vgicp(src2, m, sn2, trace_cap=64))
        m.close()
        m = c.vmap(tgt, 0.1, normals=tn)
        lin2, st2 = m.read()
        assert np.array_equal(lin0, lin2) and np.array_equal(_bits(st0), _bits(st2))
        _same_run(fresh[0], c.icp_vgicp(src, m, sn, trace_cap=64))
        # the context goes with a map still alive: it frees it
    finally:
        c.close()


def test_vgicp_bad_arguments(pkg, ctx, scene0):
    src, tgt, sn, tn, _, _ = scene0
    m = ctx.vmap(tgt, 0.1, normals=tn)
    lin0, st0 = m.read()
    good = ctx.icp_vgicp(src, m, sn, trace_cap=64)

    def refused(call):
        with pytest.raises(pkg.KssError) as e:
            call()
        assert e.value.status == -1

    for leaf in (0.0, -0.1, float("nan"), float("inf")):
        refused(lambda: ctx.vmap(tgt, leaf, normals=tn))
    refused(lambda: ctx.vmap(np.zeros((0, 3), F32), 0.1, normals=np.zeros((0, 3), F32)))     # nt = 0
    refused(lambda: ctx.vmap(tgt, 0.1, normals=np.full_like(tn, np.nan)))                    # every target unmapped
    refused(lambda: ctx.vmap(tgt, 1e-3, normals=tn))                                         # a grid over 2^26 cells
    refused(lambda: ctx.vmap(tgt, 0.1, normals_k=2))
    refused(lambda: ctx.icp_vgicp(src, None, sn))                                            # a NULL map
    refused(lambda: ctx.vgicp_sums(src, sn, None))
    other = pkg.Context(0)
    try:
        theirs = other.vmap(tgt, 0.1, normals=tn)
        refused(lambda: ctx.icp_vgicp(src, theirs, sn))                                      # a map of another context
        refused(lambda: ctx.vgicp_sums(src, sn, theirs))
        assert other.icp_vgicp(src, theirs, sn)["iterations"] == good["iterations"]
        theirs.close()
    finally:
        other.close()
    for eps in (0.0, -1.0, 2.0, float("nan")):
        refused(lambda: ctx.icp_vgicp(src, m, sn, gp=pkg.gicp_params(epsilon=eps)))
        refused(lambda: ctx.vgicp_sums(src, sn, m, gp=pkg.gicp_params(epsilon=eps)))
    p = ctx.icp_params()
    cb = pkg.binding.ALLREDUCE_FN(lambda user, values, n: 0)
    p.allreduce = cb
    refused(lambda: ctx.icp_vgicp(src, m, sn, params=p))
    idx, d2 = np.zeros(len(src), np.int32), np.zeros(len(src), F32)
    p = ctx.icp_params()
    p.fitness_idx = idx.ctypes.data_as(C.POINTER(C.c_int32))
    refused(lambda: ctx.icp_vgicp(src, m, sn, params=p))
    p = ctx.icp_params()
    p.fitness_d2 = d2.ctypes.data_as(C.POINTER(C.c_float))
    refused(lambda: ctx.icp_vgicp(src, m, sn, params=p))
    assert not idx.any() and not d2.any()
    # nothing else happened: the map and a good call are what they were
    lin1, st1 = m.read()
    assert np.array_equal(lin0, lin1) and np.array_equal(_bits(st0), _bits(st1))
    _same_run(good, ctx.icp_vgicp(src, m, sn, trace_cap=64))
    m.close()
    refused(lambda: ctx.icp_vgicp(src, m, sn))                                               # a closed map


def test_vgicp_states(pkg, ctx, scene0):
    src, tgt, sn, tn, _, _ = scene0
    m = ctx.vmap(tgt, 0.1, normals=tn)
    eye = np.eye(4, dtype=F32)
    for bad in (src + F32(100.0), np.full_like(src, np.nan)):      # wholly outside the box; a cloud of NaNs
        got = ctx.icp_vgicp(bad, m, sn)
        assert got["state"] == 5 and got["iterations"] == 0 and not got["converged"]
        assert np.array_equal(got["T"], eye)
        assert got["info"][0] == 0.0 and np.isnan(got["fitness"])
    got = ctx.icp_vgicp(src, m, sn, params=ctx.icp_params(max_iterations=0))
    assert got["iterations"] == 0 and np.array_equal(got["T"], eye)
    assert got["info"][0] == 0.0 and got["info"][1] == len(src)
    m.close()
