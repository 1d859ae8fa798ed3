"""A voxel map that grows on the device (kss_vmap_create_box, kss_vmap_insert[_dev]) against the restatement in
tests/vmap_insert_ref.py, which continues every voxel's f64 sums as the header defines: kss_vmap_read and kss_vmap_info are
compared BIT FOR BIT throughout.  Then what a grown map is for: the calls that register against it see the map kss_vmap_create
builds from the concatenation, and the scan-to-map sequence stays registered where the static map of the first view runs out."""
import ctypes as C

import numpy as np
import pytest

import vgicp_ref as V
import vmap_insert_ref as R

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
WRAP = 2048 * 256 + 300   # the first count at which a grid-stride walk of 2048 workgroups of 256 wraps
BAR = 5e-3                # 1.5 x the restatement's largest error over both seeds on the CPU, 3.42e-3 (test_vmap_insert_host.py)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)


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


def _both(m, ref, pts, nrm, T=None):
    """The insert on the device and restated: the same tallies, then the same map."""
    got = m.insert(pts, nrm, T)
    want = R.insert(ref, pts, nrm, T)
    assert np.array_equal(got, want), (got, want)
    _same_map(m, ref)
    return got


def _pose(pkg, deg=17.0, t=(0.05, -0.02, 0.04)):
    T = np.eye(4)
    T[:3, :3] = pkg.synth.rot_axis_angle(R.AXIS, np.deg2rad(deg))
    T[:3, 3] = t
    return T.astype(F32)


def _halves(pkg, n, scale=1.05):
    """Two independent samplings of the bumpy surface with unit normals; the second a little larger, so part of it lies outside
    the first one's box."""
    rng = np.random.default_rng(n)
    return (pkg.synth.bumpy(n, n).astype(F32), _unit(rng, n), (pkg.synth.bumpy(500 + n, n) * scale).astype(F32), _unit(rng, n))


@pytest.mark.parametrize("leaf", [1e3, 0.1, 1e-2])
@pytest.mark.parametrize("n", [1, 255, 257, 1000, 5000])
def test_create_then_insert_is_create_of_the_concatenation(pkg, ctx, n, leaf):
    """Consequence 1, against the restatement and against the independent vgicp_ref.build of A || B_inside."""
    A, an, B, bn = _halves(pkg, n)
    m = ctx.vmap(A, leaf, normals=an)
    try:
        ref = R.create(A, an, leaf)
        _same_map(m, ref)                              # kss_vmap_create's bits are what they were
        sel = R.select(ref, B, bn)[0]
        info = _both(m, ref, B, bn)
        print("n %d leaf %g: added %d, outside %d, %d voxels created of %d" % (n, leaf, info[0], info[2], info[3], len(ref.lin)))
        assert info[0] == sel.sum() and info[1] == 0 and info[0] + info[2] == n
        _same_map(m, V.build(np.concatenate([A, B[sel]]), np.concatenate([an, bn[sel]]), leaf))
        if n >= 255 and leaf == 0.1:
            assert 0 < info[2] < n and info[3] > 0
    finally:
        m.close()


@pytest.mark.parametrize("n,chunk", [(257, 1), (1000, 7), (1000, 256), (1000, 1000)])
def test_box_map_any_split(pkg, ctx, n, chunk):
    """Consequence 2.  The box is the cloud's own, so the whole is also vgicp_ref.build's map."""
    A = pkg.synth.bumpy(9, n).astype(F32)
    an = _unit(np.random.default_rng(9), n)
    lo, hi = A.min(0), A.max(0)
    m = ctx.vmap_box(lo, hi, 0.1)
    try:
        assert m.read()[0].size == 0 and m.read()[1].shape == (0, 10)
        _same_map(m, R.box(lo, hi, 0.1))
        for i in range(0, n, chunk):
            m.insert(A[i:i + chunk], an[i:i + chunk])
        whole = V.build(A, an, 0.1)
        _same_map(m, whole)
        ref = R.box(lo, hi, 0.1)
        R.insert(ref, A, an)
        _same_map(m, ref)
    finally:
        m.close()


def test_voxel_renumbering(pkg, ctx):
    """An insert that touches existing voxels only, one that only creates voxels whose lin interleave the old ones (the odd z
    layers after the even ones), and a mixed one."""
    A, an, B, bn = _halves(pkg, 5000, scale=1.0)
    m = ctx.vmap_box(R.BOX_LO, R.BOX_HI, 0.1)
    ref = R.box(R.BOX_LO, R.BOX_HI, 0.1)
    try:
        layer = V.cells(A, ref.lo, ref.inv)[:, 2].astype(np.int64) % 2
        even = _both(m, ref, A[layer == 0], an[layer == 0])
        assert even[3] == len(ref.lin) > 100
        odd = _both(m, ref, A[layer == 1], an[layer == 1])
        assert odd[3] == len(ref.lin) - even[3] > 100                # every voxel of this insert is new ...
        z = ref.lin // (int(ref.dims[0]) * int(ref.dims[1])) % 2
        assert 0.2 < z.mean() < 0.8 and (np.diff(z) != 0).sum() > 10  # ... and they lie between the old ones
        again = _both(m, ref, A, an)                                 # the same cloud once more: no voxel is created
        assert again[3] == 0 and again[0] == len(A)
        mixed = _both(m, ref, B, bn)
        assert 0 < mixed[3] < mixed[0]
    finally:
        m.close()


def test_pose(pkg, ctx):
    A, an, B, bn = _halves(pkg, 1000, scale=1.0)
    A[7, 0] = -0.0
    T = _pose(pkg)
    m = ctx.vmap_box(R.BOX_LO, R.BOX_HI, 0.1)
    ref = R.box(R.BOX_LO, R.BOX_HI, 0.1)
    a, b = ctx.vmap_box(R.BOX_LO, R.BOX_HI, 0.1), ctx.vmap_box(R.BOX_LO, R.BOX_HI, 0.1)
    try:
        _both(m, ref, A, an, T)
        _both(m, ref, B, bn, _pose(pkg, -40.0, (0.3, 0.2, -0.1)))
        for x, Tx in ((a, None), (b, np.eye(4))):                    # consequence 3
            x.insert(A, an, Tx)
            x.insert(B, bn, Tx)
        la, sa = a.read()
        lb, sb = b.read()
        assert np.array_equal(la, lb) and np.array_equal(_bits(sa), _bits(sb)) and np.array_equal(_bits(a.info()), _bits(b.info()))
    finally:
        for x in (m, a, b):
            x.close()


def test_normals_and_entries(pkg, ctx):
    """Computed normals against given ones (computed from the cloud as passed in, before the pose; normals_k is read), the host
    entry against the _dev entry."""
    import torch
    A, _, B, _ = _halves(pkg, 1000, scale=1.0)
    an, bn = (ctx.normals(x.astype(F64), 20).astype(F32) for x in (A, B))
    T = _pose(pkg)
    ref = R.create(A, an, 0.1)
    R.insert(ref, B, bn, T)
    dA, dan, dB, dbn = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (A, an, B, bn))
    torch.cuda.synchronize()
    maps = []
    try:
        for given in (True, False):
            m = ctx.vmap(A, 0.1, normals=an)
            maps.append(m)
            info = m.insert(B, bn if given else None, T)
            _same_map(m, ref)
            m = ctx.vmap_dev(dA.data_ptr(), len(A), 0.1, dan.data_ptr())
            maps.append(m)
            assert np.array_equal(info, m.insert_dev(dB.data_ptr(), len(B), dbn.data_ptr() if given else None, T))
            _same_map(m, ref)
        bn12 = ctx.normals(B.astype(F64), 12).astype(F32)
        m = ctx.vmap(A, 0.1, normals=an)
        maps.append(m)
        m.insert(B, None, T, normals_k=12)
        ref12 = R.create(A, an, 0.1)
        R.insert(ref12, B, bn12, T)
        _same_map(m, ref12)
    finally:
        for m in maps:
            m.close()


def test_filtering(pkg, ctx):
    """Non-finite points and normals are counted and left out; a cloud with nothing to add leaves every bit where it was."""
    rng = np.random.default_rng(5)
    A, an, B, bn = _halves(pkg, 1000)
    B[rng.random(1000) < 0.03, 0] = np.nan
    B[rng.random(1000) < 0.02, 2] = np.inf
    bn[rng.random(1000) < 0.03] = np.nan
    bn[rng.random(1000) < 0.02, 1] = -np.inf
    B[0] = np.nan; bn[999, 2] = np.inf                               # the first and the last point too
    m = ctx.vmap(A, 0.1, normals=an)
    ref = R.create(A, an, 0.1)
    try:
        info = _both(m, ref, B, bn)
        assert 40 < info[1] < 200 and info[2] > 0 and info.sum() - info[3] == 1000
        lin0, st0 = m.read()
        i0 = m.info()
        far = m.insert(B + F32(100.0), bn)                           # wholly outside the box
        assert np.array_equal(far, [0, info[1], 1000 - info[1], 0])
        nan = m.insert(np.full_like(B, np.nan), bn)
        assert np.array_equal(nan, [0, 1000, 0, 0])
        nan = m.insert(B, np.full_like(bn, np.nan), _pose(pkg))
        assert np.array_equal(nan, [0, 1000, 0, 0])
        big = np.eye(4, dtype=F32)
        big[0, 0] = 3e38                                             # a finite T that moves finite points to infinity
        inf = m.insert(np.full_like(B, 2.0), _unit(rng, 1000), big)
        assert np.array_equal(inf, [0, 1000, 0, 0])
        lin1, st1 = m.read()
        assert np.array_equal(lin0, lin1) and np.array_equal(_bits(st0), _bits(st1)) and np.array_equal(_bits(i0), _bits(m.info()))
        _same_map(m, ref)
    finally:
        m.close()


def test_large_insert_wraps_the_grid_stride_loops(pkg, ctx):
    """One insert of WRAP points at leaf 0.02 (160^3 cells, a dozen points a voxel) behind a small one."""
    rng = np.random.default_rng(2)
    A, an = pkg.synth.bumpy(6, 1000).astype(F32), _unit(rng, 1000)
    B, bn = pkg.synth.bumpy(7, WRAP).astype(F32), _unit(rng, WRAP)
    B[-1] = np.nan
    m = ctx.vmap_box(R.BOX_LO, R.BOX_HI, 0.02)
    ref = R.box(R.BOX_LO, R.BOX_HI, 0.02)
    try:
        _both(m, ref, A, an)
        info = _both(m, ref, B, bn, _pose(pkg, 5.0))
        assert info[0] == WRAP - 1 and info[1] == 1 and ref.mapped == WRAP + 999
        print("%d points: %d voxels, largest %d" % (WRAP, len(ref.lin), int(ref.N.max())))
    finally:
        m.close()


@pytest.fixture(scope="module")
def scene0(pkg, ctx):
    src, tgt, R_true, t_true = V.halves_pair(pkg.synth, 8, 4000, 10.0, axis=[0.3, -0.5, 1.0])
    nr = [ctx.normals(x.astype(F64), 20).astype(F32) for x in (src, tgt)]
    return src, tgt, nr[0], nr[1], R_true, t_true


def test_downstream_calls_see_the_concatenation(pkg, ctx, scene0):
    """kss_vgicp_sums, kss_icp_vgicp and kss_icp_vgicp_batch against a grown map are those calls against
    kss_vmap_create(A || B_inside), bit for bit."""
    src, tgt, sn, tn, R_true, t_true = scene0
    A, an, B, bn = tgt[:2500], tn[:2500], tgt[2500:], tn[2500:]
    grown = ctx.vmap(A, 0.1, normals=an)
    ref = R.create(A, an, 0.1)
    sel = R.select(ref, B, bn)[0]
    assert 0 < sel.sum() < len(B)
    grown.insert(B, bn)
    whole = ctx.vmap(np.concatenate([A, B[sel]]), 0.1, normals=np.concatenate([an, bn[sel]]))
    try:
        la, sa = grown.read()
        lb, sb = whole.read()
        assert np.array_equal(la, lb) and np.array_equal(_bits(sa), _bits(sb)) and np.array_equal(_bits(grown.info()), _bits(whole.info()))
        Rn = pkg.synth.rot_axis_angle([0.2, -1.0, 0.4], 0.7).astype(F32)
        assert np.array_equal(_bits(ctx.vgicp_sums(src, sn, grown, 0.01, Rn=Rn)), _bits(ctx.vgicp_sums(src, sn, whole, 0.01, Rn=Rn)))
        a = ctx.icp_vgicp(src, whole, sn, trace_cap=64)
        b = ctx.icp_vgicp(src, grown, sn, trace_cap=64)
        assert a["iterations"] >= 2 and a["converged"]
        _same_run(a, b)
        eR, et = V.errors(b["T"], R_true, t_true)
        assert eR <= 1e-3 and et <= 1e-3
        src2, sn2 = src[::2] + F32(0.01), sn[::2]
        single = [b, ctx.icp_vgicp(src2, grown, sn2)]
        off = np.array([0, len(src), len(src) + len(src2)], np.int64)
        batch = ctx.icp_vgicp_batch(np.concatenate([src, src2]), off, grown, np.concatenate([sn, sn2]))
        for s_, b_ in zip(single, batch):
            assert b_["iterations"] == s_["iterations"] and b_["state"] == s_["state"]
            assert np.array_equal(_bits(b_["T"]), _bits(s_["T"])) and np.array_equal(_bits(b_["info"]), _bits(s_["info"]))
    finally:
        grown.close()
        whole.close()


def test_empty_box_map_has_no_correspondences(pkg, ctx, scene0):
    src, _, sn, _, _, _ = scene0
    m = ctx.vmap_box(R.BOX_LO, R.BOX_HI, 0.1)
    try:
        _same_map(m, R.box(R.BOX_LO, R.BOX_HI, 0.1))
        assert np.array_equal(m.info()[:5], [0, 0, 33, 33, 33])
        got = ctx.icp_vgicp(src, m, sn)
        assert got["state"] == V.STATE_NO_CORRESPONDENCES and got["iterations"] == 0 and got["info"][0] == 0 and got["info"][3] == 0
        assert ctx.vgicp_sums(src, sn, m)[0] == 0
    finally:
        m.close()


def test_grown_map_outlives_other_calls(pkg, scene0):
    """test_map_outlives_other_calls's pattern on a context of its own: a 60k x 60k point-to-point registration, which has to
    allocate the whole workspace, between two inserts."""
    src, tgt, sn, tn, _, _ = scene0
    A, an, B, bn, D, dn = tgt[:1500], tn[:1500], tgt[1500:3000], tn[1500:3000], tgt[3000:], tn[3000:]
    c = pkg.Context(0)
    try:
        m = c.vmap(A, 0.1, normals=an)
        ref = R.create(A, an, 0.1)
        _both(m, ref, B, bn)
        big_s, big_t = pkg.synth.make_pair(3, 60000, R=pkg.synth.rot_axis_angle([0, 0, 1], 0.1), shape="bumpy")
        assert c.icp(big_s, big_t, c.icp_params(max_iterations=3))["iterations"] == 3
        c.icp_gicp(src, tgt, sn, tn, params=c.icp_params(max_iterations=2))
        _same_map(m, ref)
        before = c.icp_vgicp(src, m, sn, trace_cap=64)
        _both(m, ref, D, dn, _pose(pkg, 1.0, (0.001, 0.0, 0.002)))
        assert c.icp(big_s, big_t, c.icp_params(max_iterations=2))["iterations"] == 2
        _same_map(m, ref)
        assert before["iterations"] >= 2
        # the context goes with the grown map still alive: it frees it
    finally:
        c.close()


def test_refused_arguments_change_nothing(pkg, ctx, scene0):
    src, tgt, sn, tn, _, _ = scene0
    L = pkg.load_library()
    m = ctx.vmap(tgt[:2000], 0.1, normals=tn[:2000])
    m.insert(tgt[2000:3000], tn[2000:3000])
    lin0, st0 = m.read()
    i0 = m.info()
    good = ctx.icp_vgicp(src, m, sn, trace_cap=64)
    B, bn = np.ascontiguousarray(tgt[3000:]), np.ascontiguousarray(tn[3000:])
    pB, pn = B.ctypes.data_as(C.c_void_p), bn.ctypes.data_as(C.c_void_p)
    eye = np.eye(4, dtype=F32)
    info = np.full(4, -7.0)
    pi = info.ctypes.data_as(C.c_void_p)

    def refused(call):
        with pytest.raises(pkg.KssError) as e:
            call()
        assert e.value.status == -1

    # both insert entries refuse on the host, before any pointer is read as a device or host address
    for f in (L.kss_vmap_insert, L.kss_vmap_insert_dev):
        assert f(None, m.h, pB, len(B), pn, None, 20, pi) == -1                                # a NULL context
        assert f(ctx.h, None, pB, len(B), pn, None, 20, pi) == -1                              # a NULL map
        assert f(ctx.h, m.h, None, len(B), pn, None, 20, pi) == -1                             # NULL points
        for n in (0, -5):
            assert f(ctx.h, m.h, pB, n, pn, None, 20, pi) == -1
        for k in (2, 65, 0, -1):
            assert f(ctx.h, m.h, pB, len(B), None, None, k, pi) == -1                          # normals to compute at a bad k
        for bad in (np.nan, np.inf, -np.inf):
            for at in (0, 7, 11, 12, 15):
                T = eye.copy().reshape(16)
                T[at] = bad
                assert f(ctx.h, m.h, pB, len(B), pn, T.ctypes.data_as(C.c_void_p), 20, pi) == -1
    assert (info == -7.0).all()
    refused(lambda: m.insert(np.zeros((0, 3), F32), np.zeros((0, 3), F32)))
    other = pkg.Context(0)
    try:
        theirs = other.vmap_box(R.BOX_LO, R.BOX_HI, 0.1)
        assert L.kss_vmap_insert(ctx.h, theirs.h, pB, len(B), pn, None, 20, pi) == -1          # a map of another context
        assert L.kss_vmap_insert_dev(ctx.h, theirs.h, pB, len(B), pn, None, 20, pi) == -1
        assert theirs.insert(B, bn)[0] == len(B)
        theirs.close()
    finally:
        other.close()
    # the box
    vp = pkg.vmap_params(leaf=0.1)
    lo, hi = np.array(R.BOX_LO, F32), np.array(R.BOX_HI, F32)
    plo, phi = lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p)
    h = C.c_void_p()
    assert L.kss_vmap_create_box(None, plo, phi, C.byref(vp), C.byref(h)) == -1
    assert L.kss_vmap_create_box(ctx.h, None, phi, C.byref(vp), C.byref(h)) == -1
    assert L.kss_vmap_create_box(ctx.h, plo, None, C.byref(vp), C.byref(h)) == -1
    assert L.kss_vmap_create_box(ctx.h, plo, phi, None, C.byref(h)) == -1
    assert L.kss_vmap_create_box(ctx.h, plo, phi, C.byref(vp), None) == -1
    assert not h.value
    for bad in (np.nan, np.inf, -np.inf):
        refused(lambda: ctx.vmap_box([bad, 0, 0], R.BOX_HI, 0.1))
        refused(lambda: ctx.vmap_box(R.BOX_LO, [1, bad, 1], 0.1))
    refused(lambda: ctx.vmap_box([0, 0, 0], [1, 1, -1e-3], 0.1))                               # hi < lo
    for leaf in (0.0, -0.1, float("nan"), float("inf"), 1e-40):                                # the last: an inv of infinity
        refused(lambda: ctx.vmap_box(R.BOX_LO, R.BOX_HI, leaf))
    refused(lambda: ctx.vmap_box(R.BOX_LO, R.BOX_HI, 7e-3))                                    # 458^3 cells, over 2^26
    ok = ctx.vmap_box(R.BOX_LO, R.BOX_HI, 8e-3)                                                # 401^3 cells, under it
    assert ok.info()[2] * ok.info()[3] * ok.info()[4] <= 2 ** 26
    ok.close()
    # nothing else happened: the map and a good call are what they were, and a good insert follows
    lin1, st1 = m.read()
    assert np.array_equal(lin0, lin1) and np.array_equal(_bits(st0), _bits(st1)) and np.array_equal(_bits(i0), _bits(m.info()))
    _same_run(good, ctx.icp_vgicp(src, m, sn, trace_cap=64))
    ref = R.create(tgt[:2000], tn[:2000], 0.1)
    R.insert(ref, tgt[2000:3000], tn[2000:3000])
    _both(m, ref, B, bn)
    m.close()
    refused(lambda: m.insert(B, bn))                                                           # a closed map


@pytest.fixture(scope="module")
def scenes(pkg, O):
    return {seed: R.sequence_scene(pkg.synth, O, seed) for seed in (8, 3)}


@pytest.mark.parametrize("seed", [8, 3])
def test_sequence_growing_map(pkg, ctx, O, scenes, seed):
    """Every scan is inserted at its estimated pose.  Every scan converges, the largest error over scans 1..7 stays under BAR on
    both R and t, and at every step the device's map is the restatement's, which inserts with the device's pose."""
    scene = scenes[seed]
    m = ctx.vmap_box(R.BOX_LO, R.BOX_HI, R.LEAF)
    ref = R.box(R.BOX_LO, R.BOX_HI, R.LEAF)
    p = ctx.icp_params(max_iterations=50)
    try:
        out = R.run_sequence(O, scene, lambda k, pts, nr: ctx.icp_vgicp(pts, m, nr, params=p),
                             lambda k, scan, sn, T: _both(m, ref, scan, sn, T), True)
        for k, r, eR, et, _ in out:
            print("seed %d scan %d: %d passes, state %d, kept %d of %d, |R| %.2e |t| %.2e" % (
                seed, k, r["iterations"], r["state"], int(r["info"][0]), len(scene[k][0]), eR, et))
        assert all(r["converged"] for _, r, _, _, _ in out)
        assert max(e[2] for e in out) <= BAR and max(e[3] for e in out) <= BAR
        assert ref.mapped == sum(len(s[0]) for s in scene)
    finally:
        m.close()


@pytest.mark.parametrize("seed", [8, 3])
def test_sequence_static_map_runs_out(pkg, ctx, O, scenes, seed):
    """Only scan 0 is mapped: scans 6 and 7 find no correspondences."""
    scene = scenes[seed]
    m = ctx.vmap_box(R.BOX_LO, R.BOX_HI, R.LEAF)
    p = ctx.icp_params(max_iterations=50)
    try:
        out = R.run_sequence(O, scene, lambda k, pts, nr: ctx.icp_vgicp(pts, m, nr, params=p),
                             lambda k, scan, sn, T: m.insert(scan, sn, T), False)
        for k, r, eR, et, _ in out:
            print("seed %d static scan %d: %d passes, state %d, kept %d, |R| %.2e |t| %.2e" % (
                seed, k, r["iterations"], r["state"], int(r["info"][0]), eR, et))
        assert [e[1]["state"] for e in out[5:]] == [V.STATE_NO_CORRESPONDENCES] * 2
    finally:
        m.close()


def _equal_maps(a, b):
    (la, sa), (lb, sb) = a.read(), b.read()
    assert np.array_equal(la, lb) and np.array_equal(_bits(sa), _bits(sb)) and np.array_equal(_bits(a.info()), _bits(b.info()))


@pytest.mark.parametrize("n", [1, 255, 257, 1000])
def test_create_is_box_plus_insert(pkg, ctx, n):
    """kss_vmap_create is the cloud's own box, made empty, and one insert: the two doors into the one pipeline give the same bits."""
    A, an, _, _ = _halves(pkg, n)
    m, b = ctx.vmap(A, 0.1, normals=an), ctx.vmap_box(A.min(0), A.max(0), 0.1)
    try:
        info = b.insert(A, an)
        _equal_maps(m, b)
        assert np.array_equal(info, [n, 0, 0, len(m.read()[0])]), info
    finally:
        m.close(); b.close()


def test_non_finite_through_both_doors(pkg, ctx):
    """A NaN coordinate, an infinite coordinate and a NaN normal component, at the first, a middle and the last index: the create
    leaves the three out of its box and of its map, the insert into the finite rows' box counts them as not mapped."""
    A, an, _, _ = _halves(pkg, 257)
    A[0, 1] = np.nan; A[128, 2] = np.inf; an[256, 0] = np.nan
    ok = np.isfinite(A).all(1) & np.isfinite(an).all(1)
    assert ok.sum() == 254
    m, b = ctx.vmap(A, 0.1, normals=an), ctx.vmap_box(A[ok].min(0), A[ok].max(0), 0.1)
    try:
        info = b.insert(A, an)
        _equal_maps(m, b)
        assert np.array_equal(info, [254, 3, 0, len(m.read()[0])]), info
        assert m.info()[0] == 254
        _same_map(m, V.build(A, an, 0.1))
    finally:
        m.close(); b.close()


def test_two_inserts_into_a_created_map(pkg, ctx):
    """A created map has records of exactly its voxel count and none to spare: the first insert allocates its destination, the
    second goes into the records the first one replaced (too small by now, so they are grown) -- the swap in both directions."""
    A, an, B, bn = _halves(pkg, 1000)
    m = ctx.vmap(A, 0.1, normals=an)
    ref = R.create(A, an, 0.1)
    try:
        _same_map(m, ref)
        first = _both(m, ref, B, bn)
        second = _both(m, ref, (B * F32(0.97)).astype(F32), bn, _pose(pkg, 5.0, (0.01, 0.0, -0.01)))
        third = _both(m, ref, A, an)                                 # no voxel is created: the spare is large enough as it is
        assert first[3] > 0 and second[3] > 0 and third[3] == 0 and third[0] == len(A)
    finally:
        m.close()
