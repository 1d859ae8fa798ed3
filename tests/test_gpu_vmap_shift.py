"""A voxel map whose box slides on the device (kss_vmap_shift, kss_vmap_recentre, kss_vmap_window) against the
restatement in tests/vmap_shift_ref.py: kss_vmap_read, kss_vmap_info and kss_vmap_window are compared BIT FOR BIT throughout.
Then the consequences the header states, on the device alone and against a kss_vmap_create_box map that never slides, the
cells a shift leaves behind, the calls that register against a shifted map, and the strip sequence: a sensor that travels ten
window-lengths' worth of cells in a table of 33^3."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import vgicp_ref as V
import vmap_insert_ref as R
import vmap_shift_ref as H

pytestmark = pytest.mark.gpu

F32, F64, I64 = np.float32, np.float64, np.int64
WRAP = 2048 * 256 + 300   # test_gpu_vmap_insert.py's large cloud
STRIP_BAR = 1.5 * 5.549e-3   # 1.5 x the restatement's largest error over both seeds on the CPU (test_vmap_shift_host.py)
KS = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (2, -3, 1)]


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
    assert np.array_equal(m.window(), ref.window())


def _state(m):
    lin, stats = m.read()
    return lin, stats, m.info(), m.window()


def _same_state(a, b):
    for x, y in zip(a, b):
        assert np.array_equal(_bits(x), _bits(y))


def _shift(m, ref, k):
    """The shift on the device and restated: the same tallies, then the same map."""
    got = m.shift(k)
    want = H.shift(ref, k)
    assert np.array_equal(got, want), (k, got, want)
    _same_map(m, ref)
    return got


def _insert(m, ref, pts, nrm, T=None):
    got = m.insert(pts, nrm, T)
    want = H.insert(ref, pts, nrm, T)
    assert np.array_equal(got, want), (got, want)
    _same_map(m, ref)
    return got


def _view(m):
    """A device map as the restatement's helpers read one: lin, stats, dims, base."""
    lin, stats = m.read()
    return SimpleNamespace(lin=lin, stats=stats, dims=m.info()[2:5].astype(I64), base=m.window())


def _cell_points(ref, cells, u=0.5):
    """One float point inside every LATTICE cell given, at fraction u of the cell."""
    return (ref.lo.astype(F64) + (np.asarray(cells, F64) + u) * ref.leaf).astype(F32)


def _box_pair(ctx, leaf=0.1, lo=H.W_LO, hi=H.W_HI):
    return ctx.vmap_box(lo, hi, leaf), H.box(lo, hi, leaf)


@pytest.mark.parametrize("nvox", [1, 255, 257])
def test_shift_small_maps(pkg, ctx, nvox):
    """Exactly nvox voxels of one point each, scattered over the 33^3 table: +-1 on each axis alone and a mixed-sign k, each
    from a fresh map."""
    rng = np.random.default_rng(nvox)
    flat = rng.choice(33 ** 3, 1) if nvox == 1 else np.concatenate(   # with the two corners of the table
        [[0, 33 ** 3 - 1], 1 + rng.choice(33 ** 3 - 2, nvox - 2, replace=False)])
    cells = np.stack(np.unravel_index(flat, (33, 33, 33)), axis=1)
    nr = _unit(rng, len(cells))
    for k in KS:
        m, ref = _box_pair(ctx)
        try:
            pts = _cell_points(ref, cells)
            _insert(m, ref, pts, nr)
            assert len(ref.lin) == len(cells)
            info = _shift(m, ref, k)
            assert info[0] + info[1] == len(cells) and info[2] == info[1]
        finally:
            m.close()


def test_shift_a_created_map(pkg, ctx):
    """About 4 900 voxels: 5 000 bumpy points at leaf 1e-2, from kss_vmap_create, whose lo is the cloud's minimum.  Every shift
    is the first one after the build: there is no spare yet."""
    A = pkg.synth.bumpy(5, 5000).astype(F32)
    an = _unit(np.random.default_rng(5), 5000)
    for k in KS + [(40, -25, 17)]:
        m = ctx.vmap(A, 1e-2, normals=an)
        ref = H.create(A, an, 1e-2)
        try:
            _same_map(m, ref)
            assert len(ref.lin) > 4800
            info = _shift(m, ref, k)
            assert info[1] > 0 and info[0] > 0
            if k == (2, -3, 1):                                      # a chain on one map: the spare changes hands every time
                for k2 in ((-2, 3, -1), (0, 0, 5), (7, 7, -7)):
                    _shift(m, ref, k2)
        finally:
            m.close()


def test_shift_to_the_edge_and_beyond(pkg, ctx):
    """dims - 1 leaves one layer, dims and more leave an empty map, and an insert into the empty map works."""
    A = pkg.synth.bumpy(6, 2000).astype(F32)
    an = _unit(np.random.default_rng(6), 2000)
    probe = H.create(A, an, 0.1)
    dims = [int(d) for d in probe.dims]
    for axis in range(3):
        for sign in (1, -1):
            m = ctx.vmap(A, 0.1, normals=an)
            ref = H.create(A, an, 0.1)
            try:
                k = [0, 0, 0]
                k[axis] = sign * (dims[axis] - 1)
                info = _shift(m, ref, k)
                assert 0 < info[0] < 0.2 * len(probe.lin)            # the cloud's own box: its last layer is occupied
                assert (H.local_cells(ref)[:, axis] == (0 if sign > 0 else dims[axis] - 1)).all()
            finally:
                m.close()
    for k in ((dims[0], 0, 0), (0, -dims[1], 0), (0, 0, dims[2] + 5), (1, 1000, -1), (-1 << 20, 0, 0)):
        m = ctx.vmap(A, 0.1, normals=an)
        ref = H.create(A, an, 0.1)
        try:
            info = _shift(m, ref, k)
            assert np.array_equal(info[:3], [0, len(probe.lin), len(A)])
            lin, stats = m.read()
            assert lin.size == 0 and stats.shape == (0, 10) and m.info()[0] == 0 and m.info()[1] == 0
            got = ctx.icp_vgicp(A, m, an)
            assert got["state"] == V.STATE_NO_CORRESPONDENCES and got["iterations"] == 0
            back = _cell_points(ref, ref.base + np.arange(500)[:, None] % np.array(dims))   # inside the window, wherever it went
            _insert(m, ref, back, an[:500])
            assert ref.mapped == 500 and len(ref.lin) > 0
            _shift(m, ref, (1, 0, 0))
        finally:
            m.close()


def test_empty_box_map_only_moves_its_base(pkg, ctx):
    m, ref = _box_pair(ctx)
    try:
        for k in ((3, 0, 0), (-40, 5, 1), (0, 0, 0), (1 << 20, -(1 << 20), 7)):
            info = _shift(m, ref, k)
            assert np.array_equal(info[:3], [0, 0, 0])
        assert np.array_equal(m.window(), [(1 << 20) - 37, 5 - (1 << 20), 8])
        pts = _cell_points(ref, ref.base + np.array([[0, 0, 0], [32, 32, 32], [5, 6, 7], [33, 0, 0], [0, -1, 0]]))
        info = _insert(m, ref, pts, _unit(np.random.default_rng(1), 5))
        assert np.array_equal(info, [3, 0, 2, 3])                    # the window's two corners are in, its neighbours are out
        assert np.array_equal(m.read()[0], [0, (7 * 33 + 6) * 33 + 5, 33 ** 3 - 1])
    finally:
        m.close()


@pytest.fixture(scope="module")
def cloud(pkg):
    n = 5000
    return pkg.synth.bumpy(11, n).astype(F32), _unit(np.random.default_rng(11), n)


def _survive(lin, dims, ks):
    dx, dy = int(dims[0]), int(dims[1])
    c = np.stack([lin % dx, lin // dx % dy, lin // (dx * dy)], axis=1)
    keep = np.ones(len(c), bool)
    for k in np.cumsum(np.asarray(ks, I64).reshape(-1, 3), axis=0):
        keep &= ((c - k >= 0) & (c - k < dims)).all(1)
    return keep


@pytest.mark.parametrize("k", [(1, 0, 0), (8, -5, 3), (-15, 2, 0)])
def test_consequence_1_on_the_device(ctx, cloud, k):
    """shift(0) changes nothing; shift(k) then shift(-k) leaves the survivors of shift(k), bit-equal and at their old lin --
    against the device's own first read, no restatement involved."""
    A, an = cloud
    m = ctx.vmap(A, 0.1, normals=an)
    try:
        s0 = _state(m)
        assert np.array_equal(m.shift((0, 0, 0)), [len(s0[0]), 0, 0, 0])
        _same_state(s0, _state(m))
        dims = s0[2][2:5].astype(I64)
        keep = _survive(s0[0], dims, [k])
        assert 0 < keep.sum() < len(keep)
        a = m.shift(k)
        assert np.array_equal(a[:3], [keep.sum(), (~keep).sum(), s0[1][~keep, 0].sum()])
        b = m.shift([-x for x in k])
        assert np.array_equal(b[:3], [keep.sum(), 0, 0]) and b[3] == -a[3]
        lin, stats, info, base = _state(m)
        assert np.array_equal(lin, s0[0][keep]) and np.array_equal(_bits(stats), _bits(s0[1][keep]))
        assert np.array_equal(base, [0, 0, 0]) and info[0] == s0[1][keep, 0].sum() and info[1] == keep.sum()
        assert np.array_equal(_bits(info[2:]), _bits(s0[2][2:]))
    finally:
        m.close()


@pytest.mark.parametrize("k1,k2", [((3, 0, 0), (0, 4, 0)), ((5, -2, 1), (-9, 2, 3)), ((20, 0, 0), (20, 0, 0))])
def test_consequence_2_on_the_device(ctx, cloud, k1, k2):
    A, an = cloud
    m = ctx.vmap(A, 0.1, normals=an)
    try:
        lin0, st0, info0, _ = _state(m)
        dims = info0[2:5].astype(I64)
        keep = _survive(lin0, dims, [k1, k2])
        d = m.shift(k1)[3] + m.shift(k2)[3]
        lin, stats, info, base = _state(m)
        assert np.array_equal(lin, lin0[keep] - int(d)) and np.array_equal(_bits(stats), _bits(st0[keep]))
        assert np.array_equal(base, np.add(k1, k2)) and info[0] == st0[keep, 0].sum()
        assert (keep.sum() == 0) == (k1 == (20, 0, 0))
    finally:
        m.close()


def _anchor_walk(pkg, ctx):
    """W slides by (3, 0, 0) and (0, 4, 0) with inserts between, G is a kss_vmap_create_box map over the same lo that contains
    every window and never slides.  Both get the same clouds, filtered on the CPU to W's window at the time."""
    W, wref = _box_pair(ctx)
    G = ctx.vmap_box(H.W_LO, [2.6, 2.6, 1.6], 0.1)
    rng = np.random.default_rng(21)
    for step, (k, off) in enumerate([((0, 0, 0), (0, 0, 0)), ((3, 0, 0), (0.3, 0.05, 0)), ((0, 4, 0), (0.35, 0.4, 0.02))]):
        _shift(W, wref, k)
        P = (pkg.synth.bumpy(30 + step, 3000) * 1.4 + np.array(off)).astype(F32)
        nr = _unit(rng, len(P))
        ok = H.in_window(wref, H.cells_of(wref, P))
        assert 0.5 * len(P) < ok.sum() < len(P)
        iw = _insert(W, wref, P[ok], nr[ok])
        ig = G.insert(P[ok], nr[ok])
        assert iw[2] == 0 and ig[2] == 0 and iw[0] == ig[0] == ok.sum()
    return W, wref, G


def test_consequences_3_and_4_against_a_box_that_never_slides(pkg, ctx):
    W, wref, G = _anchor_walk(pkg, ctx)
    try:
        assert np.array_equal(W.window(), [3, 4, 0]) and np.array_equal(G.window(), [0, 0, 0])
        assert np.array_equal(_bits(W.info()[5:]), _bits(G.info()[5:]))           # the same leaf, lo and inv
        w, g = _view(W), _view(G)
        lin, rows = H.as_seen_from(g, w)
        assert 0 < len(rows) < len(g.lin) and W.info()[0] < G.info()[0]
        assert np.array_equal(lin, w.lin) and np.array_equal(_bits(g.stats[rows]), _bits(w.stats))
        # consequence 4: sources in W's final window whose voxels W never dropped -- every voxel of G in that window is one
        rng = np.random.default_rng(23)
        src = (w.stats[::2, 1:4] + rng.normal(scale=0.01, size=(len(w.lin[::2]), 3))).astype(F32)
        src = src[H.in_window(wref, H.cells_of(wref, src))]
        sn = _unit(rng, len(src))
        Rn = pkg.synth.rot_axis_angle([0.2, -1.0, 0.4], 0.7).astype(F32)
        a = ctx.vgicp_sums(src, sn, W, 0.01, Rn=Rn)
        b = ctx.vgicp_sums(src, sn, G, 0.01, Rn=Rn)
        assert a[0] > 500 and np.array_equal(_bits(a), _bits(b))
        want, absc = H.sums(src, sn, wref, 0.01, Rn=Rn)
        assert a[0] == want[0] and np.all(np.abs(a - want) <= 1e-12 * absc)
    finally:
        W.close()
        G.close()


def test_stale_cells_and_re_entry(pkg, ctx, cloud):
    """A shift leaves no voxel number behind in the table: the slots the dropped voxels held find nothing, an insert of one point
    there starts a voxel from zero; and after shift(k), shift(-k) the cells that came back are empty and take new sums."""
    A, an = cloud
    rng = np.random.default_rng(31)
    k = np.array([12, -10, 6])
    m, ref = _box_pair(ctx)
    try:
        _insert(m, ref, A, an)
        old = ref.copy()
        info = _shift(m, ref, k)
        assert info[1] > 100
        keep = _survive(old.lin, old.dims, [k])
        c_old = H.local_cells(old)
        taken = {tuple(c) for c in (c_old[keep] - k)}                 # the slots the survivors hold now
        slots = np.array([c for c in c_old[~keep] if tuple(c) not in taken])
        assert len(slots) > 50
        src = _cell_points(ref, slots + ref.base)                     # the lattice cells those slots stand for now
        sn = _unit(rng, len(src))
        assert H.in_window(ref, H.cells_of(ref, src)).all()
        assert ctx.vgicp_sums(src, sn, m, 1.0)[0] == 0
        assert ctx.icp_vgicp(src, m, sn)["state"] == V.STATE_NO_CORRESPONDENCES
        one = _insert(m, ref, src[:1], sn[:1])
        assert np.array_equal(one, [1, 0, 0, 1])
        lin, stats = m.read()
        at = np.searchsorted(lin, (slots[0][2] * 33 + slots[0][1]) * 33 + slots[0][0])
        assert stats[at, 0] == 1.0 and np.array_equal(_bits(stats[at, 1:4]), _bits(src[0].astype(F64)))
        assert ctx.vgicp_sums(src, sn, m, 1.0)[0] == H.sums(src, sn, ref, 1.0)[0][0] == 1
    finally:
        m.close()
    m, ref = _box_pair(ctx)                                           # re-entry, on a fresh map
    try:
        _insert(m, ref, A, an)
        _shift(m, ref, k)
        _shift(m, ref, -k)
        gone = _cell_points(ref, c_old[~keep] + ref.base)             # base is 0 again: the dropped voxels' own cells
        gn = _unit(rng, len(gone))
        assert ctx.vgicp_sums(gone, gn, m, 1.0)[0] == 0
        again = _insert(m, ref, gone[:1], gn[:1])
        assert np.array_equal(again, [1, 0, 0, 1])
        lin, stats = m.read()
        at = np.searchsorted(lin, old.lin[~keep][0])
        assert lin[at] == old.lin[~keep][0] and stats[at, 0] == 1.0 and np.array_equal(_bits(stats[at, 1:4]), _bits(gone[0].astype(F64)))
        full = _insert(m, ref, A, an)                                 # every returned cell starts from zero sums
        assert full[3] == (~keep).sum() - 1 and full[0] == len(A)
        lin, stats = m.read()
        assert np.array_equal(lin, old.lin)
        assert np.array_equal(stats[~keep, 0][1:], old.N[~keep][1:]) and np.array_equal(stats[keep, 0], 2 * old.N[keep])
    finally:
        m.close()


@pytest.fixture(scope="module")
def scene0(pkg, ctx):
    src, tgt, R_true, t_true = V.halves_pair(pkg.synth, 8, 4000, 10.0, axis=[0.3, -0.5, 1.0])
    nr = [ctx.normals(x.astype(F64), 20).astype(F32) for x in (src, tgt)]
    return src, tgt, nr[0], nr[1], R_true, t_true


def test_registration_against_a_shifted_reinserted_map(pkg, ctx, O, scene0):
    """kss_icp_vgicp and kss_icp_vgicp_batch against a map that was shifted, shifted back and filled again, off base 0 at the
    end: the restatement's loop on the restatement's map (test_gpu_vgicp.py's bars), the known motion (test_gpu_vmap_insert.py's
    1e-3), and the batch the single call bit for bit."""
    src, tgt, sn, tn, R_true, t_true = scene0
    m, ref = _box_pair(ctx)
    try:
        _insert(m, ref, tgt[:2500], tn[:2500])
        _shift(m, ref, (6, -4, 2))
        _shift(m, ref, (-6, 4, -2))
        _insert(m, ref, tgt, tn)
        n_before = len(ref.lin)
        _shift(m, ref, (-1, -1, -1))                                  # the window [-1.7, 1.6)^3 still holds every voxel
        assert ref.mapped > len(tgt) and len(ref.lin) == n_before and ref.base.all()
        got = ctx.icp_vgicp(src, m, sn, params=ctx.icp_params(max_iterations=60), trace_cap=64)
        want = H.icp_vgicp(O, src, sn, ref, max_iterations=60)
        eR, et = V.errors(got["T"], R_true, t_true)
        print("%d / %d passes, state %d / %d, kept %d of %d, |T - T_ref| %.2e, |R| %.2e |t| %.2e" % (
            got["iterations"], want["iterations"], got["state"], want["state"], int(got["info"][0]), len(src),
            np.abs(got["T"] - want["T"]).max(), eR, et))
        assert got["iterations"] == want["iterations"] >= 2 and got["state"] == want["state"] and got["converged"]
        assert got["trace_sums"][0][0] == want["trace_sums"][0][0] > 0.5 * len(src)
        assert np.abs(got["trace_Tk"] - want["trace_Tk"]).max() <= 1e-6
        assert np.abs(got["T"] - want["T"]).max() <= 5e-6
        assert eR <= 1e-3 and et <= 1e-3
        src2, sn2 = src[::2] + F32(0.01), sn[::2]
        single = [ctx.icp_vgicp(src, m, sn), ctx.icp_vgicp(src2, m, sn2)]
        off = np.array([0, len(src), len(src) + len(src2)], np.int64)
        batch = ctx.icp_vgicp_batch(np.concatenate([src, src2]), off, m, np.concatenate([sn, sn2]))
        for s_, b_ in zip(single, batch):
            assert b_["iterations"] == s_["iterations"] and b_["state"] == s_["state"]
            assert np.array_equal(_bits(b_["T"]), _bits(s_["T"])) and np.array_equal(_bits(b_["info"]), _bits(s_["info"]))
    finally:
        m.close()


def test_large_map(pkg, ctx):
    """WRAP points at leaf 0.02 from kss_vmap_create, shifted by (3, -2, 1): the first shift after a build, so the kept count is
    above the spare's capacity of zero; then a second shift into the spare the first one left."""
    rng = np.random.default_rng(2)
    B, bn = pkg.synth.bumpy(7, WRAP).astype(F32), _unit(rng, WRAP)
    B[-1] = np.nan
    m = ctx.vmap(B, 0.02, normals=bn)
    ref = H.create(B, bn, 0.02)
    try:
        _same_map(m, ref)
        info = _shift(m, ref, (3, -2, 1))
        print("%d points, %d voxels: kept %d, dropped %d voxels with %d points" % (WRAP, int(info[0] + info[1]), *[int(x) for x in info[:3]]))
        assert info[0] > 20000 and info[1] > 0
        _shift(m, ref, (-40, 0, 0))
        _shift(m, ref, (0, 70, 0))
    finally:
        m.close()


def test_shifted_map_outlives_other_calls(pkg, scene0):
    """A 60k x 60k point-to-point registration, which allocates the whole workspace, between two shifts."""
    src, tgt, sn, tn, _, _ = scene0
    c = pkg.Context(0)
    try:
        m = c.vmap(tgt, 0.1, normals=tn)
        ref = H.create(tgt, tn, 0.1)
        _shift(m, ref, (2, -1, 1))
        big_s, big_t = pkg.synth.make_pair(3, 60000, R=pkg.synth.rot_axis_angle([0, 0, 1], 0.1), shape="bumpy")
        assert c.icp(big_s, big_t, c.icp_params(max_iterations=3))["iterations"] == 3
        _same_map(m, ref)
        _shift(m, ref, (-3, 2, 0))
        assert c.icp(big_s, big_t, c.icp_params(max_iterations=2))["iterations"] == 2
        _same_map(m, ref)
        _insert(m, ref, src, sn)
        # the context goes with the shifted map still alive: it frees it
    finally:
        c.close()


def test_refused_arguments_change_nothing(pkg, ctx, scene0):
    src, tgt, sn, tn, _, _ = scene0
    L = pkg.load_library()
    m = ctx.vmap(tgt[:3000], 0.1, normals=tn[:3000])
    ref = H.create(tgt[:3000], tn[:3000], 0.1)
    _shift(m, ref, (1, -1, 2))
    s0 = _state(m)
    dims = [int(d) for d in ref.dims]
    lim = 1 << 24
    info = np.full(4, -7.0)
    kout = np.full(3, -7, I64)
    pi, pk = info.ctypes.data_as(C.c_void_p), kout.ctypes.data_as(C.c_void_p)
    centre = np.zeros(3, F32)
    pc = centre.ctypes.data_as(C.c_void_p)

    def k_of(*k):
        a = np.array(k, I64)
        return a, a.ctypes.data_as(C.c_void_p)

    def unchanged_and_working():
        nonlocal s0
        assert (info == -7.0).all() and (kout == -7).all()
        _same_state(s0, _state(m))
        _shift(m, ref, (1, 0, 0))                                     # a good call behind the refusal ...
        _shift(m, ref, (-1, 0, 0))
        s0 = _state(m)

    one, p1 = k_of(1, 0, 0)
    base = np.zeros(3, I64)
    assert L.kss_vmap_window(None, base.ctypes.data_as(C.c_void_p)) == -1
    assert L.kss_vmap_window(m.h, None) == -1
    assert L.kss_vmap_shift(None, m.h, p1, pi) == -1                                              # a NULL context
    assert L.kss_vmap_shift(ctx.h, None, p1, pi) == -1                                            # a NULL map
    assert L.kss_vmap_shift(ctx.h, m.h, None, pi) == -1                                           # a NULL k
    unchanged_and_working()
    for k in ((-lim - 1 - 1, 0, 0), (0, lim + 1 - dims[1] + 1, 0), (0, 0, 1 << 40), (0, -(1 << 62), 0), ((1 << 63) - 1, 0, 0),
              (-(1 << 63), 0, 0)):
        a, pa = k_of(*k)
        assert H.shift(ref, k) is None
        assert L.kss_vmap_shift(ctx.h, m.h, pa, pi) == -1, k                                      # the window would leave +-2^24
        unchanged_and_working()
    assert L.kss_vmap_recentre(None, m.h, pc, 0, pk, pi) == -1
    assert L.kss_vmap_recentre(ctx.h, None, pc, 0, pk, pi) == -1
    assert L.kss_vmap_recentre(ctx.h, m.h, None, 0, pk, pi) == -1
    assert L.kss_vmap_recentre(ctx.h, m.h, pc, -1, pk, pi) == -1                                  # slack < 0
    unchanged_and_working()
    for at in range(3):
        for bad in (np.nan, np.inf, -np.inf, 3e6, -3e6):                                          # 3e6 * 10 cells is beyond 2^24
            centre[:] = 0
            centre[at] = bad
            assert H.recentre(ref, centre, 0) is None
            assert L.kss_vmap_recentre(ctx.h, m.h, pc, 0, pk, pi) == -1, (at, bad)
        unchanged_and_working()
    centre[:] = 0
    other = pkg.Context(0)
    try:
        theirs = other.vmap_box(R.BOX_LO, R.BOX_HI, 0.1)
        assert L.kss_vmap_shift(ctx.h, theirs.h, p1, pi) == -1                                    # a map of another context
        assert L.kss_vmap_recentre(ctx.h, theirs.h, pc, 0, pk, pi) == -1
        assert np.array_equal(theirs.window(), [0, 0, 0])
        assert np.array_equal(theirs.shift((1, 0, 0)), [0, 0, 0, 1]) and np.array_equal(theirs.window(), [1, 0, 0])
        theirs.close()
    finally:
        other.close()
    unchanged_and_working()
    # the edges themselves are taken, NULL info and k_out are fine, and recentre reports its k
    assert L.kss_vmap_shift(ctx.h, m.h, p1, None) == 0
    assert H.shift(ref, (1, 0, 0)) is not None
    _same_map(m, ref)
    centre[:] = tgt[:3000].mean(0)
    assert L.kss_vmap_recentre(ctx.h, m.h, pc, 0, None, None) == 0
    want = H.recentre(ref, centre, 0)
    _same_map(m, ref)
    k, inf = m.recentre(centre, 0)
    assert np.array_equal(k, [0, 0, 0]) and want is not None and np.array_equal(inf, [len(ref.lin), 0, 0, 0])
    k, inf = m.recentre(centre + F32(0.35), 2)
    wk, winf = H.recentre(ref, centre + F32(0.35), 2)
    assert np.array_equal(k, wk) and np.array_equal(inf, winf) and (np.abs(k) >= 3).all()
    _same_map(m, ref)
    _shift(m, ref, tuple(-lim - ref.base))
    _shift(m, ref, (2 * lim - dims[0], 0, 0))
    assert m.window()[0] + dims[0] == lim
    m.close()
    with pytest.raises(pkg.KssError) as e:
        m.shift((1, 0, 0))                                                                        # a closed map
    assert e.value.status == -1


@pytest.fixture(scope="module")
def strips(pkg, O):
    return {seed: H.strip_scene(pkg.synth, O, seed) for seed in (3, 8)}


@pytest.mark.parametrize("seed", [3, 8])
def test_strip_sequence(pkg, ctx, O, strips, seed):
    """Arm W on the device: a 33^3 table follows the sensor over 64 scans with recentre(t_found, slack 2) behind every insert.
    Every scan converges, the largest error over scans 1..63 stays under STRIP_BAR on both R and t, nothing is counted as outside,
    and at every step the device's map and window are the restatement's, which inserts and recentres with the device's pose."""
    scene = strips[seed]
    m, ref = _box_pair(ctx, H.STRIP_LEAF)
    p = ctx.icp_params(max_iterations=50)
    moves = []

    def put(k, scan, sn, T):
        assert _insert(m, ref, scan, sn, T)[2] == 0

    def recentre(t):
        k, info = m.recentre(t, H.STRIP_SLACK)
        wk, winfo = H.recentre(ref, t, H.STRIP_SLACK)
        assert np.array_equal(k, wk) and np.array_equal(info, winfo)
        _same_map(m, ref)
        if k.any():
            moves.append(tuple(k))

    try:
        out = H.run_strip(O, scene, lambda k, pts, nr: ctx.icp_vgicp(pts, m, nr, params=p), put, recentre)
        print("seed %d: worst |R| %.3e |t| %.3e, window %s after %d moves, %d voxels of %d mapped points" % (
            seed, max(e[2] for e in out), max(e[3] for e in out), m.window(), len(moves), len(ref.lin), ref.mapped))
        assert all(r["converged"] for _, r, _, _, _ in out)
        assert max(e[2] for e in out) <= STRIP_BAR and max(e[3] for e in out) <= STRIP_BAR
        assert m.window()[0] >= 28 and len(moves) >= 9 and np.array_equal(m.info()[2:5], [33, 33, 33])
    finally:
        m.close()
