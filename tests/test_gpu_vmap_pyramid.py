"""The voxel-map pyramid on the device (kss_vmap_coarsen, kss_vmap_coarsen_into, kss_icp_vgicp_from, kss_icp_vgicp_c2f; DESIGN.md
2.37) against the restatement in tests/vmap_pyramid_ref.py: a coarsened map is compared BIT FOR BIT in kss_vmap_read,
kss_vmap_info and kss_vmap_window, a refreshed one against a fresh one, the start-pose loop at test_gpu_vgicp.py's bars, the
ladder against the chain of calls bit for bit, and the 55 degree scene of tests/test_vmap_pyramid_host.py, where the fine map
alone is lost and the ladder is not."""
import ctypes as C

import numpy as np
import pytest

import vgicp_ref as V
import vmap_pyramid_ref as Y
import vmap_shift_ref as H
from test_vmap_pyramid_host import AXIS, FINE_LEAF, LADDER, LADDER_BAR, LOST_BAR, ladder_scene

pytestmark = pytest.mark.gpu

F32, F64, I64 = np.float32, np.float64, np.int64
KS = (2, 3, 4, 8)
LO, HI = [-1.6] * 3, [1.6] * 3


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
    assert np.array_equal(m.window(), ref.window())


def _state(m):
    lin, stats = m.read()
    return lin, stats, m.info(), m.window()


def _same_state(a, b):
    for x, y in zip(a, b):
        assert np.array_equal(_bits(x), _bits(y))


def _same_result(a, b, fitness=True):
    assert b["iterations"] == a["iterations"] and b["state"] == a["state"] and b["converged"] == a["converged"]
    for k in ("trace_Tk", "trace_sums", "T", "info"):
        if k in a or k in b:
            assert np.array_equal(_bits(b[k]), _bits(a[k])), k
    assert np.array_equal(_bits(np.array([b["last_mse"]])), _bits(np.array([a["last_mse"]])))
    if fitness:
        assert np.array_equal(_bits(np.array([b["fitness"]])), _bits(np.array([a["fitness"]])))


def _coarsen_all(m, ref, ks=KS):
    """Every k twice on the device against the restatement; the source is what it was after each call."""
    before = _state(m)
    for k in ks:
        a, b = m.coarsen(k), m.coarsen(k)
        _same_state(before, _state(m))
        want = Y.coarsen(ref, k)
        _same_map(a, want)
        _same_state(_state(a), _state(b))
        a.close(); b.close()


# ---- coarsen -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("leaf", [1e3, 0.1, 1e-2])
@pytest.mark.parametrize("nt", [1, 255, 257, 5000])
def test_coarsen_matches_restatement(pkg, ctx, nt, leaf):
    A = pkg.synth.bumpy(60 + nt % 7, nt).astype(F32)
    an = _unit(np.random.default_rng(nt), nt)
    m, ref = ctx.vmap(A, leaf, normals=an), H.create(A, an, leaf)
    _same_map(m, ref)
    if leaf == 1e3:
        assert len(ref.lin) == 1
    _coarsen_all(m, ref)
    m.close()


@pytest.mark.parametrize("base", [(-3, 1, 5), (7, -8, 0)])
def test_coarsen_shifted_map(pkg, ctx, base):
    A = pkg.synth.bumpy(11, 5000).astype(F32)
    an = _unit(np.random.default_rng(11), 5000)
    m, ref = ctx.vmap(A, 2.0 ** -4, normals=an), H.create(A, an, 2.0 ** -4)
    assert np.array_equal(m.shift(base), H.shift(ref, base))
    _same_map(m, ref)
    assert 0 < len(ref.lin) and np.array_equal(ref.window(), base)
    _coarsen_all(m, ref)
    for k in KS:                                      # a negative base is divided towards minus infinity
        assert np.array_equal(Y.coarsen(ref, k).window(), np.floor_divide(np.array(base), k))
    m.close()


def test_coarsen_empty_box_map(pkg, ctx):
    m, ref = ctx.vmap_box(LO, HI, 0.1), H.box(LO, HI, 0.1)
    for k in KS:
        c, want = m.coarsen(k), Y.coarsen(ref, k)
        _same_map(c, want)
        assert c.info()[0] == 0 and c.info()[1] == 0
        A = pkg.synth.bumpy(12, 300).astype(F32)      # and it is a map an insert fills as it fills a box map
        an = _unit(np.random.default_rng(12), 300)
        assert np.array_equal(c.insert(A, an), H.insert(want, A, an))
        _same_map(c, want)
        c.close()
    m.close()


def test_coarsen_three_inserts_against_one(pkg, ctx):
    A = pkg.synth.bumpy(13, 3000).astype(F32)
    an = _unit(np.random.default_rng(13), 3000)
    A[::97, 1] = np.nan                               # left out by the insert
    an[5::131, 2] = np.inf
    A[7::211] += F32(50.0)                            # outside the box
    a, b, ref = ctx.vmap_box(LO, HI, 0.1), ctx.vmap_box(LO, HI, 0.1), H.box(LO, HI, 0.1)
    for lo, hi in ((0, 900), (900, 901), (901, 3000)):
        a.insert(A[lo:hi], an[lo:hi])
    b.insert(A, an)
    H.insert(ref, A, an)
    assert 0 < ref.mapped < 3000
    _same_map(a, ref); _same_map(b, ref)
    for k in KS:
        ca, cb = a.coarsen(k), b.coarsen(k)
        _same_map(ca, Y.coarsen(ref, k))
        _same_state(_state(ca), _state(cb))
        ca.close(); cb.close()
    a.close(); b.close()


# ---- the result is a full map ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fine_pair(pkg, ctx):
    A = pkg.synth.bumpy(21, 5000).astype(F32)
    an = _unit(np.random.default_rng(21), 5000)
    m, ref = ctx.vmap(A, 0.05, normals=an), H.create(A, an, 0.05)
    yield A, an, m, ref
    m.close()


@pytest.mark.parametrize("k", KS)
def test_vgicp_sums_against_a_coarse_map(pkg, ctx, fine_pair, k):
    """test_vgicp_sums_match_restatement's bar, on the coarse map's own inv'."""
    _, _, m, ref = fine_pair
    c, cref = m.coarsen(k), Y.coarsen(ref, k)
    n = 2000
    rng = np.random.default_rng(k)
    src = (pkg.synth.bumpy(100 + k, n) + rng.normal(scale=0.01, size=(n, 3))).astype(F32)
    src[rng.random(n) < 0.1] += F32(100.0)
    sn = _unit(rng, n)
    Rn = pkg.synth.rot_axis_angle(rng.normal(size=3), 0.8).astype(F32)
    got = ctx.vgicp_sums(src, sn, c, 0.05, Rn=Rn)
    want, absc = H.sums(src, sn, cref, 0.05, Rn=Rn, eps=1e-3)
    print("k %d: kept %d of %d, max |got - ref| / sum|term| %.2e" % (k, int(got[0]), n, (np.abs(got - want) / np.maximum(absc, 1e-300)).max()))
    assert 0 < got[0] < n and got[0] == want[0]
    assert np.all(np.abs(got - want) <= 1e-12 * absc)
    c.close()


@pytest.mark.parametrize("k", KS)
def test_insert_into_and_shift_of_a_coarse_map(pkg, ctx, fine_pair, k):
    A, an, m, ref = fine_pair
    c, cref = m.coarsen(k), Y.coarsen(ref, k)
    B = (pkg.synth.bumpy(22, 1500) * 1.05).astype(F32)
    bn = _unit(np.random.default_rng(22), 1500)
    T = np.eye(4, dtype=F32)
    T[:3, :3] = pkg.synth.rot_axis_angle(AXIS, 0.2).astype(F32)
    T[:3, 3] = (0.03, -0.02, 0.01)
    assert np.array_equal(c.insert(B, bn, T), H.insert(cref, B, bn, T))
    _same_map(c, cref)
    assert np.array_equal(c.shift((1, -1, 0)), H.shift(cref, (1, -1, 0)))
    _same_map(c, cref)
    assert np.array_equal(c.insert(A[:700], an[:700]), H.insert(cref, A[:700], an[:700]))
    _same_map(c, cref)
    c.close()


def test_coarse_map_survives_its_source(pkg, ctx):
    A = pkg.synth.bumpy(23, 2000).astype(F32)
    an = _unit(np.random.default_rng(23), 2000)
    m, ref = ctx.vmap(A, 0.05, normals=an), H.create(A, an, 0.05)
    c, cref = m.coarsen(4), Y.coarsen(ref, 4)
    m.close()
    junk = ctx.vmap(A[:1500] * F32(1.3), 0.04, normals=an[:1500])   # the allocator may hand the source's memory out again
    _same_map(c, cref)
    got = ctx.vgicp_sums(A, an, c, 1.0)
    want, absc = H.sums(A, an, cref, 1.0)
    assert got[0] == want[0] > 0 and np.all(np.abs(got - want) <= 1e-12 * absc)
    junk.close(); c.close()


# ---- coarsen_into ------------------------------------------------------------------------------------------------------------
def _refresh(m, ref, dst, k):
    """dst refreshed from m: equal to the restatement and to a fresh coarsen, bit for bit."""
    m.coarsen_into(dst, k)
    _same_map(dst, Y.coarsen(ref, k))
    fresh = m.coarsen(k)
    _same_state(_state(dst), _state(fresh))
    fresh.close()


@pytest.mark.parametrize("k", [2, 4])
def test_coarsen_into_after_insert_and_recentre(pkg, ctx, k):
    scans = [(pkg.synth.bumpy(30 + i, 1500) * (0.8 + 0.1 * i) + [0.1 * i, 0, 0]).astype(F32) for i in range(4)]
    ns = [_unit(np.random.default_rng(30 + i), 1500) for i in range(4)]
    m, ref = ctx.vmap_box(LO, HI, 0.05), H.box(LO, HI, 0.05)
    m.insert(scans[0], ns[0]); H.insert(ref, scans[0], ns[0])
    dst = m.coarsen(k)
    _same_map(dst, Y.coarsen(ref, k))
    for i in (1, 2):                                  # the scan-to-map loop's step: insert, recentre, refresh
        assert np.array_equal(m.insert(scans[i], ns[i]), H.insert(ref, scans[i], ns[i]))
        kk, _ = m.recentre([0.25 * i, -0.1 * i, 0.05], 1)
        assert np.array_equal(kk, H.recentre(ref, [0.25 * i, -0.1 * i, 0.05], 1)[0]) and kk.any()
        _same_map(m, ref)
        _refresh(m, ref, dst, k)
    # ... and behind an insert into and a shift of dst itself
    dref = Y.coarsen(ref, k)
    assert np.array_equal(dst.insert(scans[3], ns[3]), H.insert(dref, scans[3], ns[3]))
    assert np.array_equal(dst.shift((2, 0, -1)), H.shift(dref, (2, 0, -1)))
    _same_map(dst, dref)
    _refresh(m, ref, dst, k)
    _refresh(m, ref, dst, k)                          # and once more, with nothing changed
    dst.close(); m.close()


def test_coarsen_into_outgrows_the_records(pkg, ctx):
    A = pkg.synth.bumpy(40, 6000).astype(F32)
    an = _unit(np.random.default_rng(40), 6000)
    m, ref = ctx.vmap_box(LO, HI, 0.05), H.box(LO, HI, 0.05)
    m.insert(A[:3], an[:3]); H.insert(ref, A[:3], an[:3])
    dst = m.coarsen(2)
    n0 = int(dst.info()[1])
    m.insert(A, an); H.insert(ref, A, an)
    _refresh(m, ref, dst, 2)
    assert n0 <= 3 and dst.info()[1] > 50 * n0        # far beyond any headroom
    m.shift((100, 0, 0)); H.shift(ref, (100, 0, 0))   # and back to nothing: an empty map
    assert len(ref.lin) == 0
    _refresh(m, ref, dst, 2)
    assert dst.info()[0] == 0 and dst.info()[1] == 0
    m.close(); dst.close()


def test_coarsen_refusals_change_nothing(pkg, ctx):
    L = pkg.load_library()
    A = pkg.synth.bumpy(41, 2000).astype(F32)
    an = _unit(np.random.default_rng(41), 2000)
    m, ref = ctx.vmap(A, 0.05, normals=an), H.create(A, an, 0.05)
    other_fine = ctx.vmap(A[:1000] * F32(0.7), 0.05, normals=an[:1000])
    dst, d4, d_other = m.coarsen(2), m.coarsen(4), other_fine.coarsen(2)
    assert not np.array_equal(d_other.info()[2:5], dst.info()[2:5])
    sm, sd, s4, so = _state(m), _state(dst), _state(d4), _state(d_other)
    foreign_ctx = pkg.Context(0)
    foreign = foreign_ctx.vmap(A, 0.05, normals=an)
    fdst = foreign.coarsen(2)
    dead = m.coarsen(2)
    dead_h = C.c_void_p(dead.h.value)
    dead.close()
    out = C.c_void_p(0x77)

    def refused(rc):
        assert rc == -1
        _same_state(sm, _state(m)); _same_state(sd, _state(dst)); _same_state(s4, _state(d4)); _same_state(so, _state(d_other))

    for k in (1, 0, -2, 9, 1 << 20):
        refused(L.kss_vmap_coarsen(ctx.h, m.h, k, C.byref(out)))
        assert out.value is None                      # (*out is cleared)
        out = C.c_void_p(0x77)
        refused(L.kss_vmap_coarsen_into(ctx.h, m.h, k, dst.h))
    refused(L.kss_vmap_coarsen(ctx.h, m.h, 2, None))
    for h in (None, foreign.h, dead_h):
        refused(L.kss_vmap_coarsen(ctx.h, h, 2, C.byref(out)))
        refused(L.kss_vmap_coarsen_into(ctx.h, h, 2, dst.h))
    for h in (None, fdst.h, dead_h):
        refused(L.kss_vmap_coarsen_into(ctx.h, m.h, 2, h))
    refused(L.kss_vmap_coarsen_into(ctx.h, m.h, 2, d4.h))          # a dst of another k
    refused(L.kss_vmap_coarsen_into(ctx.h, m.h, 4, dst.h))
    refused(L.kss_vmap_coarsen_into(ctx.h, m.h, 2, d_other.h))     # another fine map's shape
    refused(L.kss_vmap_coarsen_into(ctx.h, m.h, 2, m.h))           # dst is map
    refused(L.kss_vmap_coarsen_into(None, m.h, 2, dst.h))
    with pytest.raises(pkg.KssError):
        m.coarsen(9)
    with pytest.raises(pkg.KssError):
        m.coarsen_into(d4, 2)
    _refresh(m, ref, dst, 2)                                       # a good call behind the refusals
    _refresh(m, ref, d4, 4)
    for x in (fdst, foreign):
        x.close()
    foreign_ctx.close()
    for x in (dst, d4, d_other, other_fine, m):
        x.close()


# ---- icp_vgicp_from ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene25(pkg, ctx):
    src, tgt, R_true, t_true = V.halves_pair(pkg.synth, 8, 4000, 25.0, axis=AXIS)
    sn, tn = _normals(ctx, src), _normals(ctx, tgt)
    T0 = np.eye(4, dtype=F32)                         # 15 of the 25 degrees about the scene's axis, and its translation
    R0 = pkg.synth.rot_axis_angle(AXIS, np.deg2rad(15.0)).T
    T0[:3, :3] = R0.astype(F32)
    T0[:3, 3] = (-R0 @ np.array([0.02, -0.01, 0.03])).astype(F32)
    return src, sn, tgt, tn, R_true, t_true, T0


def test_from_null_and_identity_are_icp_vgicp(pkg, ctx, scene25):
    src, sn, tgt, tn, _, _, _ = scene25
    m = ctx.vmap(tgt, 0.1, normals=tn)
    p = ctx.icp_params(max_iterations=60)
    a = ctx.icp_vgicp(src, m, sn, params=p, trace_cap=64)
    assert a["iterations"] >= 3
    _same_result(a, ctx.icp_vgicp_from(src, m, None, sn, params=p, trace_cap=64))
    _same_result(a, ctx.icp_vgicp_from(src, m, np.eye(4), sn, params=p, trace_cap=64))
    b = ctx.icp_vgicp(src, m, params=p)               # computed normals too
    _same_result(b, ctx.icp_vgicp_from(src, m, np.eye(4), params=p))
    m.close()


def test_from_matches_restatement(pkg, ctx, O, scene25):
    """test_icp_vgicp_matches_restatement's bars.  Pass 0 works on T0 * src, the same float expression on both sides, so its cells
    are the restatement's and its record agrees within the sums tolerance."""
    src, sn, tgt, tn, R_true, t_true, T0 = scene25
    m, vm = ctx.vmap(tgt, 0.1, normals=tn), H.create(tgt, tn, 0.1)
    _same_map(m, vm)
    got = ctx.icp_vgicp_from(src, m, T0, sn, params=ctx.icp_params(max_iterations=60), trace_cap=64)
    ref = Y.icp_vgicp_from(O, src, sn, vm, T0, max_iterations=60)
    assert got["iterations"] == ref["iterations"] >= 1
    assert got["state"] == ref["state"] and got["converged"] == ref["converged"]
    s0, r0 = got["trace_sums"][0], ref["trace_sums"][0]
    _, a0 = H.sums(O.transform_points_f32(T0, src), sn, vm, 1.0, Rn=T0[:3, :3])
    eR, et = V.errors(got["T"], R_true, t_true)
    print("%d passes, state %d, |trace_Tk| %.2e  |T| %.2e  |fitness| %.2e rel  first sums %.2e of sum|term|, errors %.2e %.2e" % (
        got["iterations"], got["state"], np.abs(got["trace_Tk"] - ref["trace_Tk"]).max(), np.abs(got["T"] - ref["T"]).max(),
        abs(got["fitness"] - ref["fitness"]) / ref["fitness"], (np.abs(s0 - r0) / np.maximum(a0, 1e-300)).max(), eR, et))
    assert s0[0] == r0[0]
    assert np.all(np.abs(s0 - r0) <= 1e-12 * a0)
    assert np.abs(got["trace_Tk"] - ref["trace_Tk"]).max() <= 1e-6
    assert np.abs(got["T"] - ref["T"]).max() <= 5e-6
    assert abs(got["fitness"] - ref["fitness"]) <= 1e-9 * ref["fitness"]
    assert got["info"][1] == len(src) and got["info"][3] == len(vm.lin)
    assert got["converged"] and eR <= 1e-3 and et <= 1e-3          # T includes the start pose
    # the _dev entry is the host entry
    import torch
    ds, dn = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (src, sn))
    torch.cuda.synchronize()
    res, info = ctx.icp_vgicp_from_dev(ds.data_ptr(), len(src), dn.data_ptr(), m, T0, ctx.icp_params(max_iterations=60))
    assert np.array_equal(_bits(res.matrix()), _bits(got["T"])) and res.iterations == got["iterations"]
    assert np.array_equal(_bits(info), _bits(got["info"])) and res.fitness == got["fitness"]
    m.close()


def test_from_refuses_a_non_finite_pose(pkg, ctx, scene25):
    src, sn, tgt, tn, _, _, T0 = scene25
    m = ctx.vmap(tgt, 0.1, normals=tn)
    good = ctx.icp_vgicp_from(src, m, T0, sn)
    for at, v in (((0, 0), np.nan), ((2, 3), np.inf), ((3, 3), -np.inf), ((3, 0), np.nan)):
        bad = T0.copy()
        bad[at] = v
        with pytest.raises(pkg.KssError):
            ctx.icp_vgicp_from(src, m, bad, sn)
        with pytest.raises(pkg.KssError):
            ctx.icp_vgicp_c2f(src, [m], bad, sn)
    _same_result(good, ctx.icp_vgicp_from(src, m, T0, sn))
    m.close()


# ---- icp_vgicp_c2f -----------------------------------------------------------------------------------------------------------
def _chain(ctx, src, maps, T0, sn, p_last, p_quiet, trace_cap=0):
    out, A = [], T0
    for l, m in enumerate(maps):
        last = l == len(maps) - 1
        r = ctx.icp_vgicp_from(src, m, A, sn, params=p_last if last else p_quiet, trace_cap=trace_cap if last else 0)
        out.append(r)
        A = r["T"]
    return out


@pytest.mark.parametrize("given", [True, False])
def test_c2f_is_the_chain_of_calls(pkg, ctx, scene25, given):
    src, sn, tgt, tn, _, _, T0 = scene25
    m = ctx.vmap(tgt, 0.05, normals=tn)
    maps = [m.coarsen(4), m.coarsen(2), m]
    p, quiet = ctx.icp_params(max_iterations=60), ctx.icp_params(max_iterations=60, compute_fitness=0)
    normals = sn if given else None
    for start in (None, T0):
        got = ctx.icp_vgicp_c2f(src, maps, start, normals, params=p, trace_cap=64)
        want = _chain(ctx, src, maps, start, normals, p, quiet, 64)
        assert len(got) == 3 and [r["iterations"] >= 1 for r in got] == [True] * 3
        for l in range(3):
            _same_result(want[l], got[l])
        assert "trace_Tk" in got[2] and "trace_Tk" not in got[0] and len(got[2]["trace_Tk"]) == got[2]["iterations"]
        assert got[0]["fitness"] == 0.0 and got[1]["fitness"] == 0.0 and got[2]["fitness"] > 0.0
        _same_result(got[2], ctx.icp_vgicp_c2f(src, maps, start, normals, params=p, trace_cap=64)[2])   # deterministic
    # one level is icp_vgicp_from
    one = ctx.icp_vgicp_c2f(src, [m], T0, normals, params=p, trace_cap=64)
    assert len(one) == 1
    _same_result(ctx.icp_vgicp_from(src, m, T0, normals, params=p, trace_cap=64), one[0])
    if given:                                         # the _dev entry is the host entry
        import torch
        ds, dn = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (src, sn))
        torch.cuda.synchronize()
        got = ctx.icp_vgicp_c2f(src, maps, T0, sn, params=p)
        res, info = ctx.icp_vgicp_c2f_dev(ds.data_ptr(), len(src), dn.data_ptr(), maps, T0, p)
        for l in range(3):
            assert np.array_equal(_bits(res[l].matrix()), _bits(got[l]["T"])) and res[l].iterations == got[l]["iterations"]
            assert res[l].pair_id == l and np.array_equal(_bits(info[l]), _bits(got[l]["info"]))
    for x in maps[:2]:
        x.close()
    m.close()


@pytest.mark.parametrize("seed", [8, 3, 5])
def test_c2f_ladder_scene(pkg, ctx, O, seed):
    """tests/test_vmap_pyramid_host.py's scene with device-coarsened maps: the restatement's passes and states level by level, the
    host test's bars at the end."""
    src, sn, tgt, tn, R_true, t_true = ladder_scene(pkg.synth, O, seed)
    m, vm = ctx.vmap(tgt, FINE_LEAF, normals=tn), H.create(tgt, tn, FINE_LEAF)
    maps, vms = [m.coarsen(k) for k in LADDER] + [m], Y.ladder(vm, LADDER)
    for a, b in zip(maps, vms):
        _same_map(a, b)
    p = ctx.icp_params(max_iterations=200)
    got = ctx.icp_vgicp_c2f(src, maps, None, sn, params=p)
    ref = Y.icp_vgicp_c2f(O, src, sn, vms, max_iterations=200)
    alone = ctx.icp_vgicp(src, m, sn, params=p)
    eR, et = V.errors(got[-1]["T"], R_true, t_true)
    eR0, et0 = V.errors(alone["T"], R_true, t_true)
    print("seed %d: fine map alone %.2e %.2e (%d passes)   ladder %.2e %.2e  passes %s / %s  states %s / %s  |T - ref| %.2e" % (
        seed, eR0, et0, alone["iterations"], eR, et, [r["iterations"] for r in got], [r["iterations"] for r in ref],
        [r["state"] for r in got], [r["state"] for r in ref], np.abs(got[-1]["T"] - ref[-1]["T"]).max()))
    assert [r["iterations"] for r in got] == [r["iterations"] for r in ref]
    assert [r["state"] for r in got] == [r["state"] for r in ref]
    assert eR <= LADDER_BAR and et <= LADDER_BAR
    assert eR0 >= LOST_BAR
    for x in maps[:-1]:
        x.close()
    m.close()


def test_c2f_refusals_change_nothing(pkg, ctx, scene25):
    L = pkg.load_library()
    src, sn, tgt, tn, _, _, T0 = scene25
    m = ctx.vmap(tgt, 0.05, normals=tn)
    c2 = m.coarsen(2)
    p = ctx.icp_params(max_iterations=60)
    good = ctx.icp_vgicp_c2f(src, [c2, m], T0, sn, params=p)
    dead = m.coarsen(4)
    stale = pkg.VoxelMap(ctx, C.c_void_p(dead.h.value))
    dead.close()
    other = pkg.Context(0)
    foreign = other.vmap(tgt, 0.05, normals=tn)
    for maps in ([], [m] * 9, [c2, None], [None, m], [c2, stale], [foreign, m]):
        with pytest.raises(pkg.KssError):
            ctx.icp_vgicp_c2f(src, maps, T0, sn, params=p)
    with pytest.raises(pkg.KssError):                 # what kss_icp_vgicp refuses
        ctx.icp_vgicp_c2f(src, [c2, m], T0, sn, params=p, gp=pkg.gicp_params(epsilon=0.0))
    gp = pkg.gicp_params()
    s = np.ascontiguousarray(src)
    res = (pkg.IcpResult * 2)()
    lv = (C.c_void_p * 2)(c2.h, m.h)
    ps, pl, pr = s.ctypes.data_as(C.c_void_p), C.cast(lv, C.c_void_p), C.cast(res, C.c_void_p)
    assert L.kss_icp_vgicp_c2f(ctx.h, ps, len(s), None, None, 2, None, C.byref(p), C.byref(gp), pr, None) == -1    # NULL maps
    assert L.kss_icp_vgicp_c2f(ctx.h, ps, len(s), None, pl, 2, None, C.byref(p), C.byref(gp), None, None) == -1    # NULL results
    assert L.kss_icp_vgicp_c2f(ctx.h, None, len(s), None, pl, 2, None, C.byref(p), C.byref(gp), pr, None) == -1    # NULL src
    assert L.kss_icp_vgicp_c2f(ctx.h, ps, 0, None, pl, 2, None, C.byref(p), C.byref(gp), pr, None) == -1           # no point
    assert L.kss_icp_vgicp_c2f(ctx.h, ps, len(s), None, pl, 2, None, None, C.byref(gp), pr, None) == -1            # NULL p
    assert L.kss_icp_vgicp_c2f(None, ps, len(s), None, pl, 2, None, C.byref(p), C.byref(gp), pr, None) == -1       # NULL ctx
    again = ctx.icp_vgicp_c2f(src, [c2, m], T0, sn, params=p)
    for a, b in zip(good, again):
        _same_result(a, b)
    foreign.close(); other.close()
    c2.close(); m.close()
