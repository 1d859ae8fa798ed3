"""CPU tests of similarity ICP's host side (include/kssicp.h at kss_icp_sim): kss_sim_from_sums against numpy's own
SVD with Umeyama's scale, the rigid anchor bit for bit, the clamp on both sides, the degenerate records, the argument checks."""
import ctypes as C

import numpy as np

import sim_ref as SR

F32, F64 = np.float32, np.float64


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == F64 else np.uint32)


def _record(P, Q):
    """The KSS_NSUMS record of the correspondences P[i] -> Q[i] (float32 clouds, every one kept)."""
    n = len(P)
    d2 = ((P.astype(F64) - Q.astype(F64)) ** 2).sum(1).astype(F32)
    return SR.point_sums(P, Q, np.arange(n), np.ones(n, bool), d2)


def _set(pkg, seed, scale, noise=1e-3):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(10, 2000))
    P = rng.normal(size=(n, 3)) * rng.uniform(0.3, 2.0, 3) + rng.uniform(-1, 1, 3)
    R = pkg.synth.rot_axis_angle(rng.normal(size=3), rng.uniform(0, np.pi))
    t = rng.uniform(-1, 1, 3)
    Q = scale * (P @ R.T) + t + noise * rng.normal(size=(n, 3))
    return P.astype(F32), Q.astype(F32), R, t


SCALES = [0.5, 0.7, 0.9, 1.0, 1.1, 1.5, 2.0]


def test_solve_matches_numpy(pkg):
    # T: the bar at which test_abi.py and test_p2l_host.py compare kss_rigid_from_sums / kss_rigid_from_p2l_sums with numpy (1e-6).
    # s_k is an f64 quotient of f64 sums of O(1) terms (the singular values of a 3 x 3 matrix and a variance without cancellation
    # beyond |mu|^2 / var < 1e2 here): two SVD algorithms agree to a few hundred ulp, 1e-12 relative leaves 10x on that.
    for seed in range(40):
        scale = SCALES[seed % len(SCALES)]
        P, Q, R, t = _set(pkg, seed, scale)
        s = _record(P, Q)
        T, sk, rc = pkg.sim_from_sums(s, 0.25, 4.0)
        Tn, Cn, skn, deg = SR.solve(s, 0.25, 4.0)
        assert rc == 0 and not deg
        assert abs(sk - skn) <= 1e-12 * skn
        assert np.abs(T.astype(F64) - Tn.astype(F64)).max() <= 1e-6
        assert np.array_equal(T[3], np.array([0, 0, 0, 1], F32))
        # and both recover the similarity the set was made with (noise 1e-3 over >= 10 points)
        assert abs(sk - scale) <= 5e-3 * scale
        assert np.abs(T[:3, :3].astype(F64) - scale * R).max() <= 5e-3 and np.abs(T[:3, 3] - t).max() <= 1e-2


def test_rigid_anchor_bit_for_bit(pkg):
    for seed in range(40):
        P, Q, _, _ = _set(pkg, 100 + seed, SCALES[seed % len(SCALES)])
        s = _record(P, Q)
        T, sk, rc = pkg.sim_from_sums(s, 1.0, 1.0)
        assert rc == 0 and sk == 1.0
        s20 = s.copy()
        s20[17] = 0.0       # kss_rigid_from_sums does not read it
        for rec in (s, s20):
            assert np.array_equal(_bits(T), _bits(pkg.rigid_from_sums(rec)))
    # a reflection-prone (planar) set takes the sgn branch on both sides
    rng = np.random.default_rng(7)
    P = rng.normal(size=(200, 3)); P[:, 2] = 0
    R = pkg.synth.rot_axis_angle([1, 2, 3], 0.7)
    s = _record(P.astype(F32), (P @ R.T).astype(F32))
    T, sk, rc = pkg.sim_from_sums(s, 1.0, 1.0)
    assert rc == 0 and np.array_equal(_bits(T), _bits(pkg.rigid_from_sums(s)))


def test_clamp_both_sides(pkg):
    for seed, scale, lo, hi in [(1, 1.5, 0.5, 1.2), (2, 0.6, 0.8, 2.0), (3, 2.0, 1.0, 1.0 + 2.0 ** -40), (4, 0.5, 0.999, 1.0)]:
        P, Q, _, _ = _set(pkg, 200 + seed, scale)
        s = _record(P, Q)
        T, sk, rc = pkg.sim_from_sums(s, lo, hi)
        bound = hi if scale > hi else lo
        assert rc == 0 and sk == bound                      # the bound itself, not a value near it
        free, sk_free, _ = pkg.sim_from_sums(s, 0.01, 100.0)
        assert (sk_free > hi) if scale > hi else (sk_free < lo)
        # the rotation is the free one's, the scale the bound's, and t is consistent with it: t = mu_d - s_k R mu_s
        Rf = free[:3, :3].astype(F64) / sk_free
        assert np.abs(T[:3, :3].astype(F64) - sk * Rf).max() <= 1e-6
        mu_s, mu_d = s[1:4] / s[0], s[4:7] / s[0]
        assert np.abs(T[:3, 3].astype(F64) - (mu_d - sk * (Rf @ mu_s))).max() <= 1e-6
        Tn, _, skn, _ = SR.solve(s, lo, hi)
        assert skn == sk and np.abs(T.astype(F64) - Tn.astype(F64)).max() <= 1e-6


def test_degenerate_records(pkg):
    eye = np.eye(4, dtype=F32)
    # all kept sources equal (dyadic coordinates: every sum is exact, var is exactly 0)
    P = np.tile(np.array([0.5, 0.25, -0.75], F32), (128, 1))
    Q = np.random.default_rng(0).normal(size=(128, 3)).astype(F32)
    T, sk, rc = pkg.sim_from_sums(_record(P, Q), 0.5, 2.0)
    assert rc == pkg.ERR_DEGENERATE and np.array_equal(T, eye) and sk == 1.0
    # a NaN record, a NaN in one slot, an empty record
    good = _record(*_set(pkg, 5, 1.1)[:2])
    nan1 = good.copy(); nan1[17] = np.nan
    nan2 = good.copy(); nan2[9] = np.nan
    for rec in (np.full(20, np.nan), nan1, nan2, np.zeros(20)):
        T, sk, rc = pkg.sim_from_sums(rec, 0.5, 2.0)
        assert rc == pkg.ERR_DEGENERATE and np.array_equal(T, eye) and sk == 1.0
        assert SR.solve(rec, 0.5, 2.0)[3]


def test_argument_checks(pkg):
    L = pkg.load_library()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    s, T, sk = _record(*_set(pkg, 9, 1.0)[:2]), np.zeros(16, F32), C.c_double(0)
    assert L.kss_sim_from_sums(None, 0.5, 2.0, vp(T), C.byref(sk)) == -1
    assert L.kss_sim_from_sums(vp(s), 0.5, 2.0, None, C.byref(sk)) == -1
    assert L.kss_sim_from_sums(vp(s), 0.5, 2.0, vp(T), None) == -1
    for lo, hi in ((0.0, 2.0), (-1.0, 2.0), (2.0, 1.0), (float("nan"), 2.0), (0.5, float("nan"))):
        assert L.kss_sim_from_sums(vp(s), lo, hi, vp(T), C.byref(sk)) == -1
    assert L.kss_sim_default_params(None) == -1
    sp = pkg.sim_params()
    assert (sp.overlap, sp.scale_min, sp.scale_max) == (1.0, 0.5, 2.0) and not sp.trace_sim
    assert pkg.SIM_NINFO == 6
