"""The device paths of the reference's f32 sqrt sites against tests/refmath.py, not against the oracle.

initRegistrationKSS.hpp:444 (rot_search_kernel), Method_Octree.hpp:141 (kss_downsample_octree) and
normalCompute.hpp:345-347 (normals_kernel) take `float sqrt(float)` and widen the result; a kernel that reads them as
f64 sqrt stays within 1e-9 of the truth, so these tests compare bit for bit where the arithmetic allows it."""
import os

import numpy as np
import pytest

import refmath as R

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64


def _with_env(settings, fn):
    """Run fn() with the given environment variables set (None: unset), restoring the old values afterwards."""
    old = {k: os.environ.get(k) for k in settings}
    try:
        for k, v in settings.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def test_rotation_search_origin_case_is_bit_exact_at_every_padding(ctx):
    """Sources all at the origin, the nearest target at (x, y, 0): every candidate of every rotation is the widened
    sqrtf of the same f32 d2 (a sum of equal widened floats is exact in any order, and so is the division by n).
    The nearest target is the last one, next to the padding; a padded target that were not a far sentinel would
    give d2 = 0 here."""
    x, y, d2 = R.origin_case(21)
    want = F64(np.sqrt(d2))
    assert want != np.sqrt(F64(d2))
    rng = np.random.default_rng(22)
    checked = 0
    for nt in (1, 255, 256, 257, 700):
        far = rng.normal(size=(nt - 1, 3))
        far = far / np.linalg.norm(far, axis=1, keepdims=True) * rng.uniform(3.0, 6.0, size=(nt - 1, 1))
        T = np.concatenate([far, [[float(x), float(y), 0.0]]])
        for ns in (1, 127, 128, 129, 255, 256, 257, 1000):
            S = np.zeros((ns, 3))
            for nth in ("128", "256"):
                for width in ("1", "2", "4"):
                    for step in (1, 6):
                        err = _with_env({"KSS_ROT_NTH": nth, "KSS_ROT_S": width}, lambda: ctx.rotation_search(S, T, step))
                        assert err.shape == (len(R.grid_angles(step)),) * 3
                        assert (err == want).all(), (nt, ns, nth, width, step, np.unique(err))
                        checked += 1
    assert checked == 5 * 8 * 2 * 3 * 2


@pytest.mark.parametrize("seed,ns,nt", [(23, 300, 400), (24, 129, 257), (25, 1000, 255)])
def test_rotation_search_matches_restated_error_volume(ctx, pkg, seed, ns, nt):
    """Random pairs: the volume within 1e-13 relative of the restatement (tree-order summation; the f64-sqrt reading
    is ~1e-9 off), the same arg-min and the same angle / angleList from the volume."""
    rng = np.random.default_rng(seed)
    S = rng.normal(size=(ns, 3)) * np.array([1.0, 0.6, 0.3])
    T = rng.normal(size=(nt, 3)) * np.array([0.9, 0.5, 0.35]) + 0.05
    for step in (1, 6):
        vol = R.error_volume(S, T, step)
        err = ctx.rotation_search(S, T, step)
        assert err.shape == vol.shape
        assert (np.abs(err - vol) <= 1e-13 * np.abs(vol)).all(), np.abs(err / vol - 1).max()
        assert np.argmin(err) == np.argmin(vol)
        if step > 1:
            best, alist = pkg.rotation_candidates(err, step)
            rbest, ralist = pkg.rotation_candidates(vol, step)
            assert np.array_equal(best, rbest) and np.array_equal(alist, ralist)
            assert np.array_equal(best, np.array(R.grid_angles(step))[list(np.unravel_index(np.argmin(vol), vol.shape))])


@pytest.mark.parametrize("case", ["random-1000", "random-5000", "random-81000", "constructed"])
def test_octree_resolution_matches_restatement(ctx, O, case):
    """The resolution bit for bit against the restatement (the constructed cloud separates the f32 and the f64
    readings of Method_Octree.hpp:141); the selection still equal to the oracle's."""
    if case == "constructed":
        P, new, old = R.paired_octree_cloud(12)
        assert new != old
    else:
        n = int(case.split("-")[1])
        P = np.random.default_rng(n).uniform(-1.0, 1.0, size=(n, 3)) * np.array([1.0, 2.0, 0.5])
    idx, res = ctx.downsample_octree(P)
    assert res == R.octree_resolution(P)
    if case == "constructed":
        assert res == new
    oi, ores = O.octree_downsample(P)
    assert ores == res and np.array_equal(idx, oi)


def test_normals_are_renormalised_in_float(ctx, pkg, ref_pairs):
    for P in (pkg.synth.bumpy(4, 6000), ref_pairs[("registration", "Horse")][0]):
        n = ctx.normals(P, 20)
        assert np.isfinite(n).all()
        assert len(R.check_renormalised(n)) == 0
