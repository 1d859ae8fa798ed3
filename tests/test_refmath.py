"""The oracle against tests/refmath.py, an independent numpy restatement of the reference's f32 sqrt sites.

The golden vectors and almost every GPU test compare with the oracle; these tests compare the oracle itself with a
second restatement written from the reference, bit for bit, at the places where the reference narrows a squared
distance or a normal to float, takes `float sqrt(float)` and widens the result:
initRegistrationKSS.hpp:444 (error volume), Method_Octree.hpp:141 (octree resolution) and normalCompute.hpp:345-347
(renormalised PCL normals).  The constructed cases below are built so that reading those sqrt calls as f64 sqrt
gives a different answer (refmath.origin_case, refmath.paired_octree_cloud)."""
import os

import numpy as np
import pytest

import refmath as R
from conftest import GOLDEN

F32, F64 = np.float32, np.float64


# ---- initRegistrationKSS.hpp:430-450, Error_Ave -------------------------------------------------------------------
@pytest.mark.parametrize("seed,ns,nt", [(0, 300, 400), (1, 57, 911), (2, 1000, 130)])
def test_error_ave_matches_restatement_on_random_clouds(O, seed, ns, nt):
    rng = np.random.default_rng(seed)
    S = rng.normal(size=(ns, 3))
    T = rng.normal(size=(nt, 3)) * 0.8 + 0.1
    assert O.error_ave(S, T) == R.error_ave(S, T)


@pytest.mark.parametrize("seed", [3, 4, 5])
def test_error_ave_origin_case_takes_the_float_sqrt(O, seed):
    x, y, d2 = R.origin_case(seed)
    T = np.array([[x, y, 0.0], [4.0, 4.0, 4.0], [-3.0, 5.0, 1.0]], F64)
    S = np.zeros((37, 3))
    want = F64(np.sqrt(d2))
    assert R.error_ave(S, T) == want                     # n equal widened floats: the sum and the division are exact
    assert want != np.sqrt(F64(d2))
    assert O.error_ave(S, T) == want


# ---- initRegistrationKSS.hpp:222-260, the error volume --------------------------------------------------------------
def test_rotation_search_at_step_1_is_error_ave(O):
    x, y, _ = R.origin_case(6)
    rng = np.random.default_rng(7)
    S = rng.normal(size=(200, 3))
    T = np.concatenate([[[x, y, 0.0]], rng.normal(size=(250, 3))])
    r = O.rotation_search(S, T, 1)
    assert r["g"] == 1                                   # the only angle is 0: the rotation is the identity
    assert r["value"][0, 0, 0] == R.error_ave(S, T)
    z = O.rotation_search(np.zeros((9, 3)), T[:1], 1)
    assert z["value"][0, 0, 0] == F64(np.sqrt(F32(x * x + y * y)))


def test_rotation_search_matches_restated_error_volume(O):
    rng = np.random.default_rng(8)
    S = rng.normal(size=(300, 3)) * np.array([1.0, 0.6, 0.3])
    T = rng.normal(size=(400, 3)) * np.array([0.9, 0.5, 0.35])
    r = O.rotation_search(S, T, 6)
    vol = R.error_volume(S, T, 6)
    assert r["g"] == len(R.grid_angles(6)) == 6
    assert np.array_equal(r["value"], vol)
    ang = np.array(R.grid_angles(6))
    a = np.unravel_index(np.argmin(vol), vol.shape)      # :258 strict `<`: the first minimum in (i, j, k) order
    assert np.array_equal(r["angle"], ang[list(a)])


def test_golden_error_volume_matches_restatement():
    """The committed G2 volume (tests/golden/make_golden.py) is the reference's arithmetic, not only the oracle's."""
    g = np.load(os.path.join(GOLDEN, "oracle_vectors.npz"))
    vol = R.error_volume(g["g1_preshaped"], g["g1_tgt"].astype(F64), 6)
    assert np.array_equal(g["g2_value_6"], vol)


# ---- Method_Octree.hpp:110-165, the octree resolution -----------------------------------------------------------------
@pytest.mark.parametrize("seed,n", [(9, 1000), (10, 5000), (11, 81000)])
def test_octree_resolution_matches_restatement_on_random_clouds(O, seed, n):
    P = np.random.default_rng(seed).uniform(-1.0, 1.0, size=(n, 3)) * np.array([1.0, 2.0, 0.5])
    assert R.octree_kn(n) == (7 if n >= 80000 else 2)
    assert O.octree_downsample(P)[1] == R.octree_resolution(P)


def test_octree_resolution_constructed_case_takes_the_float_sqrt(O):
    P, new, old = R.paired_octree_cloud(12)
    assert new != old
    assert R.octree_resolution(P) == new
    assert O.octree_downsample(P)[1] == new


# ---- normalCompute.hpp:342-348, renormalised PCL normals ------------------------------------------------------------
def test_check_renormalised_separates_the_two_readings():
    rng = np.random.default_rng(13)
    v = rng.normal(size=(4000, 3)).astype(F32)
    v /= np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])[:, None]
    s = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    f32_reading = v.astype(F64) / s.astype(F64)[:, None]
    f64_reading = v.astype(F64) / np.sqrt((v.astype(F64) ** 2).sum(1))[:, None]
    assert len(R.check_renormalised(f32_reading)) == 0
    assert len(R.check_renormalised(f64_reading)) > 0.5 * len(v)
    assert len(R.check_renormalised(f32_reading * (1 + 2.0 ** -50))) == len(v)


def test_oracle_normals_are_renormalised_in_float(O, pkg, ref_pairs):
    for P in (pkg.synth.bumpy(4, 6000), ref_pairs[("registration", "Horse")][0]):
        n = O.normals_pcl(P, 20)
        assert np.isfinite(n).all()
        assert len(R.check_renormalised(n)) == 0
