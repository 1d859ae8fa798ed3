"""The device's KSS front end against the reference's own classes, compiled (tests/golden/ref_front.npz).

The records were written by oracle/_ref/kss_ref_front -- the reference's initRegistration_KSS and PCR_QM compiled
untouched behind oracle/ref_front.cpp -- so nothing here depends on a reading of the reference: neither the oracle nor a
numpy restatement is consulted.  Only the fixture is read; the reference tree and the binary need not exist.

Bars: f64 reductions at the suite's REL (tree against serial summation); the pose arithmetic bit for bit, as
test_gpu_parity.py::test_pose_apply_bit_exact; the error volume within 1e-13 relative, as test_gpu_refmath.py --
tests/test_ref_front_host.py shows that no two unequal entries of a 5^3 window of a recorded volume are closer than
1e-10, so that bar cannot move the arg-min or an angleList entry."""
import numpy as np
import pytest

import ref_front as RF
from test_gpu_parity import REL, _close

pytestmark = pytest.mark.gpu

FRONT, QM = RF.load_fixture()


@pytest.mark.parametrize("name", list(FRONT))
def test_preshape_stats_match_compiled_reference(ctx, name):
    S, T, _, rec = FRONT[name]
    cS, rS = ctx.preshape_stats(S)
    cT, rT = ctx.preshape_stats(T)
    st = rec["stats"]
    assert _close(cT, st[0:3])
    assert _close(rT / rS, st[6])
    bound = REL * np.maximum(1.0, np.maximum(np.abs(cT), np.abs(cS)))
    assert (np.abs((cT - cS) - st[3:6]) <= bound).all(), np.abs((cT - cS) - st[3:6]) / bound


@pytest.mark.parametrize("name", list(FRONT))
def test_pose_apply_reproduces_compiled_reference_bit_for_bit(ctx, name):
    S, _, _, rec = FRONT[name]
    st = rec["stats"]

    def posed(angle):
        return ctx.pose_apply(S, ctx.make_pose(st[3:6], st[0:3], st[6], angle))

    assert np.array_equal(posed([0.0, 0.0, 0.0]), rec["preshaped"])
    assert np.array_equal(posed(rec["angle"]), rec["posed"])
    assert len(rec["posed_list"]) == 3
    for a, want in zip(rec["angle_list"], rec["posed_list"]):
        assert np.array_equal(posed(a), want)


@pytest.mark.parametrize("name", list(FRONT))
def test_rotation_search_matches_compiled_reference(ctx, pkg, name):
    _, T, step, rec = FRONT[name]
    vol = rec["value"]
    err = ctx.rotation_search(rec["preshaped"], T, step)
    assert err.shape == (int(rec["g"]),) * 3 == vol.shape
    assert (np.abs(err - vol) <= 1e-13 * np.abs(vol)).all(), (np.abs(err - vol) / np.where(vol == 0, 1.0, np.abs(vol))).max()
    best, alist = pkg.rotation_candidates(err, step)
    assert np.array_equal(best, rec["angle"])
    assert np.array_equal(alist, rec["angle_list"])


@pytest.mark.parametrize("name", list(FRONT) + list(QM))
def test_pcr_qm_matches_compiled_reference(ctx, name):
    if name in FRONT:
        A, T, want = FRONT[name][3]["posed"], FRONT[name][1], FRONT[name][3]["qm"]
    else:
        A, T, want = QM[name]
    assert _close(ctx.pcr_qm(A, T), want)


@pytest.mark.parametrize("name", list(FRONT))
def test_register_front_end_matches_compiled_reference(ctx, name):
    """grid, n_angle_list, scale and the angle against the record.  register() reports the angle it went on with: the
    recorded arg-min, or -- when E_d_init sent it through the angleList (KSS_ICP.hpp:99-120, an ICP decision the compiled
    front end takes no part in) -- the recorded angleList entry of the index it reports."""
    S, T, step, rec = FRONT[name]
    got = ctx.register(S, T, S, step, 1000)
    assert got["grid"] == int(rec["g"])
    assert got["n_angle_list"] == len(rec["angle_list"])
    assert _close(got["scale"], rec["stats"][6])
    want = rec["angle_list"][got["angle_index"]] if got["used_angle_list"] else rec["angle"]
    assert np.array_equal(got["angle"], want)
