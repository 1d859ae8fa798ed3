"""The oracle's KSS front end against the reference's own classes, compiled (CPU).

tests/golden/ref_front.npz holds what oracle/_ref/kss_ref_front -- the reference's initRegistration_KSS and PCR_QM behind
oracle/ref_front.cpp and the stand-in PCL headers of oracle/ref_shim -- computed on six pairs and five PCR_QM inputs.
Every other parity test compares with oracle/kss_oracle.c or a numpy restatement, both written from a reading of the
reference; here a compiler has settled the `for (double i = 0; i < 6.3; i += 6.3 / step)` trip counts, the sqrt(float)
overload, the order of shift and scale, and the strict comparisons of the arg-min and of the 5^3 local minimum.

The bar is bit equality: oracle and reference do the same IEEE operations in the same order on one thread."""
import numpy as np
import pytest

import ref_front as RF

FRONT, QM = RF.load_fixture()


def _assert_same_record(got, want, where):
    assert set(got) == set(want) == set(RF.FIELDS)
    for k in RF.FIELDS:
        assert RF.same_bits(np.asarray(got[k], np.float64), np.asarray(want[k], np.float64)), (where, k)


def test_fixture_holds_the_cases_of_the_issue():
    assert list(FRONT) == ["c1", "c2", "c3", "c4", "c5", "c6"]
    assert [(len(S), len(T), step) for S, T, step, _ in FRONT.values()] == [
        (400, 500, 8.0), (257, 300, 6.0), (128, 129, 12.0), (400, 450, 8.0), (200, 255, 16.0), (129, 1, 6.0)]
    assert [(len(A), len(T)) for A, T, _ in QM.values()] == list(RF.QM_SIZES)
    # the loop trip counts, as compiled: 6.3 / step accumulated `step` times stays below 6.3 for step 8 and 16 only
    assert [int(rec["g"]) for _, _, _, rec in FRONT.values()] == [9, 6, 12, 9, 17, 6]
    for _, _, _, rec in FRONT.values():
        assert all(np.isfinite(v).all() for v in rec.values())
        assert len(rec["angle_list"]) >= 3                  # three angleList poses are recorded for every case


@pytest.mark.parametrize("name", list(FRONT))
def test_oracle_equals_recorded_reference_bit_for_bit(O, name):
    S, T, step, rec = FRONT[name]
    _assert_same_record(RF.oracle_front(O, S, T, step), rec, name)


@pytest.mark.parametrize("name", list(QM))
def test_oracle_pcr_qm_equals_recorded_reference_bit_for_bit(O, name):
    A, T, want = QM[name]
    assert RF.same_bits(O.pcr_qm(A, T), want)


@pytest.mark.parametrize("name", list(FRONT))
def test_recorded_volume_has_no_near_ties_within_a_window(name):
    """Two unequal entries of one 5x5x5 window differ by more than 1e-10 relative, so a device volume within 1e-13 of the
    record orders every window -- and the arg-min -- as the record does.  Equal entries stay equal candidates only if the
    device makes them equal too; the GPU test compares the candidates outright."""
    v = FRONT[name][3]["value"]
    g = v.shape[0]

    def cut(d):          # the two slices that pair entry x with entry x + d along one axis
        return (slice(0, g - d), slice(d, g)) if d >= 0 else (slice(-d, g), slice(0, g + d))

    worst = np.inf
    for d in np.ndindex(9, 9, 9):
        d = tuple(int(x) - 4 for x in d)
        if d <= (0, 0, 0) or max(abs(x) for x in d) >= g:     # each unordered pair once
            continue
        (a0, b0), (a1, b1), (a2, b2) = (cut(x) for x in d)
        a, b = v[a0, a1, a2], v[b0, b1, b2]
        ne = a != b
        if ne.any():
            worst = min(worst, (np.abs(a - b)[ne] / np.maximum(np.abs(a), np.abs(b))[ne]).min())
    assert worst > 1e-10, worst


def test_recorded_argmin_is_strict_in_the_whole_volume():
    """The arg-min runs over the whole volume, not a window: the recorded minimum is unique or its runners-up are more
    than 1e-10 relative away."""
    for name, (_, _, _, rec) in FRONT.items():
        v = np.sort(rec["value"].reshape(-1))
        later = v[v != v[0]]
        assert later.size == 0 or (later[0] - v[0]) > 1e-10 * later[0], name


# ---- live runs: only where oracle/_ref/kss_ref_front has been built (the reference tree does not travel) -----------------
needs_binary = pytest.mark.skipif(not RF.have_binary(), reason="oracle/_ref/kss_ref_front is built only where the reference tree exists")


@needs_binary
@pytest.mark.parametrize("name", list(FRONT))
def test_live_reference_reproduces_fixture(name):
    S, T, step, rec = FRONT[name]
    _assert_same_record(RF.ref_front(S, T, step), rec, name)


@needs_binary
def test_live_reference_reproduces_fixture_qm():
    for name, (A, T, want) in QM.items():
        assert RF.same_bits(RF.ref_qm(A, T), want), name


@needs_binary
@pytest.mark.parametrize("seed,ns,nt,step", [(31, 150, 131, 8.0), (32, 97, 200, 4.0), (33, 64, 65, 10.0)])
def test_live_reference_equals_oracle_on_fresh_pairs(O, seed, ns, nt, step):
    rng = np.random.default_rng(seed)
    S = rng.normal(size=(ns, 3)) * np.array([1.0, 0.6, 0.3]) * rng.uniform(0.5, 3.0) + rng.normal(size=3)
    T = rng.normal(size=(nt, 3)) * np.array([0.9, 0.5, 0.35]) + rng.normal(size=3) * 2.0
    _assert_same_record(RF.oracle_front(O, S, T, step), RF.ref_front(S, T, step), seed)
    A = rng.normal(size=(ns, 3))
    assert RF.same_bits(O.pcr_qm(A, T), RF.ref_qm(A, T))
