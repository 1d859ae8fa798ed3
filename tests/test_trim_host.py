"""CPU tests of trimmed ICP: kss_trim_rank against the Python expression, and the yardstick itself -- the restatement in
tests/trim_ref.py must recover the true motion of the three partly overlapping pairs with half of the correspondences
kept, and miss it with all of them kept (the rule of every other ICP entry point).

The bars judge the restatement and the method, never the library's output (DESIGN.md 2.10 holds the values): trimmed
max|dR| and max|dt| below 2e-3, untrimmed max|dt| above 2e-2."""
import math

import numpy as np
import pytest

import trim_ref as TR

F32, F64 = np.float32, np.float64

PAIRS = [(1, 6000, 10.0, -0.35, 0.5), (2, 6000, 15.0, -0.2, 0.6), (3, 8000, 8.0, -0.5, 0.3)]
SHAPES = {1: (4395, 3999, 0.545), 2: (4604, 3662, 0.492), 3: (5204, 5892, 0.595)}
# (iterations, state) of the restatement, PCL's default criteria, max_iterations 200: [pair][metric] = (overlap 1, overlap 0.5)
EXPECTED = {1: {TR.POINT: ((13, 4), (23, 2)), TR.PLANE: ((7, 4), (6, 2))},
            2: {TR.POINT: ((13, 4), (21, 2)), TR.PLANE: ((4, 4), (4, 2))},
            3: {TR.POINT: ((16, 4), (28, 2)), TR.PLANE: ((4, 4), (5, 2))}}


@pytest.mark.parametrize("overlap", [1e-9, 0.1, 1.0 / 3.0, 0.5, 0.9, 1.0 - 2.0 ** -53, 1.0])
@pytest.mark.parametrize("m", [0, 1, 2, 3, 10, 4395, 2 ** 31 + 5])
def test_trim_rank_matches_expression(pkg, m, overlap):
    want = 0 if m == 0 else max(1, int(math.ceil(overlap * float(m))))
    assert pkg.trim_rank(m, overlap) == want
    assert TR.rank(m, overlap) == want


@pytest.mark.parametrize("overlap", [0.0, -0.5, 1.0000001, float("nan")])
def test_trim_rank_rejects_overlap_out_of_range(pkg, overlap):
    with pytest.raises(pkg.KssError) as e:
        pkg.trim_rank(10, overlap)
    assert e.value.status == -1


def test_threshold_restatement_on_small_cases():
    d2 = np.array([0.5, np.nan, -1.0, 0.25, np.inf, 2.0, 0.25, -0.0, 0.75], F32)
    cand, m, k, tau, kept = TR.threshold(d2, 1.0, 0.5)
    assert m == 5 and k == 3 and tau == F32(0.25) and kept.sum() == 3      # {-0.0, 0.25, 0.25}
    cand, m, k, tau, kept = TR.threshold(d2, 1.0, 1.0)
    assert k == 5 and tau == F32(0.75) and np.array_equal(kept, cand)
    cand, m, k, tau, kept = TR.threshold(d2, 1.0, 0.3)
    assert k == 2 and tau == F32(0.25) and kept.sum() == 3                 # the tie at tau is kept whole
    cand, m, k, tau, kept = TR.threshold(np.array([np.nan, 5.0], F32), 1.0, 0.5)
    assert m == 0 and k == 0 and tau == 0 and kept.sum() == 0


def _pair(pkg, O, spec):
    pid, n, deg, lo, hi = spec
    src, tgt, R, t, ov = pkg.synth.make_partial_pair(pid, n, deg, lo, hi)
    nrm = O.normals_pcl(tgt.astype(F64), 20).astype(F32)
    return src, tgt, nrm, R.T, -R.T @ t, ov


@pytest.mark.parametrize("spec", PAIRS, ids=lambda s: "pair%d" % s[0])
def test_partial_pairs_have_the_stated_shape(pkg, spec):
    src, tgt, R, t, ov = pkg.synth.make_partial_pair(*spec)
    ns, nt, o = SHAPES[spec[0]]
    assert (len(src), len(tgt)) == (ns, nt) and abs(ov - o) < 5e-4
    assert src.dtype == F32 and tgt.dtype == F32
    again = pkg.synth.make_partial_pair(*spec)
    assert np.array_equal(src, again[0]) and np.array_equal(tgt, again[1])


@pytest.mark.parametrize("metric", [TR.POINT, TR.PLANE], ids=["point", "plane"])
@pytest.mark.parametrize("spec", PAIRS, ids=lambda s: "pair%d" % s[0])
def test_yardstick_trimmed_recovers_untrimmed_does_not(pkg, O, spec, metric):
    src, tgt, nrm, R_true, t_true, _ = _pair(pkg, O, spec)
    full = TR.icp_trimmed(O, src, tgt, nrm, 1.0, metric, max_iterations=200)
    half = TR.icp_trimmed(O, src, tgt, nrm, 0.5, metric, max_iterations=200)
    for name, r in (("overlap 1.0", full), ("overlap 0.5", half)):
        print("pair %d metric %d %s: %d it., state %d, max|dR| %.2e, max|dt| %.2e" % (
            spec[0], metric, name, r["iterations"], r["state"], np.abs(r["T"][:3, :3] - R_true).max(),
            np.abs(r["T"][:3, 3] - t_true).max()))
    assert np.abs(half["T"][:3, :3] - R_true).max() < 2e-3
    assert np.abs(half["T"][:3, 3] - t_true).max() < 2e-3
    assert np.abs(full["T"][:3, 3] - t_true).max() > 2e-2
    e_full, e_half = EXPECTED[spec[0]][metric]
    assert (full["iterations"], full["state"]) == e_full
    assert (half["iterations"], half["state"]) == e_half
    assert half["converged"] and full["converged"]
    # every pass kept at least k and at most m, and the cut is one of the pass's distances
    tt = half["trace_trim"]
    assert np.all(tt[:, 3] <= tt[:, 0]) and np.all(tt[:, 1] == np.ceil(0.5 * tt[:, 0]))
    if metric == TR.POINT:
        assert np.all(tt[:, 3] >= tt[:, 1])
