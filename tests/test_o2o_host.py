"""CPU tests of one-to-one ICP: the restatement in tests/o2o_ref.py checks itself -- the filter on small cases
written out by hand and against a plain loop over the targets, the loop on the three partly overlapping pairs of
tests/test_trim_host.py, where it must recover the true motion at overlap 1.0 and 0.9 with nothing told while all correspondences
miss it -- and the library's default parameters.

The bars judge the restatement and the method, never the library's output: max|dR| and max|dt| below 2e-3 (the trimmed
yardstick's bar), all correspondences max|dt| above 2e-2."""
import numpy as np
import pytest

import o2o_ref as OR
import trim_ref as TR

F32, F64 = np.float32, np.float64
PAIRS = [(1, 6000, 10.0, -0.35, 0.5), (2, 6000, 15.0, -0.2, 0.6), (3, 8000, 8.0, -0.5, 0.3)]
QNAN = 0x7FC00000


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def test_filter_restatement_by_hand():
    #                0     1     2      3     4       5      6     7     8    9
    idx = np.array([2, 2, 2, 0, 0, 1, 5, -1, 1, 2], np.int32)
    d2 = np.array([0.5, 0.25, 0.25, -0.0, 0.0, np.nan, 0.1, 0.1, 2.0, -1.0], F32)
    idx_f, d2_f, m, u = OR.filter(idx, d2, 5, 1.0)
    # target 2: sources 1 and 2 tie at 0.25, the lower index wins; target 0: -0.0 and +0.0 tie, source 3 wins; target 1 has no
    # candidate (a NaN, a d2 above max_d2); source 6 points outside the target, 7 has no target, 9 is negative
    assert m == 5 and u == 2
    assert idx_f.tolist() == [-1, 2, -1, 0, -1, 1, 5, -1, 1, 2]
    want = _bits(d2).copy()
    want[[0, 2, 4]] = QNAN
    assert np.array_equal(_bits(d2_f), want)
    assert _bits(d2_f)[3] == 0x80000000          # the winner keeps its -0.0f bit for bit


def test_filter_restatement_matches_a_plain_loop():
    rng = np.random.default_rng(3)
    n, nt = 5000, 700
    idx = rng.integers(-2, nt + 3, n).astype(np.int32)
    d2 = rng.choice(np.array([0.0, -0.0, 0.125, 0.25, 0.5, 1.0, 1.5, np.nan, -0.5], F32), n).astype(F32)
    idx_f, d2_f, m, u = OR.filter(idx, d2, nt, 1.0)
    cand = OR.candidates(idx, d2, nt, 1.0)
    want_i, want_b = idx.copy(), _bits(d2).copy()
    winners = 0
    for j in range(nt):
        rows = np.nonzero(cand & (idx == j))[0]
        if len(rows) == 0:
            continue
        winners += 1
        best = min(rows, key=lambda i: (abs(float(d2[i])), i))
        for i in rows:
            if i != best:
                want_i[i] = -1
                want_b[i] = QNAN
    assert m == int(cand.sum()) and u == winners
    assert np.array_equal(idx_f, want_i) and np.array_equal(_bits(d2_f), want_b)


def test_filter_restatement_leaves_an_injective_map_alone():
    rng = np.random.default_rng(4)
    idx = rng.permutation(300).astype(np.int32)
    d2 = rng.uniform(0, 1, 300).astype(F32)
    idx_f, d2_f, m, u = OR.filter(idx, d2, 300, 1.0)
    assert m == u == 300 and np.array_equal(idx_f, idx) and np.array_equal(_bits(d2_f), _bits(d2))


@pytest.mark.parametrize("metric", [OR.POINT, OR.PLANE], ids=["point", "plane"])
@pytest.mark.parametrize("spec", PAIRS, ids=lambda s: "pair%d" % s[0])
def test_yardstick_one_to_one_recovers_with_nothing_told(pkg, O, spec, metric):
    src, tgt, R, t, _ = pkg.synth.make_partial_pair(*spec)
    R_true, t_true = R.T, -R.T @ t
    nrm = O.normals_pcl(tgt.astype(F64), 20).astype(F32) if metric == OR.PLANE else None
    full = TR.icp_trimmed(O, src, tgt, nrm, 1.0, metric, max_iterations=200)
    assert np.abs(full["T"][:3, 3] - t_true).max() > 2e-2
    for overlap in (1.0, 0.9):
        r = OR.icp_o2o(O, src, tgt, nrm, overlap, metric, max_iterations=200)
        print("pair %d metric %d overlap %.1f: %d it., state %d, max|dR| %.2e, max|dt| %.2e" % (
            spec[0], metric, overlap, r["iterations"], r["state"], np.abs(r["T"][:3, :3] - R_true).max(),
            np.abs(r["T"][:3, 3] - t_true).max()))
        assert r["converged"]
        assert np.abs(r["T"][:3, :3] - R_true).max() < 2e-3
        assert np.abs(r["T"][:3, 3] - t_true).max() < 2e-3
        tt = r["trace_o2o"]
        assert np.all(tt[:, 0] <= tt[:, 4]) and np.all(tt[:, 0] < len(src))      # u <= m, and the rejection bites
        assert np.all(tt[:, 1] == np.ceil(overlap * tt[:, 0])) and np.all(tt[:, 3] <= tt[:, 0])


def test_default_parameters(pkg):
    op = pkg.o2o_params()
    assert op.overlap == 1.0 and op.metric == pkg.METRIC_POINT and not op.trace_o2o
    assert pkg.load_library().kss_o2o_default_params(None) == -1
    assert pkg.O2O_NINFO == 5
