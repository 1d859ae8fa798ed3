"""CPU test: the restatement of reciprocal ICP (tests/recip_ref.py) against itself -- on exact NN maps its two forms
of the filter agree bit for bit and its mutual winners are a subset of tests/o2o_ref.py's winners; on an injective mutual map the
filter is the identity; a stray source alone on its target goes where one-to-one keeps it -- and the defaults of recip_params."""
import numpy as np
import pytest

import o2o_ref as OR
import recip_ref as RR

F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _clouds(seed, n, nt, spread=1.0):
    rng = np.random.default_rng(seed)
    return (spread * rng.uniform(-1.0, 1.0, (n, 3))).astype(F32), rng.uniform(-1.0, 1.0, (nt, 3)).astype(F32)


@pytest.mark.parametrize("n,nt", [(1, 1), (63, 80), (257, 200), (1000, 1300), (1500, 400)])
def test_both_forms_agree_and_winners_are_a_subset_of_one_to_one(O, n, nt):
    src, tgt = _clouds(n + 7 * nt, n, nt)
    src[: n // 20] = src[n // 2: n // 2 + n // 20]          # duplicate rows: equal keys, the lower index wins
    idx, d2 = O.nn_brute(src, tgt)
    a = RR.filter_nn(O, src, tgt, idx, d2, 1.0)
    b = RR.filter_direct(src, tgt, idx, d2, 1.0)
    assert a[2:] == b[2:]
    assert np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1]))
    o_idx, o_d2, m, u = OR.filter(idx, d2, nt, 1.0)
    assert (a[2], a[3]) == (m, u) and a[4] <= u <= m
    kept = a[0] >= 0
    assert np.all(o_idx[kept] == a[0][kept]) and np.array_equal(_bits(o_d2[kept]), _bits(a[1][kept]))
    assert int(kept.sum()) == a[4]
    # every target is claimed by at most one mutual winner, and that winner is its nearest source
    assert len(np.unique(a[0][kept])) == a[4]
    rev, _ = O.nn_brute(tgt, src)
    assert np.array_equal(rev[a[0][kept]], np.nonzero(kept)[0])


def test_injective_mutual_map_is_the_identity(O):
    g = (np.arange(12) - 5.5) * 0.1
    tgt = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(F32)
    rng = np.random.default_rng(5)
    pick = rng.permutation(len(tgt))[:700]
    src = (tgt[pick] + rng.uniform(-0.01, 0.01, (700, 3))).astype(F32)
    idx, d2 = O.nn_brute(src, tgt)
    assert np.array_equal(idx, pick)
    for got in (RR.filter_nn(O, src, tgt, idx, d2, 1.0), RR.filter_direct(src, tgt, idx, d2, 1.0)):
        assert got[2:] == (700, 700, 700)
        assert np.array_equal(got[0], idx) and np.array_equal(_bits(got[1]), _bits(d2))


def test_a_stray_source_alone_on_its_target_is_dropped(O):
    tgt = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]], F32)
    src = np.array([[0.01, 0, 0], [1.01, 0, 0], [2.4, 0, 0], [2.01, 0.3, 0]], F32)          # 2 and 3 both choose target 2: 3 is nearer
    src = np.concatenate([src, np.array([[-0.5, 0, 0]], F32)])                             # 4 chooses target 0, where 0 is nearer
    idx, d2 = O.nn_brute(src, tgt)
    assert list(idx) == [0, 1, 2, 2, 0]
    o_idx = OR.filter(idx, d2, 3, 1.0)[0]
    assert list(o_idx) == [0, 1, -1, 2, -1]
    assert list(RR.filter_nn(O, src, tgt, idx, d2, 1.0)[0]) == [0, 1, -1, 2, -1]
    d2[0] = F32(0.5)          # an arbitrary d2: the filter takes it as given -- source 4 now wins target 0 ...
    assert list(OR.filter(idx, d2, 3, 1.0)[0]) == [-1, 1, -1, 2, 0]
    got = RR.filter_direct(src, tgt, idx, d2, 1.0)
    assert list(got[0]) == [-1, 1, -1, 2, -1] and got[2:] == (5, 3, 2)          # ... and source 0, nearer by rkey, rejects it
    d2[4] = F32(0.0)          # a winner whose given d2 is below every reverse distance is mutual, whatever its true distance
    assert list(RR.filter_direct(src, tgt, idx, d2, 1.0)[0]) == [-1, 1, -1, 2, 0]


def test_direct_form_special_values():
    tgt = np.array([[0, 0, 0], [5, 5, 5]], F32)
    src = np.array([[0.1, 0, 0], [0.1, 0, 0], [np.nan, 0, 0], [5, 5, 5]], F32)
    idx = np.array([0, 0, 0, 1], np.int32)
    d2 = np.array([0.01, 0.01, 0.0, -0.0], F32)
    d2[:2] = RR.dist2(src[:2], tgt[0])
    got = RR.filter_direct(src, tgt, idx, d2, 1.0)
    # source 2 claims target 0 with d2 = 0 and wins it; its own NaN distance beats nothing, but sources 0 and 1 do not beat key 0
    assert list(got[0]) == [-1, -1, 0, 1] and got[2:] == (4, 2, 2)
    assert _bits(got[1])[3] == 0x80000000 and _bits(got[1])[0] == 0x7FC00000


def test_recip_params_defaults(pkg):
    rp = pkg.recip_params()
    assert rp.overlap == 1.0 and rp.metric == pkg.binding.METRIC_POINT and not rp.trace_recip
    assert pkg.recip_params(overlap=0.5, metric=pkg.binding.METRIC_PLANE).metric == pkg.binding.METRIC_PLANE
    with pytest.raises(AttributeError):
        pkg.recip_params(nothing=1)
