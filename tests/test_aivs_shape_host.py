"""The premises of tests/test_gpu_aivs_paths.py, checked on the CPU: every designed cloud has the shape its test relies on.

`aivs_shape.box_stats` bounds, per box, the neighbour samples in reach from the oracle's selection (below) and from the
populations and budgets (above); `aivs_shape.classes` names the path a box is then CERTAIN to take in `aivs_fps_box`
(kss-icp_amd/csrc/kss_aivs.hip).  The thresholds 64, 256 and 512 live in aivs_shape.py.  A path test can therefore not
pass because its input missed the path: if a seed or a parameter drifts, these fail first, without a GPU."""
import time

import numpy as np
import pytest

import aivs_shape as A


@pytest.fixture(scope="module")
def shapes(O, pkg):
    """name -> (cloud, point_num, oracle selection, box stats, class counts), computed once."""
    out = {}
    for name, (P, m) in A.path_cases(pkg.synth).items():
        idx = O.aivs(P, m)
        st = A.box_stats(P, idx, m)
        out[name] = (P, m, idx, st, A.classes(st))
    return out


def _boxes(st, size, reach):
    """Boxes of one class, with their populations: size in fast64 / fast256 / general, reach in seed / list / over."""
    m, lo, hi = st.m, st.reach_lo, st.reach_hi
    in_size = {"fast64": m <= A.WAVE, "fast256": (m > A.WAVE) & (m <= A.FAST_MAX), "general": m > A.FAST_MAX}[size]
    in_reach = {"seed": hi == 0, "list": (lo >= 1) & (hi <= A.L2_CAP), "over": lo > A.L2_CAP}[reach]
    return np.flatnonzero(in_size & in_reach)


def test_helper_restates_the_grid():
    assert (A.WAVE, A.FAST_MAX, A.L2_CAP) == (64, 256, 512)
    assert [A.box_num(n) for n in (1, 9999, 10000, 49999, 50000, 99999, 100000, 499999, 500000, 999999)] == [
        10, 10, 20, 20, 30, 30, 40, 40, 50, 50]
    P = np.array([[0.0, 0.0, 0.0], [1.0, 0.5, 0.21], [0.1, 0.25, 0.2], [0.10000001, 0.5, 0.05]])
    g = A.grid_of(P)
    assert (g.box_num, g.unit, g.nx, g.ny, g.nz, g.R) == (10, 0.1, 10, 5, 3, 0.1 * 3.0 / 4.0)
    # 0 maps to box 1; a point on a face belongs to the box below it; anything above the face to the next
    assert A.box_coords(P, g).tolist() == [[1, 1, 1], [10, 5, 3], [1, 3, 2], [2, 5, 1]]
    assert A.colour_of(np.array([[1, 1, 1], [2, 1, 1], [2, 2, 1], [1, 2, 1], [1, 1, 2], [2, 1, 2], [2, 2, 2], [1, 2, 2]])).tolist() == list(range(8))
    assert A.budgets([10, 10, 11, 3], 100, 12).tolist() == [1, 1, 2, 1]      # 1.2 -> 1, 1.32 -> 2, 0.36 -> 1
    # two boxes side by side: (1,1,1) of the first colour, (2,1,1) of the second, whose cube spans x in [0.075, 0.225]:
    # of the three points of (1,1,1), only the one at x = 0.09 is inside it
    Q = np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [0.09, 0.05, 0.05], [0.05, 0.05, 0.05], [0.16, 0.05, 0.05]])
    st = A.box_stats(Q, selection=[2])
    k1, k2 = st.box.tolist().index(1), st.box.tolist().index(2)
    assert (st.m[k1], st.colour[k1], st.reach_lo[k1], st.reach_hi[k1]) == (3, 0, 0, 0)
    assert (st.m[k2], st.colour[k2], st.reach_lo[k2], st.reach_hi[k2]) == (1, 1, 1, 1)
    st = A.box_stats(Q, selection=[3, 0])
    assert (st.reach_lo[k2], st.reach_hi[k2]) == (0, 1) and A.box_stats(Q, selection=[4]).reach_lo[k2] == 0
    assert A.box_stats(Q, selection=[2], point_num=1).reach_hi[k2] == 1      # budget of (1,1,1): 3 * 0.2 = 0.6 -> 1


def test_helper_is_quick_on_the_largest_designed_cloud():
    P = A.cloud_a()
    assert len(P) == 7500
    t0 = time.perf_counter()
    A.box_stats(P, np.arange(0, len(P), 2), 3750)
    assert time.perf_counter() - t0 < 1.0


def test_every_designed_cloud_has_ten_boxes_along_its_largest_extent(shapes):
    for name, (P, m, idx, st, cls) in shapes.items():
        assert len(P) < 10000 and st.grid.box_num == 10, name
        assert max(st.grid.nx, st.grid.ny, st.grid.nz) == 10, name
        assert len(set(idx.tolist())) == len(idx), name
        assert st.m.sum() == len(P), name
        assert (st.reach_lo <= st.reach_hi).all(), name                      # the two bounds never cross


def test_a_general_path_with_seed_with_list_and_with_rescan(shapes):
    P, m, idx, st, cls = shapes["A-corner-cluster-general-seed-list-rescan"]
    assert st.grid.unit == 0.1 and len(P) == 7500 and m == 3750
    assert (st.m > A.FAST_MAX).sum() == 8                                    # the eight boxes round the corner, one of every colour
    assert sorted(st.colour[st.m > A.FAST_MAX].tolist()) == list(range(8))
    assert len(_boxes(st, "general", "seed")) >= 1, cls
    assert len(_boxes(st, "general", "list")) >= 1, cls                      # reach_lo >= 1 and reach_hi <= 512
    assert len(_boxes(st, "general", "over")) >= 1, cls
    assert st.reach_lo.max() > 4 * A.L2_CAP, cls                             # far past the list, not just over its edge


def test_b_half_rate_fast_path_without_seed(shapes):
    P, m, idx, st, cls = shapes["B-half-fast-noseed-slots123"]
    assert st.grid.unit == 0.1 and m == len(P) // 2
    assert len(_boxes(st, "fast256", "list")) >= 1, cls
    assert len(_boxes(st, "fast64", "list")) >= 1, cls
    assert len(_boxes(st, "general", "list")) >= 1, cls


@pytest.mark.parametrize("name", ["B-nearfull-fast-overflow-then-rescan", "B-full-rate1-overflow", "B-over-rate-above-1"])
def test_b_near_full_rate_fast_path_overflows(shapes, name):
    P, m, idx, st, cls = shapes[name]
    assert len(_boxes(st, "fast256", "over")) >= 1, cls                      # the overflow exit, then the re-scan
    assert len(_boxes(st, "general", "over")) >= 1, cls
    assert (st.reach_lo[_boxes(st, "fast256", "over")] > 2 * A.L2_CAP).any(), cls
    if m >= len(P):
        # rate >= 1: every budget meets or exceeds its box, the loop ends on "nothing left", every point comes back
        assert (st.budget >= st.m).all() and len(idx) == len(P), (name, len(idx))
    else:
        assert len(idx) == m, (name, len(idx))


def test_c_isolated_boxes_take_the_seed_forms(shapes):
    P, m, idx, st, cls = shapes["C-isolated-general-seed-and-fast-seed"]
    k = _boxes(st, "general", "seed")
    assert len(k) == 1 and st.colour[k[0]] == 0 and st.m[k[0]] >= 1200, cls
    k = _boxes(st, "fast256", "seed")
    assert len(k) >= 1 and (st.m[k] > 3 * A.WAVE).any(), cls                 # slot 3 live, with seed
    k = _boxes(st, "fast256", "list")
    assert len(k) >= 1 and (st.m[k] > 3 * A.WAVE).any(), cls                 # slot 3 live, without seed


def test_d_duplicates_are_never_both_selected(shapes):
    P, m, idx, st, cls = shapes["D-exact-duplicates"]
    assert len(P) - len(np.unique(P, axis=0)) >= 500                         # (a copied row may be overwritten itself)
    assert len(idx) == m == 2250
    assert len(np.unique(P[idx], axis=0)) == len(idx)                        # a copy of a sampled point has min-distance 0
    assert len(_boxes(st, "general", "list")) >= 1 and len(_boxes(st, "fast256", "list")) >= 1, cls


def _nearest_selected(P, idx):
    S = np.asarray(P, np.float64)[idx]
    d2 = ((S[:, None, :] - S[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(d2, np.inf)
    return np.sqrt(d2.min(axis=1))


@pytest.mark.parametrize("name", ["E-scaled-1e5", "E-scaled-1e5-offset-3e6", "E-scaled-1e6-centre-beyond-9999"])
def test_e_distances_pass_the_9999_sentinels(shapes, name):
    P, m, idx, st, cls = shapes[name]
    assert st.grid.unit * np.sqrt(3.0) > 9999                                # own points of one box can be further apart than that
    assert (_nearest_selected(P, idx) > 9999).any()                          # and some sample's nearest sample is: the cut skips it
    assert len(_boxes(st, "general", "list")) >= 1 and len(_boxes(st, "fast256", "list")) >= 1, cls
    if "1e6" in name:
        # boxes none of whose points lies within 9999 of the centre have no "centre point": no seed, every min-distance 9999
        far = np.array([np.sqrt(((P[st.point_box == b] - c) ** 2).sum(axis=1)).min() > 9999 for b, c in zip(st.box, st.centre)])
        assert (far & (st.reach_hi == 0)).any() and (far & (st.m > A.FAST_MAX)).any()


@pytest.mark.parametrize("name", ["F-unit-lattice-16", "F-int-lattice-20x20x10", "F-int-lattice-permuted"])
def test_f_lattice_points_sit_on_box_faces_and_tie(shapes, name):
    P, m, idx, st, cls = shapes[name]
    f = (P - st.grid.mins) / st.grid.unit
    on_face = (f == np.trunc(f)).any(axis=1)
    assert on_face.sum() >= len(P) // 4, on_face.sum()
    assert (f == 0).any() and (f == 10).any()                                # both ends of the `== 0` / `int(f) == f` rules
    d = _nearest_selected(P, idx)
    assert len(np.unique(d.astype(np.float32))) <= 8                         # nearly all nearest distances tie
    assert cls["fast64_list"] >= 1 and cls["fast64_seed"] >= 1, cls


def test_g_tiny_clouds(shapes):
    got = {name: (len(P), m, len(idx)) for name, (P, m, idx, st, cls) in shapes.items() if name.startswith("G-")}
    assert got == {"G-tiny-2-points": (2, 1, 2), "G-tiny-3-points": (3, 1, 2),     # fewer than three samples: no cut
                   "G-tiny-4-points": (4, 2, 2), "G-tiny-5-points": (5, 3, 3), "G-tiny-64-points": (64, 30, 30)}, got


def test_the_six_classes_of_the_box_paths_are_all_driven(shapes):
    total = dict.fromkeys(A.CLASSES, 0)
    for name, (P, m, idx, st, cls) in shapes.items():
        for k in A.CLASSES:
            total[k] += cls[k]
    for k in ("fast64_list", "fast256_seed", "fast256_overflow", "general_seed", "general_list", "general_rescan"):
        assert total[k] >= 1, total
