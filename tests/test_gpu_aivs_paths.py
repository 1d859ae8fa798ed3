"""The AIVS sampler's box paths on the device against the oracle, index for index.

`aivs_fps_box` (kss-icp_amd/csrc/kss_aivs.hip) samples a box on its fast path (own points in registers), on the general
path with the neighbour samples listed in LDS, or on the general path that re-scans the neighbour boxes; each with or
without a seeded box centre.  Evenly sampled surfaces only ever reach the fast path with a handful of neighbours.  The
clouds here (tests/aivs_shape.py) are built to reach the others; tests/test_aivs_shape_host.py proves on the CPU that each
does, and the case names say which path a case is there for.  The reference is `O.aivs`, the serial restatement with none
of these paths.  The selection is integer and the coordinates are copies: no tolerance anywhere."""
import numpy as np
import pytest

import aivs_shape as A

pytestmark = pytest.mark.gpu

_CACHE = {}


def _cases(pkg):
    if "cases" not in _CACHE:
        _CACHE["cases"] = A.path_cases(pkg.synth)
    return _CACHE["cases"]


def _oracle(O, pkg, name, P=None, m=None):
    """The oracle's selection of a named case, computed once and handed out read-only."""
    if name not in _CACHE:
        if P is None:
            P, m = _cases(pkg)[name]
        ref = O.aivs(P, m)
        ref.setflags(write=False)
        _CACHE[name] = ref
    return _CACHE[name]


def _check(got, P, m, ref, where):
    out, idx = got
    P = np.asarray(P, dtype=np.float64)
    same = np.array_equal(idx, ref)
    if not same:
        k = min(len(idx), len(ref))
        diff = np.flatnonzero(idx[:k] != ref[:k])
        first = int(diff[0]) if len(diff) else k
        raise AssertionError("%s: selection differs from the oracle's: %d against %d indices, first difference at output %d; %s"
                             % (where, len(idx), len(ref), first, A.describe(P, ref, m)))
    assert out.dtype == np.float64 and out.shape == (len(ref), 3), where
    assert np.array_equal(out.view(np.uint64), P[idx].view(np.uint64)), where      # copies, bit for bit
    assert len(np.unique(idx)) == len(idx), where


CASE_NAMES = ["A-corner-cluster-general-seed-list-rescan",
              "B-half-fast-noseed-slots123", "B-nearfull-fast-overflow-then-rescan", "B-full-rate1-overflow", "B-over-rate-above-1",
              "C-isolated-general-seed-and-fast-seed", "D-exact-duplicates",
              "E-scaled-1e5", "E-scaled-1e5-offset-3e6", "E-scaled-1e6-centre-beyond-9999",
              "F-unit-lattice-16", "F-int-lattice-20x20x10", "F-int-lattice-permuted",
              "G-tiny-2-points", "G-tiny-3-points", "G-tiny-4-points", "G-tiny-5-points", "G-tiny-64-points"]


def test_case_list_is_the_helper_s(pkg):
    assert CASE_NAMES == list(_cases(pkg))


@pytest.mark.parametrize("name", CASE_NAMES)
def test_box_paths_match_oracle(ctx, O, pkg, name):
    P, m = _cases(pkg)[name]
    ref = _oracle(O, pkg, name)
    _check(ctx.downsample_aivs(P, m), P, m, ref, name)
    if name in ("B-full-rate1-overflow", "B-over-rate-above-1"):
        assert len(ref) == len(P)           # rate >= 1: every box ends on "nothing left" and every point comes back


def test_h_one_context_changing_shapes(ctx, O, pkg):
    """A, a small even cloud, A again, then B on ONE context: the working arrays are carved from one grow-only workspace,
    so a smaller call after a larger one sees stale bytes wherever a memset is missing."""
    cases = _cases(pkg)
    a, b = "A-corner-cluster-general-seed-list-rescan", "B-half-fast-noseed-slots123"
    small = pkg.synth.bumpy(5, 2000)
    seq = [(a,) + cases[a], ("bumpy(5, 2000)", small, 1000), (a,) + cases[a], (b,) + cases[b]]
    for step, (name, P, m) in enumerate(seq):
        _check(ctx.downsample_aivs(P, m), P, m, _oracle(O, pkg, name, P, m), "step %d: %s" % (step, name))


@pytest.mark.parametrize("order", ["A-then-even", "even-then-A"])
def test_i_pair_entry(ctx, O, pkg, order):
    """Both clouds of a registration in one call; the second runs on a worker context of its own."""
    a = "A-corner-cluster-general-seed-list-rescan"
    PA, mA = _cases(pkg)[a]
    PE, mE = pkg.synth.bumpy(6, 5000), 2000
    rA, rE = _oracle(O, pkg, a), _oracle(O, pkg, "bumpy(6, 5000)", PE, mE)
    if order == "A-then-even":
        g0, g1 = ctx.downsample_aivs_pair(PA, mA, PE, mE)
        _check(g0, PA, mA, rA, "first cloud (A)")
        _check(g1, PE, mE, rE, "second cloud (even)")
    else:
        g0, g1 = ctx.downsample_aivs_pair(PE, mE, PA, mA)
        _check(g0, PE, mE, rE, "first cloud (even)")
        _check(g1, PA, mA, rA, "second cloud (A)")
