"""CPU tests of robust symmetric ICP: the restatement in tests/symm_robust_ref.py against the symmetric and the
robust restatements it is composed from, the two headline scenes on the restatement under the conditions the GPU test repeats,
and the header, the exports and the binding of the four entry points."""
import os
import re

import numpy as np
import pytest

import robust_ref as RR
import symm_ref as S
import symm_robust_ref as SR
from conftest import ROOT

F32, F64 = np.float32, np.float64
NAMES = ["kss_symm_robust_sums", "kss_symm_robust_sums_dev", "kss_icp_symm_robust", "kss_icp_symm_robust_dev"]
SHARED = list(range(29)) + [30]          # the slots kss_icp_symm and the L2 form share


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == F64 else np.uint32)


def test_l2_restatement_equals_symm_restatement(pkg, O):
    """KSS_LOSS_L2 is kss_icp_symm: w = 1 multiplies exactly, so the two restatements agree bit for bit in the shared slots
    (both sum the same terms in the same numpy order), with a fixed and with the automatic scale."""
    src, tgt, _, _ = SR.halves_pair(pkg.synth, 2, 1500, 10.0, n_src=1100)
    sn = O.normals_pcl(src.astype(F64), 20).astype(F32)
    tn = O.normals_pcl(tgt.astype(F64), 20).astype(F32)
    a = S.icp_symm(O, src, sn, tgt, tn, max_iterations=40)
    assert a["iterations"] >= 2
    for scale in (0.05, 0.0):
        b = SR.icp_symm_robust(O, src, sn, tgt, tn, SR.L2, scale=scale, max_iterations=40)
        assert b["iterations"] == a["iterations"] and b["state"] == a["state"] and b["converged"] == a["converged"]
        assert np.array_equal(_bits(b["T"]), _bits(a["T"]))
        assert np.array_equal(_bits(b["trace_Tk"]), _bits(a["trace_Tk"]))
        assert np.array_equal(_bits(b["trace_sums"][:, SHARED]), _bits(a["trace_sums"][:, SHARED]))
        assert b["last_mse"] == a["last_mse"] and b["fitness"] == a["fitness"]
        # [29] = m and [31] = cnt: with L2 every candidate is kept
        assert np.array_equal(b["trace_sums"][:, 29], b["trace_sums"][:, 31])
        assert np.array_equal(b["trace_sums"][:, 31], a["trace_sums"][:, 0])
        assert np.array_equal(b["trace_robust"][:, 0], a["trace_sums"][:, 0])


@pytest.mark.parametrize("loss", RR.LOSSES)
def test_weights_match_the_library(pkg, loss):
    """The restatement's weight is kss_robust_weight, bit for bit, on squared symmetric residuals around and far from the scale."""
    rng = np.random.default_rng(loss)
    r = np.concatenate([rng.normal(scale=0.05, size=200), [0.0, 0.05, -0.05, 2.0, 1e-20, 1e20]])
    x = r * r
    for c2 in (0.05 * 0.05, 0.0, 1e-60, 7.3):
        ref = RR.weight(loss, x, c2)
        got = np.array([pkg.robust_weight(loss, float(v), float(c2)) for v in x], F64)
        assert np.array_equal(_bits(got), _bits(ref)), (loss, c2)


# ---- the headline: only the combination registers these pairs ----
_RUNS = {}


def _run(pkg, O, name, what):
    key = (name, what)
    if key not in _RUNS:
        src, tgt, sn, tn, R_true, t_true = SR.scene(pkg, O, name)
        if what == "symm":
            out = S.icp_symm(O, src, sn, tgt, tn, max_iterations=100)
        elif what == "p2l_tukey":
            out = RR.icp_robust(O, src, tgt, tn, RR.TUKEY, RR.PLANE, max_iterations=100)
        else:
            out = SR.icp_symm_robust(O, src, sn, tgt, tn, what, max_iterations=100)
        eR, et = SR.errors(out["T"], R_true, t_true)
        print("scene %s %s: %d passes, state %d, converged %d, |R - R_true| %.2e, |t - t_true| %.2e" % (
            name, what, out["iterations"], out["state"], out["converged"], eR, et))
        _RUNS[key] = (out, eR)
    return _RUNS[key]


@pytest.mark.parametrize("name", ["A", "B"])
def test_scene_sizes(pkg, O, name):
    src, tgt, sn, tn, _, _ = SR.scene(pkg, O, name)
    assert (len(src), len(tgt)) == ((2000, 2000) if name == "A" else (2196, 2177))
    assert sn.shape == src.shape and tn.shape == tgt.shape


@pytest.mark.parametrize("loss", [SR.TUKEY, SR.CAUCHY])
@pytest.mark.parametrize("name", ["A", "B"])
def test_robust_symmetric_registers_the_scene(pkg, O, name, loss):
    """Restatement, max_iterations = 100, oracle PCL normals at k = 20 on the clouds as given.  Measured:
    A Tukey 3.3e-4 in 11 passes, A Cauchy 3.5e-4 in 12, B Tukey 4.2e-4 in 19, B Cauchy 3.0e-4 in 26."""
    out, eR = _run(pkg, O, name, loss)
    assert out["converged"] and out["state"] in (2, 3, 4)
    assert eR <= 1e-3


@pytest.mark.parametrize("name", ["A", "B"])
def test_huber_symmetric_is_reported(pkg, O, name):
    """Printed, not asserted: Huber's weight never reaches zero, gross outliers keep pulling (A 6.1e-4 in 10 passes, B 1.8e-3 in
    21)."""
    out, eR = _run(pkg, O, name, SR.HUBER)
    assert out["iterations"] >= 1


@pytest.mark.parametrize("name,bar", [("A", 3e-3), ("B", 2e-2)])
def test_plain_symmetric_does_not(pkg, O, name, bar):
    """The bars are the f64 prototype's; the restatement ends at 8.3e-3 (A, 8 passes) and 7.6e-2 (B, 12 passes)."""
    out, eR = _run(pkg, O, name, "symm")
    assert eR >= bar


@pytest.mark.parametrize("name", ["A", "B"])
def test_tukey_point_to_plane_ends_in_a_wrong_minimum(pkg, O, name):
    """1.2 on both scenes (34 and 30 passes)."""
    out, eR = _run(pkg, O, name, "p2l_tukey")
    assert eR >= 0.5


# ---- header, exports, binding ----
def test_header_declares_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "kssicp.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(kss_[a-z0-9_]+)\s*\(", hdr))
    assert [n for n in NAMES if n not in declared] == []


def test_library_exports_and_binding_lists_them(pkg):
    exported = set(pkg.exported_symbols())
    assert [n for n in NAMES if n not in exported] == []
    assert [n for n in NAMES if n not in pkg.binding.SYMBOLS] == []
    L = pkg.load_library()
    for n, k in zip(NAMES, (14, 14, 12, 12)):
        assert len(getattr(L, n).argtypes) == k, n
    for m in ("symm_robust_sums", "symm_robust_sums_dev", "icp_symm_robust", "icp_symm_robust_dev"):
        assert callable(getattr(pkg.Context, m))


def test_null_context_needs_no_device(pkg):
    L = pkg.load_library()
    assert L.kss_symm_robust_sums(None, None, None, None, None, None, 1, 1, 1.0, None, None, None, None, None) == -1
    assert L.kss_symm_robust_sums_dev(None, None, None, None, None, None, 1, 1, 1.0, None, None, None, None, None) == -1
    assert L.kss_icp_symm_robust(None, None, 1, None, None, 1, None, None, None, None, None, None) == -1
    assert L.kss_icp_symm_robust_dev(None, None, 1, None, None, 1, None, None, None, None, None, None) == -1
