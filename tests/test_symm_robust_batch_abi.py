"""CPU test: the two entry points of batched robust symmetric ICP are declared by the header, exported by the
built library and listed by the binding with their signatures, the Context methods exist, a null context is refused before anything
touches a device, and the header no longer says that robust symmetric ICP has no batched form."""
import os
import re

from conftest import ROOT

NAMES = ["kss_icp_symm_robust_batch", "kss_icp_symm_robust_batch_dev"]


def _header():
    return open(os.path.join(ROOT, "include", "kssicp.h")).read()


def test_header_declares_the_symm_robust_batch_entry_points():
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = set(re.findall(r"\b(kss_[a-z0-9_]+)\s*\(", hdr))
    assert [n for n in NAMES if n not in declared] == []


def test_header_no_longer_says_the_batched_form_is_missing():
    hdr = " ".join(_header().split())
    m = re.search(r"robust symmetric ICP for one pair.*?\*/", hdr)
    assert m, "the comment of kss_icp_symm_robust is gone"
    comment = m.group(0)
    assert "The batched form" not in comment
    assert "kss_icp_symm_robust_batch" in comment          # it points at the batch instead
    for kept in ("rimming on this metric", "generalized ICP", "mirror classes", "CLI"):   # what stays out of scope is still said
        assert kept in comment, kept


def test_library_exports_and_binding_lists_them(pkg):
    exported = set(pkg.exported_symbols())
    assert [n for n in NAMES if n not in exported] == []
    assert [n for n in NAMES if n not in pkg.binding.SYMBOLS] == []
    L = pkg.load_library()
    for n in NAMES:
        assert len(getattr(L, n).argtypes) == 15, n          # the binding declares its signature
    for m in ("icp_symm_robust_batch", "icp_symm_robust_batch_dev"):
        assert callable(getattr(pkg.Context, m))


def test_null_context_needs_no_device(pkg):
    L = pkg.load_library()
    none15 = [None] * 7 + [1] + [None] * 7
    assert L.kss_icp_symm_robust_batch(*none15) == -1
    assert L.kss_icp_symm_robust_batch_dev(*none15) == -1
