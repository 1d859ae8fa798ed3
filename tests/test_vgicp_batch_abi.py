"""CPU test: the two entry points of batched voxelized generalized ICP are declared by the header, exported by
the built library and listed by the binding with their signatures, the Context methods exist, and a null context is refused before
anything touches a device."""
import os
import re

from conftest import ROOT

NAMES = ["kss_icp_vgicp_batch", "kss_icp_vgicp_batch_dev"]


def test_header_declares_the_vgicp_batch_entry_points():
    hdr = open(os.path.join(ROOT, "include", "kssicp.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(kss_[a-z0-9_]+)\s*\(", hdr))
    assert [n for n in NAMES if n not in declared] == []


def test_library_exports_and_binding_lists_them(pkg):
    exported = set(pkg.exported_symbols())
    assert [n for n in NAMES if n not in exported] == []
    assert [n for n in NAMES if n not in pkg.binding.SYMBOLS] == []
    L = pkg.load_library()
    for n in NAMES:
        assert len(getattr(L, n).argtypes) == 11, n          # the binding declares its signature
    for m in ("icp_vgicp_batch", "icp_vgicp_batch_dev"):
        assert callable(getattr(pkg.Context, m))


def test_null_context_needs_no_device(pkg):
    L = pkg.load_library()
    assert L.kss_icp_vgicp_batch(None, None, None, None, 1, None, None, None, None, None, None) == -1
    assert L.kss_icp_vgicp_batch_dev(None, None, None, None, 1, None, None, None, None, None, None) == -1
