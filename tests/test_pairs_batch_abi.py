"""CPU test: the six entry points of the batched point-to-plane / trimmed ICP are declared by the header,
exported by the built library and listed by the binding, and the host-side wrappers exist."""
import os
import re

from conftest import ROOT

NAMES = ["kss_icp_p2l_batch", "kss_icp_p2l_batch_dev", "kss_icp_trimmed_batch", "kss_icp_trimmed_batch_dev",
         "kss_trim_threshold_batch", "kss_trim_threshold_batch_dev"]


def test_header_declares_the_batch_entry_points():
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
        assert getattr(L, n).argtypes, n          # the binding declares its signature
    assert L.kss_version() == 100
    for m in ("icp_p2l_batch", "icp_p2l_batch_dev", "icp_trimmed_batch", "icp_trimmed_batch_dev", "trim_threshold_batch",
              "trim_threshold_batch_dev"):
        assert callable(getattr(pkg.Context, m))


def test_argument_errors_need_no_device(pkg):
    """A null context is refused before anything touches the GPU."""
    L = pkg.load_library()
    assert L.kss_icp_p2l_batch(None, None, None, None, None, None, 1, None, None) == -1
    assert L.kss_icp_trimmed_batch_dev(None, None, None, None, None, None, 1, None, None, None, None, None) == -1
    assert L.kss_trim_threshold_batch(None, None, None, 1, 1.0, None, None) == -1
