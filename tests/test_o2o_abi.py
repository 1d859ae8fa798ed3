"""CPU test: the entry points of one-to-one ICP, the filter alone and the loop, single pair and batch, are declared
by the header, exported by the built library and listed by the binding with their signatures, the Context methods exist, the header
says what is not offered, and a null context is refused before anything touches a device (the argument errors that need a context
are in tests/test_gpu_o2o.py)."""
import os
import re

from conftest import ROOT

NAMES = {"kss_o2o_filter": 9, "kss_o2o_filter_dev": 9, "kss_o2o_filter_batch": 10, "kss_o2o_filter_batch_dev": 10,
         "kss_o2o_default_params": 1, "kss_icp_o2o": 10, "kss_icp_o2o_dev": 10, "kss_icp_o2o_batch": 12, "kss_icp_o2o_batch_dev": 12}


def _header():
    return open(os.path.join(ROOT, "include", "kssicp.h")).read()


def test_header_declares_the_o2o_entry_points():
    hdr = _header()
    assert re.search(r"#define\s+KSS_O2O_NINFO\s+5\b", hdr)
    assert re.search(r"double\s*\*\s*trace_o2o\s*;", hdr)
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(kss_[a-z0-9_]+)\s*\(", hdr))
    assert [n for n in NAMES if n not in declared] == []
    assert "kss_o2o_params" in hdr


def test_header_says_what_is_not_offered():
    text = " ".join(_header().split())
    m = re.search(r"one-to-one ICP.*?Not offered: ([^/]*?)\*/", text)
    assert m
    for word in ("robust", "generalized", "symmetric", "similarity", "reciprocal", "mirror classes", "CLI"):
        assert word in m.group(1), word


def test_library_exports_and_binding_lists_them(pkg):
    exported = set(pkg.exported_symbols())
    assert [n for n in NAMES if n not in exported] == []
    assert [n for n in NAMES if n not in pkg.binding.SYMBOLS] == []
    L = pkg.load_library()
    for n, nargs in NAMES.items():
        assert len(getattr(L, n).argtypes) == nargs, n          # the binding declares its signature
    for m in ("o2o_filter", "o2o_filter_dev", "o2o_filter_batch", "icp_o2o", "icp_o2o_dev", "icp_o2o_batch", "icp_o2o_batch_dev"):
        assert callable(getattr(pkg.Context, m))
    assert callable(pkg.o2o_params)
    assert [f[0] for f in pkg.O2oParams._fields_] == ["overlap", "metric", "trace_o2o"]


def test_null_context_needs_no_device(pkg):
    L = pkg.load_library()
    assert L.kss_o2o_filter(None, None, None, 1, 1, 1.0, None, None, None) == -1
    assert L.kss_o2o_filter_dev(None, None, None, 1, 1, 1.0, None, None, None) == -1
    assert L.kss_o2o_filter_batch(None, None, None, None, None, 1, 1.0, None, None, None) == -1
    assert L.kss_o2o_filter_batch_dev(None, None, None, None, None, 1, 1.0, None, None, None) == -1
    assert L.kss_icp_o2o(None, None, 1, None, 1, None, None, None, None, None) == -1
    assert L.kss_icp_o2o_dev(None, None, 1, None, 1, None, None, None, None, None) == -1
    assert L.kss_icp_o2o_batch(None, None, None, None, None, None, 1, None, None, None, None, None) == -1
    assert L.kss_icp_o2o_batch_dev(None, None, None, None, None, None, 1, None, None, None, None, None) == -1
