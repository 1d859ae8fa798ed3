"""CPU test: the entry points of reciprocal ICP, the filter alone and the single-pair loop, are declared by the
header, exported by the built library and listed by the binding with their signatures and struct layout, the Context methods exist,
the header says what is not built, and a null context or null params are refused before anything touches a device (the argument
errors that need a context are in tests/test_gpu_recip.py)."""
import ctypes as C
import os
import re

from conftest import ROOT

NAMES = {"kss_recip_filter": 12, "kss_recip_filter_dev": 12, "kss_recip_default_params": 1, "kss_icp_recip": 10, "kss_icp_recip_dev": 10}


def _header():
    return open(os.path.join(ROOT, "include", "kssicp.h")).read()


def test_header_declares_the_recip_entry_points():
    hdr = _header()
    assert re.search(r"#define\s+KSS_RECIP_NINFO\s+6\b", hdr)
    assert re.search(r"double\s*\*\s*trace_recip\s*;", hdr)
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(kss_[a-z0-9_]+)\s*\(", hdr))
    assert [n for n in NAMES if n not in declared] == []
    assert "kss_recip_params" in hdr
    assert "kss_icp_recip_batch" not in declared          # the batch is the named follow-up


def test_header_states_the_definition_and_what_is_not_built():
    text = " ".join(_header().split())
    m = re.search(r"reciprocal ICP.*?Not built: ([^/]*?)\*/", text)
    assert m
    for word in ("batch", "robust", "generalized", "symmetric", "similarity", "mirror classes", "CLI"):
        assert word in m.group(1), word
    for word in ("rkey(k, j)", "existence statement", "0x7fc00000", "BIT FOR BIT"):
        assert word in m.group(0), word


def test_library_exports_and_binding_lists_them(pkg):
    exported = set(pkg.exported_symbols())
    assert [n for n in NAMES if n not in exported] == []
    assert [n for n in NAMES if n not in pkg.binding.SYMBOLS] == []
    L = pkg.load_library()
    for n, nargs in NAMES.items():
        assert len(getattr(L, n).argtypes) == nargs, n          # the binding declares its signature
    for m in ("recip_filter", "recip_filter_dev", "icp_recip", "icp_recip_dev"):
        assert callable(getattr(pkg.Context, m))
    assert pkg.RECIP_NINFO == 6


def test_struct_layout(pkg):
    P = pkg.RecipParams
    assert [f[0] for f in P._fields_] == ["overlap", "metric", "trace_recip"]
    assert (P.overlap.offset, P.metric.offset, P.trace_recip.offset, C.sizeof(P)) == (0, 8, 16, 24)
    # the three records that ride through the trimmed pass share one layout
    for other in (pkg.O2oParams, pkg.binding.TrimParams):
        assert C.sizeof(other) == C.sizeof(P) and [getattr(other, f[0]).offset for f in other._fields_] == [0, 8, 16]


def test_null_context_and_null_params_need_no_device(pkg):
    L = pkg.load_library()
    assert L.kss_recip_filter(None, None, 1, None, 1, None, None, 1.0, 0, None, None, None) == -1
    assert L.kss_recip_filter_dev(None, None, 1, None, 1, None, None, 1.0, 0, None, None, None) == -1
    assert L.kss_icp_recip(None, None, 1, None, 1, None, None, None, None, None) == -1
    assert L.kss_icp_recip_dev(None, None, 1, None, 1, None, None, None, None, None) == -1
    assert L.kss_recip_default_params(None) == -1
    # a null ctx is refused first, whatever else is given
    rp, p, res = pkg.recip_params(), pkg.binding.IcpParams(), pkg.IcpResult()
    L.kss_icp_default_params(C.byref(p))
    assert L.kss_icp_recip(None, None, 1, None, 1, None, C.byref(p), C.byref(rp), C.byref(res), None) == -1
