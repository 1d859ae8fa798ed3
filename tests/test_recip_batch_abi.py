"""CPU test: the entry points of reciprocal ICP for many pairs per call -- the batched filter and the batched loop,
whose C symbols are spelled kss_icp_recip_pairs[_dev] -- are declared by the header, exported by the built library and listed by
the binding with their signatures, the Context methods carry the conventional _batch names, the header's reciprocal section names
the many-pairs form and no longer lists it as not built, and a null context is refused before anything touches a device (the
argument errors that need a context are in tests/test_gpu_recip_batch.py)."""
import ctypes as C
import os
import re

from conftest import ROOT

NAMES = {"kss_recip_filter_batch": 13, "kss_recip_filter_batch_dev": 13, "kss_icp_recip_pairs": 12, "kss_icp_recip_pairs_dev": 12}


def _header():
    return open(os.path.join(ROOT, "include", "kssicp.h")).read()


def test_header_declares_the_four_entry_points():
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = set(re.findall(r"\b(kss_[a-z0-9_]+)\s*\(", hdr))
    assert [n for n in NAMES if n not in declared] == []


def test_header_names_the_many_pairs_form_and_what_is_not_built():
    text = " ".join(_header().split())
    m = re.search(r"reciprocal ICP.*?Not built: ([^/]*?)\*/", text)
    assert m
    section, not_built = m.group(0), m.group(1)
    assert "Many pairs per call: kss_icp_recip_pairs" in section
    assert section.index("Many pairs per call: kss_icp_recip_pairs") < section.index("Not built:")
    # the batch is no longer listed as a function that is not built; the word stays for the forms that are not
    assert "kss_icp_recip_batch" not in not_built and "follow-up" not in not_built
    assert not re.match(r"the batch\b", not_built)
    assert "for one pair or a batch" in not_built
    # the spelling of the C symbol is explained where it is declared
    assert re.search(r"spelled _pairs because", text)


def test_library_exports_and_binding_lists_them(pkg):
    exported = set(pkg.exported_symbols())
    assert [n for n in NAMES if n not in exported] == []
    assert [n for n in NAMES if n not in pkg.binding.SYMBOLS] == []
    L = pkg.load_library()
    for n, nargs in NAMES.items():
        assert len(getattr(L, n).argtypes) == nargs, n          # the binding declares its signature
    for m in ("recip_filter_batch", "recip_filter_batch_dev", "icp_recip_batch", "icp_recip_batch_dev"):
        assert callable(getattr(pkg.Context, m))


def test_null_context_needs_no_device(pkg):
    L = pkg.load_library()
    assert L.kss_recip_filter_batch(None, None, None, None, None, 1, None, None, 1.0, 0, None, None, None) == -1
    assert L.kss_recip_filter_batch_dev(None, None, None, None, None, 1, None, None, 1.0, 0, None, None, None) == -1
    assert L.kss_icp_recip_pairs(None, None, None, None, None, None, 1, None, None, None, None, None) == -1
    assert L.kss_icp_recip_pairs_dev(None, None, None, None, None, None, 1, None, None, None, None, None) == -1
    # a null ctx is refused first, whatever else is given: valid clouds, offsets, parameters and outputs
    import numpy as np
    src, tgt = np.zeros((4, 3), np.float32), np.ones((3, 3), np.float32)
    so, to = np.array([0, 4], np.int64), np.array([0, 3], np.int64)
    idx, d2, info = np.zeros(4, np.int32), np.ones(4, np.float32), np.zeros(6)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    rp, p, res = pkg.recip_params(), pkg.binding.IcpParams(), pkg.IcpResult()
    L.kss_icp_default_params(C.byref(p))
    for f in (L.kss_icp_recip_pairs, L.kss_icp_recip_pairs_dev):
        assert f(None, vp(src), vp(so), vp(tgt), vp(to), None, 1, C.byref(p), C.byref(rp), None, C.cast(C.byref(res), C.c_void_p), vp(info)) == -1
    for f in (L.kss_recip_filter_batch, L.kss_recip_filter_batch_dev):
        assert f(None, vp(src), vp(so), vp(tgt), vp(to), 1, vp(idx), vp(d2), 1.0, 0, None, None, vp(info)) == -1
