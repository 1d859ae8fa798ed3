"""CPU test: the entry points of similarity ICP, single pair and batch, are declared by the header, exported by
the built library and listed by the binding with their signatures, the Context methods exist, and a null context is refused before
anything touches a device."""
import os
import re

from conftest import ROOT

NAMES = {"kss_sim_default_params": 1, "kss_sim_from_sums": 5, "kss_sim_sums": 8, "kss_sim_sums_dev": 8, "kss_icp_sim": 9,
         "kss_icp_sim_dev": 9, "kss_icp_sim_batch": 11, "kss_icp_sim_batch_dev": 11}


def test_header_declares_the_sim_entry_points():
    hdr = open(os.path.join(ROOT, "include", "kssicp.h")).read()
    assert re.search(r"#define\s+KSS_SIM_NINFO\s+6\b", hdr)
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(kss_[a-z0-9_]+)\s*\(", hdr))
    assert [n for n in NAMES if n not in declared] == []


def test_library_exports_and_binding_lists_them(pkg):
    exported = set(pkg.exported_symbols())
    assert [n for n in NAMES if n not in exported] == []
    assert [n for n in NAMES if n not in pkg.binding.SYMBOLS] == []
    L = pkg.load_library()
    for n, nargs in NAMES.items():
        assert len(getattr(L, n).argtypes) == nargs, n          # the binding declares its signature
    for m in ("sim_sums", "sim_sums_dev", "icp_sim", "icp_sim_dev", "icp_sim_batch", "icp_sim_batch_dev"):
        assert callable(getattr(pkg.Context, m))
    assert callable(pkg.sim_from_sums) and callable(pkg.sim_params)


def test_null_context_needs_no_device(pkg):
    L = pkg.load_library()
    assert L.kss_sim_sums(None, None, None, None, 1, 1, 1.0, None) == -1
    assert L.kss_sim_sums_dev(None, None, None, None, 1, 1, 1.0, None) == -1
    assert L.kss_icp_sim(None, None, 1, None, 1, None, None, None, None) == -1
    assert L.kss_icp_sim_dev(None, None, 1, None, 1, None, None, None, None) == -1
    assert L.kss_icp_sim_batch(None, None, None, None, None, 1, None, None, None, None, None) == -1
    assert L.kss_icp_sim_batch_dev(None, None, None, None, None, 1, None, None, None, None, None) == -1
