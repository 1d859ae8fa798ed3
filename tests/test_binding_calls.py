"""What every pair-metric method of binding.Context hands to its C symbol, without a GPU.

A recording proxy stands in for libkssicp.so (Context(lib=proxy)): it forwards the host-only kss_*_default_params,
kss_status_string and kss_last_error to the real library, records every other kss_* call and returns 0 (or the status it was
told to).  The transcript of every method -- once with every optional argument given, once with all of them defaulted -- is
compared with tests/golden/binding_calls.json, which was recorded by this file's __main__ from the binding.py of the commit
before the methods were folded onto one call path, never from the code under test:

    python tests/test_binding_calls.py path/to/binding.py [out.json]
"""
import ctypes as C
import importlib.util
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "binding_calls.json")
FORWARD = ("kss_status_string", "kss_last_error")
DEV = {"d_src": 0x10000, "d_tgt": 0x20000, "d_nrm": 0x30000, "d_snrm": 0x40000, "d_idx": 0x50000, "d_d2": 0x60000,
       "d_idx_out": 0x70000, "d_d2_out": 0x80000, "vmap": 0x90000}


def _is_ptr(t):
    return t is C.c_void_p or issubclass(t, (C._Pointer, C._CFuncPtr))


def _ptr_fields(st):
    return [f for f, t in st._fields_ if _is_ptr(t)]


class Proxy:
    """Stands in for the loaded library: see the module's docstring."""

    def __init__(self, real, names):
        self.real, self.names, self.rc = real, names, 0
        self.calls, self.structs, self.faults = [], [], []

    def __getattr__(self, name):
        if not name.startswith("kss_"):
            raise AttributeError(name)
        if name in FORWARD or name.endswith("_default_params"):
            return getattr(self.real, name)

        def call(*args):
            fn = getattr(self.real, name)
            if len(args) != len(fn.argtypes):
                self.faults.append("%s: %d arguments for %d argtypes" % (name, len(args), len(fn.argtypes)))
            for k, (a, t) in enumerate(zip(args, fn.argtypes)):
                try:
                    t.from_param(a)
                except Exception as e:  # noqa: BLE001
                    self.faults.append("%s: argument %d refused by %s: %s" % (name, k, t.__name__, e))
            self.calls.append({"symbol": name, "args": [self._norm(a) for a in args]})
            for a in args:
                st = getattr(a, "_obj", None)
                if isinstance(st, C.Structure):
                    self.structs.append(st)
                    if hasattr(st, "trace_n") and st.trace_n:
                        st.trace_n[0] = 1          # one traced pass comes back
            return self.rc
        return call

    def _addr(self, v):
        return None if not v else self.names.get(v, "fresh buffer")

    def _norm(self, a):
        if a is None or isinstance(a, (bool, int, float)):
            return a
        if isinstance(a, C.c_void_p):
            return self._addr(a.value)
        st = getattr(a, "_obj", None)              # byref(...)
        if isinstance(st, C.Structure):
            if type(st).__name__ == "IcpResult":
                return "byref IcpResult"
            out = {"byref": type(st).__name__}
            for f, t in st._fields_:
                v = getattr(st, f)
                out[f] = ("set" if v else None) if _is_ptr(t) else v
            return out
        if st is not None:
            return "byref " + type(st).__name__
        return "other " + type(a).__name__


class World:
    """The smallest inputs that tell the arguments apart: one pair of 5 sources and 7 targets, a ragged batch of 5 + 3 sources
    against 7 + 4 targets; float32 C-contiguous clouds and normals and int64 offsets, which the binding passes on as they are."""

    def __init__(self, mod, real):
        self.mod = mod
        rng = np.random.RandomState(5)
        f3 = lambda n: np.ascontiguousarray(rng.rand(n, 3), dtype=np.float32)  # noqa: E731
        self.bufs = {
            "src": f3(5), "tgt": f3(7), "nrm": f3(7), "snrm": f3(5), "idx": np.arange(5, dtype=np.int32),
            "d2": np.linspace(0.0, 0.4, 5).astype(np.float32), "Rn": np.eye(3, dtype=np.float32),
            "src_all": f3(8), "tgt_all": f3(11), "nrm_all": f3(11), "snrm_all": f3(8),
            "so": np.array([0, 5, 8], np.int64), "to": np.array([0, 7, 11], np.int64), "nts": np.array([7, 4], np.int64),
            "idx_all": np.arange(8, dtype=np.int32), "d2_all": np.linspace(0.0, 0.7, 8).astype(np.float32),
            "overlaps": np.array([0.5, 0.75]), "scales": np.array([0.0, 0.25]), "epsilons": np.array([1e-3, 2e-3]),
            "aligns": np.array([1, 0], np.int32),
        }
        names = {a.ctypes.data: k for k, a in self.bufs.items()}
        names.update({v: k for k, v in DEV.items()})
        self.__dict__.update(self.bufs)
        self.__dict__.update(DEV)
        self.proxy = Proxy(real, names)
        self.ctx = mod.Context(lib=self.proxy)
        self.map = mod.VoxelMap(self.ctx, C.c_void_p(DEV["vmap"]))
        self.owned = []

    def own(self, st):
        self.owned.append(st)
        return st

    def p(self):
        return self.own(self.ctx.icp_params(max_iterations=7))

    def sp(self):
        return self.own(self.mod.sim_params(overlap=0.75))

    def rp(self, metric=0):
        return self.own(self.mod.robust_params(self.mod.LOSS_CAUCHY, metric, tune=2.5))

    def gp(self):
        return self.own(self.mod.gicp_params(epsilon=2e-3))

    def sy(self):
        return self.own(self.mod.symm_params(align_normals=0))


def cases():
    """name -> (method, call with every optional argument given, call with all of them defaulted); w is the World, c its Context."""
    T = dict(trace_cap=2, fitness_corr=True)
    PL = 1   # METRIC_PLANE
    pair_dev = lambda w: (w.d_src, 5, w.d_tgt, 7)                                     # noqa: E731
    both_dev = lambda w: (w.d_src, 5, w.d_snrm, w.d_tgt, 7, w.d_nrm)                  # noqa: E731
    batch = lambda w: (w.src_all, w.so, w.tgt_all, w.to)                              # noqa: E731
    batch_dev = lambda w: (w.d_src, w.so, w.d_tgt, w.to)                              # noqa: E731
    bboth_dev = lambda w: (w.d_src, w.so, w.d_snrm, w.d_tgt, w.to, w.d_nrm)           # noqa: E731
    sums = lambda w: (w.src, w.snrm, w.tgt, w.nrm, w.idx)                             # noqa: E731
    sums_dev = lambda w: (w.d_src, w.d_snrm, w.d_tgt, w.d_nrm, w.d_idx, 5, 7)         # noqa: E731
    return {
        "icp": (lambda c, w: c.icp(w.src, w.tgt, params=w.p(), **T), lambda c, w: c.icp(w.src, w.tgt)),
        "p2l_sums": (lambda c, w: c.p2l_sums(w.src, w.tgt, w.nrm, w.idx, max_d2=0.5), lambda c, w: c.p2l_sums(w.src, w.tgt, w.nrm, w.idx)),
        "p2l_sums_dev": (lambda c, w: c.p2l_sums_dev(w.d_src, w.d_tgt, w.d_nrm, w.d_idx, 5, 7, max_d2=0.5),
                         lambda c, w: c.p2l_sums_dev(w.d_src, w.d_tgt, w.d_nrm, w.d_idx, 5, 7)),
        "icp_p2l": (lambda c, w: c.icp_p2l(w.src, w.tgt, normals=w.nrm, params=w.p(), **T), lambda c, w: c.icp_p2l(w.src, w.tgt)),
        "icp_p2l_dev": (lambda c, w: c.icp_p2l_dev(*pair_dev(w), w.d_nrm, w.p()), lambda c, w: c.icp_p2l_dev(*pair_dev(w), None, w.p())),
        "trim_threshold": (lambda c, w: c.trim_threshold(w.d2, max_d2=0.5, overlap=0.75), lambda c, w: c.trim_threshold(w.d2)),
        "trim_threshold_dev": (lambda c, w: c.trim_threshold_dev(w.d_d2, 5, max_d2=0.5, overlap=0.75),
                               lambda c, w: c.trim_threshold_dev(w.d_d2, 5)),
        "icp_trimmed": (lambda c, w: c.icp_trimmed(w.src, w.tgt, normals=w.nrm, overlap=0.75, metric=PL, params=w.p(), **T),
                        lambda c, w: c.icp_trimmed(w.src, w.tgt)),
        "icp_trimmed_dev": (lambda c, w: c.icp_trimmed_dev(*pair_dev(w), w.d_nrm, w.p(), overlap=0.75, metric=PL),
                            lambda c, w: c.icp_trimmed_dev(*pair_dev(w), 0, w.p())),
        "o2o_filter": (lambda c, w: c.o2o_filter(w.idx, w.d2, 7, max_d2=0.5, want_idx=True, want_d2=False, alias=True),
                       lambda c, w: c.o2o_filter(w.idx, w.d2, 7)),
        "o2o_filter_dev": (lambda c, w: c.o2o_filter_dev(w.d_idx, w.d_d2, 5, 7, max_d2=0.5, d_idx_out=w.d_idx_out, d_d2_out=w.d_d2_out),
                           lambda c, w: c.o2o_filter_dev(w.d_idx, w.d_d2, 5, 7)),
        "o2o_filter_batch": (lambda c, w: c.o2o_filter_batch(w.idx_all, w.d2_all, w.so, w.nts, max_d2=0.5),
                             lambda c, w: c.o2o_filter_batch(w.idx_all, w.d2_all, w.so, w.nts)),
        "icp_o2o": (lambda c, w: c.icp_o2o(w.src, w.tgt, normals=w.nrm, overlap=0.75, metric=PL, params=w.p(), **T),
                    lambda c, w: c.icp_o2o(w.src, w.tgt)),
        "icp_o2o_dev": (lambda c, w: c.icp_o2o_dev(*pair_dev(w), w.d_nrm, w.p(), overlap=0.75, metric=PL),
                        lambda c, w: c.icp_o2o_dev(*pair_dev(w), None, w.p())),
        "recip_filter": (lambda c, w: c.recip_filter(w.src, w.tgt, w.idx, w.d2, max_d2=0.5, nn_fma=1, want_idx=False, want_d2=True, alias=True),
                         lambda c, w: c.recip_filter(w.src, w.tgt, w.idx, w.d2)),
        "recip_filter_dev": (lambda c, w: c.recip_filter_dev(*pair_dev(w), w.d_idx, w.d_d2, max_d2=0.5, nn_fma=1, d_idx_out=w.d_idx_out,
                                                             d_d2_out=w.d_d2_out),
                             lambda c, w: c.recip_filter_dev(*pair_dev(w), w.d_idx, w.d_d2)),
        "icp_recip": (lambda c, w: c.icp_recip(w.src, w.tgt, normals=w.nrm, overlap=0.75, metric=PL, params=w.p(), **T),
                      lambda c, w: c.icp_recip(w.src, w.tgt)),
        "icp_recip_dev": (lambda c, w: c.icp_recip_dev(*pair_dev(w), w.d_nrm, w.p(), overlap=0.75, metric=PL),
                          lambda c, w: c.icp_recip_dev(*pair_dev(w), None, w.p())),
        "sim_sums": (lambda c, w: c.sim_sums(w.src, w.tgt, w.idx, max_d2=0.5), lambda c, w: c.sim_sums(w.src, w.tgt, w.idx)),
        "sim_sums_dev": (lambda c, w: c.sim_sums_dev(w.d_src, w.d_tgt, w.d_idx, 5, 7, max_d2=0.5),
                         lambda c, w: c.sim_sums_dev(w.d_src, w.d_tgt, w.d_idx, 5, 7)),
        "icp_sim": (lambda c, w: c.icp_sim(w.src, w.tgt, sp=w.sp(), params=w.p(), **T), lambda c, w: c.icp_sim(w.src, w.tgt)),
        "icp_sim_dev": (lambda c, w: c.icp_sim_dev(*pair_dev(w), w.p(), sp=w.sp()), lambda c, w: c.icp_sim_dev(*pair_dev(w), w.p())),
        "robust_sums": (lambda c, w: c.robust_sums(w.src, w.tgt, w.nrm, w.idx, max_d2=0.5, rp=w.rp(PL)),
                        lambda c, w: c.robust_sums(w.src, w.tgt, None, w.idx)),
        "robust_sums_loss": (lambda c, w: c.robust_sums(w.src, w.tgt, w.nrm, w.idx, loss=2, metric=PL), None),
        "robust_sums_dev": (lambda c, w: c.robust_sums_dev(w.d_src, w.d_tgt, w.d_nrm, w.d_idx, 5, 7, max_d2=0.5, rp=w.rp(PL)),
                            lambda c, w: c.robust_sums_dev(w.d_src, w.d_tgt, None, w.d_idx, 5, 7)),
        "robust_sums_dev_loss": (lambda c, w: c.robust_sums_dev(w.d_src, w.d_tgt, w.d_nrm, w.d_idx, 5, 7, loss=2, metric=PL), None),
        "icp_robust": (lambda c, w: c.icp_robust(w.src, w.tgt, normals=w.nrm, rp=w.rp(PL), params=w.p(), **T),
                       lambda c, w: c.icp_robust(w.src, w.tgt)),
        "icp_robust_loss": (lambda c, w: c.icp_robust(w.src, w.tgt, normals=w.nrm, loss=2, metric=PL, trace_cap=2), None),
        "icp_robust_dev": (lambda c, w: c.icp_robust_dev(*pair_dev(w), w.d_nrm, w.p(), rp=w.rp(PL)),
                           lambda c, w: c.icp_robust_dev(*pair_dev(w), None, w.p())),
        "icp_robust_dev_loss": (lambda c, w: c.icp_robust_dev(*pair_dev(w), w.d_nrm, w.p(), loss=2, metric=PL), None),
        "gicp_sums": (lambda c, w: c.gicp_sums(*sums(w), max_d2=0.5, Rn=w.Rn, gp=w.gp()), lambda c, w: c.gicp_sums(w.src, None, w.tgt, None, w.idx)),
        "gicp_sums_dev": (lambda c, w: c.gicp_sums_dev(*sums_dev(w), max_d2=0.5, Rn=w.Rn, gp=w.gp()),
                          lambda c, w: c.gicp_sums_dev(w.d_src, None, w.d_tgt, 0, w.d_idx, 5, 7)),
        "icp_gicp": (lambda c, w: c.icp_gicp(w.src, w.tgt, src_normals=w.snrm, tgt_normals=w.nrm, gp=w.gp(), params=w.p(), **T),
                     lambda c, w: c.icp_gicp(w.src, w.tgt)),
        "icp_gicp_dev": (lambda c, w: c.icp_gicp_dev(*both_dev(w), w.p(), gp=w.gp()),
                         lambda c, w: c.icp_gicp_dev(w.d_src, 5, None, w.d_tgt, 7, None, w.p())),
        "vmap": (lambda c, w: c.vmap(w.tgt, 0.25, normals=w.nrm, normals_k=12), lambda c, w: c.vmap(w.tgt, 0.25)),
        "vmap_dev": (lambda c, w: c.vmap_dev(w.d_tgt, 7, 0.25, d_normals=w.d_nrm, normals_k=12), lambda c, w: c.vmap_dev(w.d_tgt, 7, 0.25)),
        "vgicp_sums": (lambda c, w: c.vgicp_sums(w.src, w.snrm, w.map, max_d2=0.5, Rn=w.Rn, gp=w.gp()),
                       lambda c, w: c.vgicp_sums(w.src, None, w.map)),
        "vgicp_sums_nomap": (lambda c, w: c.vgicp_sums(w.src, None, None), None),
        "vgicp_sums_dev": (lambda c, w: c.vgicp_sums_dev(w.d_src, w.d_snrm, 5, w.map, max_d2=0.5, Rn=w.Rn, gp=w.gp()),
                           lambda c, w: c.vgicp_sums_dev(w.d_src, None, 5, w.map)),
        "icp_vgicp": (lambda c, w: c.icp_vgicp(w.src, w.map, src_normals=w.snrm, gp=w.gp(), params=w.p(), trace_cap=2),
                      lambda c, w: c.icp_vgicp(w.src, w.map)),
        "icp_vgicp_nomap": (lambda c, w: c.icp_vgicp(w.src, None), None),
        "icp_vgicp_dev": (lambda c, w: c.icp_vgicp_dev(w.d_src, 5, w.d_snrm, w.map, w.p(), gp=w.gp()),
                          lambda c, w: c.icp_vgicp_dev(w.d_src, 5, None, w.map, w.p())),
        "symm_sums": (lambda c, w: c.symm_sums(*sums(w), max_d2=0.5, Rn=w.Rn, sp=w.sy()), lambda c, w: c.symm_sums(w.src, None, w.tgt, None, w.idx)),
        "symm_sums_dev": (lambda c, w: c.symm_sums_dev(*sums_dev(w), max_d2=0.5, Rn=w.Rn, sp=w.sy()),
                          lambda c, w: c.symm_sums_dev(w.d_src, None, w.d_tgt, 0, w.d_idx, 5, 7)),
        "icp_symm": (lambda c, w: c.icp_symm(w.src, w.tgt, src_normals=w.snrm, tgt_normals=w.nrm, sp=w.sy(), params=w.p(), **T),
                     lambda c, w: c.icp_symm(w.src, w.tgt)),
        "icp_symm_dev": (lambda c, w: c.icp_symm_dev(*both_dev(w), w.p(), sp=w.sy()),
                         lambda c, w: c.icp_symm_dev(w.d_src, 5, None, w.d_tgt, 7, None, w.p())),
        "symm_robust_sums": (lambda c, w: c.symm_robust_sums(*sums(w), max_d2=0.5, Rn=w.Rn, sp=w.sy(), rp=w.rp(PL)),
                             lambda c, w: c.symm_robust_sums(w.src, None, w.tgt, None, w.idx)),
        "symm_robust_sums_loss": (lambda c, w: c.symm_robust_sums(*sums(w), loss=1), None),
        "symm_robust_sums_dev": (lambda c, w: c.symm_robust_sums_dev(*sums_dev(w), max_d2=0.5, Rn=w.Rn, sp=w.sy(), rp=w.rp(PL)),
                                 lambda c, w: c.symm_robust_sums_dev(w.d_src, None, w.d_tgt, 0, w.d_idx, 5, 7)),
        "symm_robust_sums_dev_loss": (lambda c, w: c.symm_robust_sums_dev(*sums_dev(w), loss=1), None),
        "icp_symm_robust": (lambda c, w: c.icp_symm_robust(w.src, w.tgt, src_normals=w.snrm, tgt_normals=w.nrm, sp=w.sy(), rp=w.rp(PL),
                                                           params=w.p(), **T),
                            lambda c, w: c.icp_symm_robust(w.src, w.tgt)),
        "icp_symm_robust_loss": (lambda c, w: c.icp_symm_robust(w.src, w.tgt, loss=1, trace_cap=2), None),
        "icp_symm_robust_dev": (lambda c, w: c.icp_symm_robust_dev(*both_dev(w), w.p(), sp=w.sy(), rp=w.rp(PL)),
                                lambda c, w: c.icp_symm_robust_dev(w.d_src, 5, None, w.d_tgt, 7, None, w.p())),
        "icp_symm_robust_dev_loss": (lambda c, w: c.icp_symm_robust_dev(*both_dev(w), w.p(), loss=1), None),
        "icp_p2l_batch": (lambda c, w: c.icp_p2l_batch(*batch(w), normals_all=w.nrm_all, params=w.p(), **T),
                          lambda c, w: c.icp_p2l_batch(*batch(w))),
        "icp_p2l_batch_dev": (lambda c, w: c.icp_p2l_batch_dev(*batch_dev(w), w.d_nrm, w.p()),
                              lambda c, w: c.icp_p2l_batch_dev(*batch_dev(w), None, w.p())),
        "icp_trimmed_batch": (lambda c, w: c.icp_trimmed_batch(*batch(w), normals_all=w.nrm_all, overlaps=w.overlaps, overlap=0.75, metric=PL,
                                                               params=w.p(), **T),
                              lambda c, w: c.icp_trimmed_batch(*batch(w))),
        "icp_trimmed_batch_dev": (lambda c, w: c.icp_trimmed_batch_dev(*batch_dev(w), w.d_nrm, w.p(), overlaps=w.overlaps, overlap=0.75, metric=PL),
                                  lambda c, w: c.icp_trimmed_batch_dev(*batch_dev(w), None, w.p())),
        "icp_o2o_batch": (lambda c, w: c.icp_o2o_batch(*batch(w), normals_all=w.nrm_all, overlaps=w.overlaps, overlap=0.75, metric=PL,
                                                       params=w.p(), **T),
                          lambda c, w: c.icp_o2o_batch(*batch(w))),
        "icp_o2o_batch_dev": (lambda c, w: c.icp_o2o_batch_dev(*batch_dev(w), w.d_nrm, w.p(), overlaps=w.overlaps, overlap=0.75, metric=PL),
                              lambda c, w: c.icp_o2o_batch_dev(*batch_dev(w), None, w.p())),
        "recip_filter_batch": (lambda c, w: c.recip_filter_batch(w.src_all, w.so, w.tgt_all, w.to, w.idx_all, w.d2_all, max_d2=0.5, nn_fma=1),
                               lambda c, w: c.recip_filter_batch(w.src_all, w.so, w.tgt_all, w.to, w.idx_all, w.d2_all)),
        "recip_filter_batch_dev": (lambda c, w: c.recip_filter_batch_dev(*batch_dev(w), w.d_idx, w.d_d2, max_d2=0.5, nn_fma=1,
                                                                         d_idx_out_all=w.d_idx_out, d_d2_out_all=w.d_d2_out),
                                   lambda c, w: c.recip_filter_batch_dev(*batch_dev(w), w.d_idx, w.d_d2)),
        "icp_recip_batch": (lambda c, w: c.icp_recip_batch(*batch(w), normals_all=w.nrm_all, overlaps=w.overlaps, overlap=0.75, metric=PL,
                                                           params=w.p(), **T),
                            lambda c, w: c.icp_recip_batch(*batch(w))),
        "icp_recip_batch_dev": (lambda c, w: c.icp_recip_batch_dev(*batch_dev(w), w.d_nrm, w.p(), overlaps=w.overlaps, overlap=0.75, metric=PL),
                                lambda c, w: c.icp_recip_batch_dev(*batch_dev(w), None, w.p())),
        "icp_sim_batch": (lambda c, w: c.icp_sim_batch(*batch(w), overlaps=w.overlaps, sp=w.sp(), params=w.p(), **T),
                          lambda c, w: c.icp_sim_batch(*batch(w))),
        "icp_sim_batch_dev": (lambda c, w: c.icp_sim_batch_dev(*batch_dev(w), w.p(), overlaps=w.overlaps, sp=w.sp()),
                              lambda c, w: c.icp_sim_batch_dev(*batch_dev(w), w.p())),
        "icp_robust_batch": (lambda c, w: c.icp_robust_batch(*batch(w), normals_all=w.nrm_all, rp=w.rp(PL), scales=w.scales, params=w.p(), **T),
                             lambda c, w: c.icp_robust_batch(*batch(w))),
        "icp_robust_batch_loss": (lambda c, w: c.icp_robust_batch(*batch(w), normals_all=w.nrm_all, loss=2, metric=PL, trace_cap=2), None),
        "icp_robust_batch_dev": (lambda c, w: c.icp_robust_batch_dev(*batch_dev(w), w.d_nrm, w.p(), rp=w.rp(PL), scales=w.scales),
                                 lambda c, w: c.icp_robust_batch_dev(*batch_dev(w), None, w.p())),
        "icp_robust_batch_dev_loss": (lambda c, w: c.icp_robust_batch_dev(*batch_dev(w), w.d_nrm, w.p(), loss=2, metric=PL), None),
        "icp_gicp_batch": (lambda c, w: c.icp_gicp_batch(*batch(w), src_normals_all=w.snrm_all, tgt_normals_all=w.nrm_all, epsilons=w.epsilons,
                                                         gp=w.gp(), params=w.p(), **T),
                           lambda c, w: c.icp_gicp_batch(*batch(w))),
        "icp_gicp_batch_dev": (lambda c, w: c.icp_gicp_batch_dev(*bboth_dev(w), params=w.p(), epsilons=w.epsilons, gp=w.gp(), trace_cap=2),
                               lambda c, w: c.icp_gicp_batch_dev(w.d_src, w.so, None, w.d_tgt, w.to, None)),
        "icp_symm_batch": (lambda c, w: c.icp_symm_batch(*batch(w), src_normals_all=w.snrm_all, tgt_normals_all=w.nrm_all, aligns=w.aligns,
                                                         sp=w.sy(), params=w.p(), **T),
                           lambda c, w: c.icp_symm_batch(*batch(w))),
        "icp_symm_batch_dev": (lambda c, w: c.icp_symm_batch_dev(*bboth_dev(w), params=w.p(), aligns=w.aligns, sp=w.sy(), trace_cap=2),
                               lambda c, w: c.icp_symm_batch_dev(w.d_src, w.so, None, w.d_tgt, w.to, None)),
        "icp_symm_robust_batch": (lambda c, w: c.icp_symm_robust_batch(*batch(w), src_normals_all=w.snrm_all, tgt_normals_all=w.nrm_all,
                                                                       aligns=w.aligns, scales=w.scales, sp=w.sy(), rp=w.rp(PL), params=w.p(), **T),
                                  lambda c, w: c.icp_symm_robust_batch(*batch(w))),
        "icp_symm_robust_batch_loss": (lambda c, w: c.icp_symm_robust_batch(*batch(w), loss=1, trace_cap=2), None),
        "icp_symm_robust_batch_dev": (lambda c, w: c.icp_symm_robust_batch_dev(*bboth_dev(w), params=w.p(), aligns=w.aligns, scales=w.scales,
                                                                               sp=w.sy(), rp=w.rp(PL), trace_cap=2),
                                      lambda c, w: c.icp_symm_robust_batch_dev(w.d_src, w.so, None, w.d_tgt, w.to, None)),
        "icp_symm_robust_batch_dev_loss": (lambda c, w: c.icp_symm_robust_batch_dev(*bboth_dev(w), loss=1), None),
        "trim_threshold_batch": (lambda c, w: c.trim_threshold_batch(w.d2_all, w.so, w.overlaps, max_d2=0.5),
                                 lambda c, w: c.trim_threshold_batch(w.d2_all, w.so, None)),
        "trim_threshold_batch_dev": (lambda c, w: c.trim_threshold_batch_dev(w.d_d2, w.so, w.overlaps, max_d2=0.5),
                                     lambda c, w: c.trim_threshold_batch_dev(w.d_d2, w.so, None)),
    }


def symbol_of(case):
    """The C symbol a case's method has to call: kss_<method>, but for the voxel map's constructors and the many-pairs form of
    reciprocal ICP, which is spelled _pairs (include/kssicp.h)."""
    m = case
    for tail in ("_loss", "_nomap"):
        if m.endswith(tail):
            m = m[:-len(tail)]
    return {"vmap": "kss_vmap_create", "vmap_dev": "kss_vmap_create_dev", "icp_recip_batch": "kss_icp_recip_pairs",
            "icp_recip_batch_dev": "kss_icp_recip_pairs_dev"}.get(m, "kss_" + m)


def shape_of(v):
    """The structure of a returned value: tuple arity, dictionary keys, array shapes and dtypes, list against ctypes array."""
    if isinstance(v, dict):
        return {"dict": {k: shape_of(v[k]) for k in sorted(v)}}
    if isinstance(v, tuple):
        return {"tuple": [shape_of(x) for x in v]}
    if isinstance(v, list):
        return {"list": [shape_of(x) for x in v]}
    if isinstance(v, np.ndarray):
        return {"ndarray": list(v.shape), "dtype": str(v.dtype)}
    if isinstance(v, C.Array):
        return {"ctypes array": type(v)._type_.__name__, "len": len(v)}
    return None if v is None else type(v).__name__


def run(w, call, rc=0):
    """One call through the proxy: (the compute calls it made, what it returned or raised, the structs to look at afterwards)."""
    w.proxy.rc, w.proxy.calls, w.proxy.structs, w.owned = rc, [], [], []
    try:
        out = shape_of(call(w.ctx, w))
    except w.mod.KssError as e:
        out = "KssError %d" % e.status
    finally:
        w.proxy.rc = 0
    return w.proxy.calls, out, w.owned + w.proxy.structs


def record(mod, real):
    """The transcript of every case, {case: {"full" / "default": {"symbol", "args", "returns"}}}, and what was wrong with the shape
    of its calls, {case: [text, ...]}: not exactly one compute call, an argument count that is not the symbol's, an argument its
    argtype refuses."""
    w = World(mod, real)
    book, problems = {}, {}
    for name, pair in cases().items():
        book[name], problems[name] = {}, []
        for kind, call in zip(("full", "default"), pair):
            if call is None:
                continue
            w.proxy.faults = []
            calls, out, _ = run(w, call)
            problems[name] += ["%s: %s" % (kind, f) for f in w.proxy.faults]
            if len(calls) != 1:
                problems[name].append("%s: %d compute calls %s" % (kind, len(calls), [c["symbol"] for c in calls]))
            book[name][kind] = dict(calls[0], returns=out) if calls else {"returns": out}
    return book, problems


@pytest.fixture(scope="module")
def world(pkg):
    return World(pkg.binding, pkg.load_library())


@pytest.fixture(scope="module")
def recorded(pkg):
    return record(pkg.binding, pkg.load_library())


@pytest.fixture(scope="module")
def book(recorded):
    return recorded[0]


def test_every_pair_metric_method_is_covered(pkg):
    """Every public method of Context between icp() and trim_threshold_batch_dev() has its case."""
    src = open(pkg.binding.__file__.replace(".pyc", ".py")).read()
    body = src[src.index("    def icp(self"):src.index("    def icp_dev(self")]
    methods = [ln.split("def ")[1].split("(")[0] for ln in body.splitlines() if ln.startswith("    def ")]
    public = [m for m in methods if not m.startswith("_")]
    assert len(public) >= 66
    assert sorted(set(public) - set(cases())) == []


@pytest.mark.parametrize("name", sorted(cases()))
def test_call_shape(recorded, name):
    """One compute call, to the method's own symbol, with as many arguments as the symbol declares, each accepted by its argtype."""
    book, problems = recorded
    assert problems[name] == []
    for kind, rec in book[name].items():
        assert rec["symbol"] == symbol_of(name), (name, kind)


@pytest.mark.parametrize("name", sorted(cases()))
def test_transcript_and_return_shape(book, name):
    golden = json.load(open(FIXTURE))
    assert book[name] == golden[name]


def test_transcript_has_no_case_the_fixture_lacks(book):
    assert sorted(book) == sorted(json.load(open(FIXTURE)))


@pytest.mark.parametrize("rc", [0, -1])
@pytest.mark.parametrize("name", sorted(cases()))
def test_detach(world, name, rc):
    """After the call -- returned, or raised as KssError -- no params struct still points at the call's arrays: the caller's
    IcpParams and metric struct, and the ones the method made itself (TrimParams among them), as the library saw them."""
    calls, out, structs = run(world, cases()[name][0], rc)
    assert len(calls) == 1
    assert (out == "KssError -1") == (rc != 0)
    for st in structs:
        assert [f for f in _ptr_fields(st) if getattr(st, f)] == [], (name, type(st).__name__)
        if hasattr(st, "trace_cap"):
            assert st.trace_cap == 0


def test_value_errors(world):
    """The binding's own refusals, with their texts."""
    c, w = world.ctx, world
    target = "normals must have one row per target point"
    for call in (lambda: c.icp_p2l(w.src, w.tgt, normals=w.snrm), lambda: c.icp_trimmed(w.src, w.tgt, normals=w.snrm),
                 lambda: c.icp_o2o(w.src, w.tgt, normals=w.snrm), lambda: c.icp_recip(w.src, w.tgt, normals=w.snrm),
                 lambda: c.icp_robust(w.src, w.tgt, normals=w.snrm), lambda: c.icp_p2l_batch(w.src_all, w.so, w.tgt_all, w.to, w.snrm_all),
                 lambda: c.icp_trimmed_batch(w.src_all, w.so, w.tgt_all, w.to, w.snrm_all),
                 lambda: c.icp_o2o_batch(w.src_all, w.so, w.tgt_all, w.to, w.snrm_all),
                 lambda: c.icp_recip_batch(w.src_all, w.so, w.tgt_all, w.to, w.snrm_all),
                 lambda: c.icp_robust_batch(w.src_all, w.so, w.tgt_all, w.to, w.snrm_all)):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == target
    both = [lambda **k: c.gicp_sums(w.src, k.get("s"), w.tgt, k.get("t"), w.idx), lambda **k: c.icp_gicp(w.src, w.tgt, k.get("s"), k.get("t")),
            lambda **k: c.symm_sums(w.src, k.get("s"), w.tgt, k.get("t"), w.idx), lambda **k: c.icp_symm(w.src, w.tgt, k.get("s"), k.get("t")),
            lambda **k: c.symm_robust_sums(w.src, k.get("s"), w.tgt, k.get("t"), w.idx),
            lambda **k: c.icp_symm_robust(w.src, w.tgt, k.get("s"), k.get("t")),
            lambda **k: c.icp_gicp_batch(w.src_all, w.so, w.tgt_all, w.to, k.get("s"), k.get("t")),
            lambda **k: c.icp_symm_batch(w.src_all, w.so, w.tgt_all, w.to, k.get("s"), k.get("t")),
            lambda **k: c.icp_symm_robust_batch(w.src_all, w.so, w.tgt_all, w.to, k.get("s"), k.get("t"))]
    for call, text in ((lambda: c.vgicp_sums(w.src, w.nrm, w.map), "source"), (lambda: c.icp_vgicp(w.src, w.map, w.nrm), "source"),
                       (lambda: c.vmap(w.tgt, 0.25, normals=w.snrm), "target")):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == text + " normals must have one row per point"
    for call in both:
        with pytest.raises(ValueError) as e:
            call(s=w.nrm_all)
        assert str(e.value) == "source normals must have one row per point"
        with pytest.raises(ValueError) as e:
            call(t=w.snrm)
        assert str(e.value) == "target normals must have one row per point"
    three = np.zeros(3)
    per_pair = {"overlaps": [lambda: c.icp_trimmed_batch(w.src_all, w.so, w.tgt_all, w.to, overlaps=three),
                             lambda: c.icp_trimmed_batch_dev(w.d_src, w.so, w.d_tgt, w.to, None, w.p(), overlaps=three),
                             lambda: c.icp_o2o_batch(w.src_all, w.so, w.tgt_all, w.to, overlaps=three),
                             lambda: c.icp_o2o_batch_dev(w.d_src, w.so, w.d_tgt, w.to, None, w.p(), overlaps=three),
                             lambda: c.icp_recip_batch(w.src_all, w.so, w.tgt_all, w.to, overlaps=three),
                             lambda: c.icp_recip_batch_dev(w.d_src, w.so, w.d_tgt, w.to, None, w.p(), overlaps=three),
                             lambda: c.icp_sim_batch(w.src_all, w.so, w.tgt_all, w.to, overlaps=three),
                             lambda: c.icp_sim_batch_dev(w.d_src, w.so, w.d_tgt, w.to, w.p(), overlaps=three),
                             lambda: c.trim_threshold_batch(w.d2_all, w.so, three), lambda: c.trim_threshold_batch_dev(w.d_d2, w.so, three)],
                "scales": [lambda: c.icp_robust_batch(w.src_all, w.so, w.tgt_all, w.to, scales=three),
                           lambda: c.icp_robust_batch_dev(w.d_src, w.so, w.d_tgt, w.to, None, w.p(), scales=three),
                           lambda: c.icp_symm_robust_batch(w.src_all, w.so, w.tgt_all, w.to, scales=three),
                           lambda: c.icp_symm_robust_batch_dev(w.d_src, w.so, None, w.d_tgt, w.to, None, scales=three)],
                "epsilons": [lambda: c.icp_gicp_batch(w.src_all, w.so, w.tgt_all, w.to, epsilons=three),
                             lambda: c.icp_gicp_batch_dev(w.d_src, w.so, None, w.d_tgt, w.to, None, epsilons=three)],
                "aligns": [lambda: c.icp_symm_batch(w.src_all, w.so, w.tgt_all, w.to, aligns=three),
                           lambda: c.icp_symm_batch_dev(w.d_src, w.so, None, w.d_tgt, w.to, None, aligns=three),
                           lambda: c.icp_symm_robust_batch(w.src_all, w.so, w.tgt_all, w.to, aligns=three),
                           lambda: c.icp_symm_robust_batch_dev(w.d_src, w.so, None, w.d_tgt, w.to, None, aligns=three)]}
    for noun, calls in per_pair.items():
        for call in calls:
            with pytest.raises(ValueError) as e:
                call()
            assert str(e.value) == "%s must hold one entry per pair" % noun
    short = w.to[:2]
    for call in (lambda: c.icp_p2l_batch(w.src_all, w.so, w.tgt_all, short), lambda: c.icp_p2l_batch_dev(w.d_src, w.so, w.d_tgt, short, None, w.p()),
                 lambda: c.icp_trimmed_batch(w.src_all, w.so, w.tgt_all, short), lambda: c.icp_o2o_batch(w.src_all, w.so, w.tgt_all, short),
                 lambda: c.icp_recip_batch(w.src_all, w.so, w.tgt_all, short), lambda: c.icp_sim_batch(w.src_all, w.so, w.tgt_all, short),
                 lambda: c.icp_robust_batch(w.src_all, w.so, w.tgt_all, short), lambda: c.icp_gicp_batch(w.src_all, w.so, w.tgt_all, short),
                 lambda: c.icp_symm_batch_dev(w.d_src, w.so, None, w.d_tgt, short, None),
                 lambda: c.icp_symm_robust_batch(w.src_all, w.so, w.tgt_all, short),
                 lambda: c.recip_filter_batch(w.src_all, w.so, w.tgt_all, short, w.idx_all, w.d2_all),
                 lambda: c.recip_filter_batch_dev(w.d_src, w.so, w.d_tgt, short, w.d_idx, w.d_d2)):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == "src_off and tgt_off must hold npairs + 1 entries each"


def test_vgicp_dev_wants_a_map(world):
    """The host form passes a missing map on as NULL (the fixture's *_nomap cases); the _dev forms never did."""
    with pytest.raises(AttributeError):
        world.ctx.icp_vgicp_dev(world.d_src, 5, None, None, world.p())
    with pytest.raises(AttributeError):
        world.ctx.vgicp_sums_dev(world.d_src, None, 5, None)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    import __graft_entry__ as graft
    package = graft.load_package()
    if not os.path.exists(package.lib_path()):
        package.build_library()
    spec = importlib.util.spec_from_file_location("binding_under_record", os.path.abspath(sys.argv[1]))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    module._LIB = module._declare(C.CDLL(package.lib_path()))      # its own struct classes in the argtypes, the product's library
    with open(sys.argv[2] if len(sys.argv) > 2 else FIXTURE, "w") as f:
        transcript, wrong = record(module, module._LIB)
        assert not any(wrong.values()), wrong
        json.dump(transcript, f, indent=1, sort_keys=True)
        f.write("\n")
