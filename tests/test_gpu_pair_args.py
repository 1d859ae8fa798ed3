"""The argument errors of the 46 pair-metric entry points of the C ABI (p2l, trimmed, sim, robust, gicp, symm, symm_robust, o2o,
recip: *_sums, single pair and batch, host and _dev), pinned: for every entry one valid call on tiny clouds (8 x 7; batches of two
pairs, 8 x 7 and 5 x 6) and variants of it with exactly one fault each, plus one with two faults from different checks.  Every
variant asserts the status and the exact kss_last_error text.  The calls go through ctx.L raw: the binding's own ValueErrors would
mask the library's checks.

EXPECT below was written from a build of commit a125812 (the parent of the change that gave these entries one checked, staged
path) and records its behaviour as it was, quirks included:
- kss_icp_p2l answers "icp_p2l: null cloud" to a null cloud, its device twin "null argument";
- the family check speaks before the shared one (a bad family parameter wins over a null result), except where the batch shape
  is looked at first (sim, trimmed and o2o batches: "bad batch" comes first);
- a batch with an overlaps array does not look at the overlap of its parameters: out of range there, the call runs (OK);
- normals_k is checked only when a set of normals has to be computed: out of range with both sets given, the call runs (OK);
- kss_p2l_sums[_dev] has no "cloud too large" answer and kss_sim_sums / kss_robust_sums do not look at the indices, so those
  variants would reach a launch with sizes the buffers do not have: they are not cases here.
Every faulty case returns before a launch.  A value is a string (both twins), a (host, _dev) pair, or OK."""

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32 = np.float32
OK, ERR_ARG = 0, -1
BIG = 0x7fff0001
NAN, INF = float("nan"), float("inf")

# base name -> the arguments after the context, in the order of include/kssicp.h
ENTRIES = {
    "p2l_sums": "src tgt nrm idx n nt max_d2 sums",
    "sim_sums": "src tgt idx n nt max_d2 sums",
    "robust_sums": "src tgt nrm idx n nt max_d2 rp sums info",
    "gicp_sums": "src snrm tgt tnrm idx n nt max_d2 Rn gp sums",
    "symm_sums": "src snrm tgt tnrm idx n nt max_d2 Rn sp sums",
    "symm_robust_sums": "src snrm tgt tnrm idx n nt max_d2 Rn sp rp sums info",
    "icp_p2l": "src ns tgt nt nrm p res",
    "icp_trimmed": "src ns tgt nt nrm p tp res last_info",
    "icp_sim": "src ns tgt nt p simp res last_info",
    "icp_robust": "src ns tgt nt nrm p rp res last_info",
    "icp_gicp": "src ns snrm tgt nt tnrm p gp res",
    "icp_symm": "src ns snrm tgt nt tnrm p sp res",
    "icp_symm_robust": "src ns snrm tgt nt tnrm p sp rp res last_info",
    "icp_o2o": "src ns tgt nt nrm p op res last_info",
    "icp_recip": "src ns tgt nt nrm p rcp res last_info",
    "icp_p2l_batch": "src src_off tgt tgt_off nrm npairs p res",
    "icp_trimmed_batch": "src src_off tgt tgt_off nrm npairs p tp overlaps res info_all",
    "icp_sim_batch": "src src_off tgt tgt_off npairs p simp overlaps res info_all",
    "icp_robust_batch": "src src_off tgt tgt_off nrm npairs p rp scales res info_all",
    "icp_gicp_batch": "src src_off snrm tgt tgt_off tnrm npairs p gp epsilons res",
    "icp_symm_batch": "src src_off snrm tgt tgt_off tnrm npairs p sp aligns res",
    "icp_symm_robust_batch": "src src_off snrm tgt tgt_off tnrm npairs p sp aligns rp scales res info_all",
    "icp_o2o_batch": "src src_off tgt tgt_off nrm npairs p op overlaps res info_all",
}
SYMBOLS = ["kss_" + b + d for b in ENTRIES for d in ("", "_dev")]
assert len(SYMBOLS) == 46

DEVICE_ARGS = ("src", "tgt", "nrm", "snrm", "tnrm", "idx")          # device memory for a _dev entry
REQUIRED = ("src", "tgt", "idx", "sums", "info", "p", "res", "tp", "simp", "rp", "gp", "sp", "op", "rcp", "src_off", "tgt_off")
OVERLAP_PARAMS = ("tp", "simp", "op", "rcp")
METRIC_PARAMS = ("tp", "op", "rcp", "rp")


def _unit(rng, n):
    v = rng.standard_normal((n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)


def valid_args(pkg, L, base):
    """name -> value of the valid call: numpy arrays, ctypes structures, numbers (fresh for every call)."""
    B = pkg.binding
    rng = np.random.default_rng(5)
    batch = base.endswith("_batch")
    ns, nt = (13, 13) if batch else (8, 7)
    tgt = rng.uniform(-1, 1, (nt, 3)).astype(F32)
    src = (tgt[np.arange(ns) % nt] + rng.uniform(-0.02, 0.02, (ns, 3))).astype(F32)
    p = B.IcpParams()
    L.kss_icp_default_params(C.byref(p))
    p.max_iterations = 2
    rp = B.RobustParams()
    L.kss_robust_default_params(B.LOSS_HUBER, B.METRIC_PLANE, C.byref(rp))
    gp, sp, simp = B.GicpParams(), B.SymmParams(), B.SimParams()
    L.kss_gicp_default_params(C.byref(gp))
    L.kss_symm_default_params(C.byref(sp))
    L.kss_sim_default_params(C.byref(simp))
    simp.overlap = 0.9
    return {"src": src, "tgt": tgt, "nrm": _unit(rng, nt), "snrm": _unit(rng, ns), "tnrm": _unit(rng, nt),
            "idx": (np.arange(ns) % nt).astype(np.int32), "n": ns, "ns": ns, "nt": nt, "max_d2": 1.0, "Rn": None,
            "sums": np.zeros(64), "info": np.zeros(8), "last_info": np.zeros(8), "info_all": np.zeros(16),
            "src_off": np.array([0, 8, 13], np.int64), "tgt_off": np.array([0, 7, 13], np.int64), "npairs": 2,
            "overlaps": np.array([0.9, 0.8]), "scales": np.array([0.1, 0.0]), "epsilons": np.array([1e-3, 1e-2]),
            "aligns": np.array([1, 0], np.int32), "res": (B.IcpResult * 2)(),
            "p": p, "rp": rp, "gp": gp, "sp": sp, "simp": simp, "tp": B.TrimParams(0.9, B.METRIC_PLANE, None),
            "op": B.O2oParams(0.9, B.METRIC_PLANE, None), "rcp": B.RecipParams(0.9, B.METRIC_PLANE, None)}


_NOOP = None


def _allreduce(pkg):
    global _NOOP
    if _NOOP is None:
        _NOOP = pkg.binding.ALLREDUCE_FN(lambda user, buf, n: 0)   # (never called: every entry here refuses it)
    return _NOOP


def variants(pkg, base, host):
    """[(label, {argument or "struct.field": value})] of one entry; "c" stands for the context."""
    names = ENTRIES[base].split()
    has = lambda a: a in names   # noqa: E731
    batch, sums = base.endswith("_batch"), base.endswith("_sums")
    V = [("valid", {}), ("null c", {"c": None})]
    required = [a for a in names if a in REQUIRED or (a == "nrm" and base in ("p2l_sums", "robust_sums"))]
    V += [("null " + a, {a: None}) for a in required]
    for a in ("n", "ns", "nt"):
        if has(a):
            V.append((a + " 0", {a: 0}))
            if base != "p2l_sums":
                V.append((a + " 0x7fff0001", {a: BIG}))
    if has("p"):
        V.append(("allreduce set", {"p.allreduce": _allreduce(pkg)}))
    if batch:
        V += [("npairs 0", {"npairs": 0}),
              ("empty source pair", {"src_off": np.array([0, 8, 8], np.int64)}),
              ("empty target pair", {"tgt_off": np.array([0, 7, 7], np.int64)}),
              ("pair too large", {"src_off": np.array([0, BIG, BIG + 5], np.int64)}),
              ("batch too large", {"tgt_off": np.array([0, 0x7fff0000, 0x7fff0000 + 6], np.int64)})]
    for s in OVERLAP_PARAMS:
        if has(s):
            V += [("overlap %s" % v, {s + ".overlap": v}) for v in (0.0, 1.5, NAN)]
            if batch:
                V += [("overlap %s, no overlaps array" % v, {s + ".overlap": v, "overlaps": None}) for v in (0.0, 1.5, NAN)]
    if has("overlaps"):
        V += [("overlaps[1] %s" % v, {"overlaps": np.array([0.9, v])}) for v in (0.0, 1.5, NAN)]
    for s in METRIC_PARAMS:
        if has(s):
            V.append(("metric 2", {s + ".metric": 2}))
            if has("nrm"):
                V.append(("metric point, normals given", {s + ".metric": 0}))
            elif has("sp"):
                V.append(("metric point", {s + ".metric": 0}))
    if has("rp"):
        V += [("loss 4", {"rp.loss": 4}), ("loss -1", {"rp.loss": -1}),
              ("scale -1", {"rp.scale": -1.0}), ("scale inf", {"rp.scale": INF}), ("scale nan", {"rp.scale": NAN}),
              ("scale 0, tune 0", {"rp.tune": 0.0}), ("scale 0, tune nan", {"rp.tune": NAN}), ("min_scale -1", {"rp.min_scale": -1.0})]
    if has("scales"):
        V += [("scales[1] -1", {"scales": np.array([0.1, -1.0])}), ("scales[1] inf", {"scales": np.array([0.1, INF])}),
              ("scales[1] nan", {"scales": np.array([0.1, NAN])}),
              ("scales[1] 0, tune 0", {"rp.scale": 0.1, "rp.tune": 0.0, "scales": np.array([0.1, 0.0])})]
    if has("gp"):
        V += [("epsilon %s" % v, {"gp.epsilon": v}) for v in (0.0, 2.0, NAN)]
    if has("epsilons"):
        V += [("epsilons[1] %s" % v, {"epsilons": np.array([1e-3, v])}) for v in (0.0, 2.0)]
    if has("sp"):
        V.append(("align_normals 2", {"sp.align_normals": 2}))
    if has("aligns"):
        V.append(("aligns[1] 2", {"aligns": np.array([1, 2], np.int32)}))
    for s in ("gp", "sp"):
        if has(s):
            for k in (2, 65):
                V += [("normals_k %d, normals missing" % k, {s + ".normals_k": k, "snrm": None, "tnrm": None}),
                      ("normals_k %d, source normals missing" % k, {s + ".normals_k": k, "snrm": None}),
                      ("normals_k %d, normals given" % k, {s + ".normals_k": k})]
    if has("simp"):
        V += [("scale_min 0", {"simp.scale_min": 0.0}), ("scale_min 1.5", {"simp.scale_min": 1.5}), ("scale_min nan", {"simp.scale_min": NAN}),
              ("scale_max 0.5", {"simp.scale_max": 0.5}), ("scale_max inf", {"simp.scale_max": INF}), ("scale_max nan", {"simp.scale_max": NAN})]
    if sums and host and base not in ("sim_sums", "robust_sums"):
        for v in ("nt", -1):
            idx = (np.arange(8) % 7).astype(np.int32)
            idx[3] = 7 if v == "nt" else -1
            V.append(("idx[3] %s" % v, {"idx": idx}))
    # two faults from different checks: which one speaks first
    out = "sums" if sums else "res"
    for s, f, v in (("tp", "metric", 2), ("op", "metric", 2), ("rcp", "metric", 2), ("simp", "scale_min", 0.0), ("gp", "epsilon", 0.0),
                    ("sp", "align_normals", 2)):
        if has(s):
            V.append(("null %s and %s %s" % (out, f, v), {out: None, s + "." + f: v}))
    if has("rp"):
        V.append(("null %s and loss 4" % out, {out: None, "rp.loss": 4}))
    if base in ("p2l_sums", "sim_sums"):
        V.append(("null sums and n 0", {"sums": None, "n": 0}))
    if base in ("icp_p2l", "icp_p2l_batch"):
        V.append(("null res and allreduce set", {"res": None, "p.allreduce": _allreduce(pkg)}))
    labels = [l for l, _ in V]
    assert len(set(labels)) == len(labels), labels
    return V


_DEVICE = {}


def _pointer(a, dev, keep):
    """The address of an argument's value: numpy arrays on the host, a device copy of them for a _dev entry's clouds."""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        if dev:
            import torch
            key = (a.dtype.str, a.tobytes())
            if key not in _DEVICE:
                _DEVICE[key] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
            return _DEVICE[key].data_ptr()
        a = np.ascontiguousarray(a)
        keep.append(a)
        return a.ctypes.data
    return a if isinstance(a, C.Array) else C.byref(a)


def call(pkg, ctx, sym, overrides):
    """One call of the entry with the valid arguments changed by overrides: (status, kss_last_error text)."""
    L = ctx.L
    dev = sym.endswith("_dev")
    base = sym[len("kss_"):-len("_dev")] if dev else sym[len("kss_"):]
    args = valid_args(pkg, L, base)
    handle = ctx.h
    for k, v in overrides.items():
        if k == "c":
            handle = v
        elif "." in k:
            s, f = k.split(".")
            setattr(args[s], f, v)
        else:
            args[k] = v
    keep, out = [], []
    for a in ENTRIES[base].split():
        v = args[a]
        out.append(v if isinstance(v, (int, float)) else _pointer(v, dev and a in DEVICE_ARGS, keep))
    rc = getattr(L, sym)(handle, *out)
    return rc, L.kss_last_error(ctx.h).decode()


def collect(pkg, ctx, sym):
    """label -> (status, text) of every variant of one entry (also what a job that records a build's answers calls)."""
    dev = sym.endswith("_dev")
    base = sym[len("kss_"):-len("_dev")] if dev else sym[len("kss_"):]
    return {label: call(pkg, ctx, sym, ov) for label, ov in variants(pkg, base, not dev)}


EXPECT = {
    "p2l_sums": {
        "valid": OK,
        "null c": "",
        "null src": "p2l_sums: null argument",
        "null tgt": "p2l_sums: null argument",
        "null nrm": "p2l_sums: null argument",
        "null idx": "p2l_sums: null argument",
        "null sums": "p2l_sums: null argument",
        "n 0": "p2l_sums: empty input",
        "nt 0": "p2l_sums: empty input",
        "idx[3] nt": ("p2l_sums: index out of range", None),
        "idx[3] -1": ("p2l_sums: index out of range", None),
        "null sums and n 0": "p2l_sums: null argument",
    },
    "sim_sums": {
        "valid": OK,
        "null c": "",
        "null src": "sim_sums: null argument",
        "null tgt": "sim_sums: null argument",
        "null idx": "sim_sums: null argument",
        "null sums": "sim_sums: null argument",
        "n 0": "sim_sums: empty input",
        "n 0x7fff0001": "sim_sums: cloud too large",
        "nt 0": "sim_sums: empty input",
        "nt 0x7fff0001": "sim_sums: cloud too large",
        "null sums and n 0": "sim_sums: null argument",
    },
    "robust_sums": {
        "valid": OK,
        "null c": "",
        "null src": "robust_sums: null argument",
        "null tgt": "robust_sums: null argument",
        "null nrm": "robust_sums: null argument",
        "null idx": "robust_sums: null argument",
        "null rp": "robust_sums: null argument",
        "null sums": "robust_sums: null argument",
        "null info": "robust_sums: null argument",
        "n 0": "robust_sums: empty input",
        "n 0x7fff0001": "robust_sums: cloud too large",
        "nt 0": "robust_sums: empty input",
        "nt 0x7fff0001": "robust_sums: cloud too large",
        "metric 2": "robust_sums: unknown metric",
        "metric point, normals given": "robust_sums: the point metric takes no normals",
        "loss 4": "robust_sums: unknown loss",
        "loss -1": "robust_sums: unknown loss",
        "scale -1": "robust_sums: scale must be finite and >= 0",
        "scale inf": "robust_sums: scale must be finite and >= 0",
        "scale nan": "robust_sums: scale must be finite and >= 0",
        "scale 0, tune 0": "robust_sums: tune must be finite and > 0",
        "scale 0, tune nan": "robust_sums: tune must be finite and > 0",
        "min_scale -1": "robust_sums: min_scale must be >= 0",
        "null sums and loss 4": "robust_sums: unknown loss",
    },
    "gicp_sums": {
        "valid": OK,
        "null c": "",
        "null src": "gicp_sums: null argument",
        "null tgt": "gicp_sums: null argument",
        "null idx": "gicp_sums: null argument",
        "null gp": "gicp_sums: null argument",
        "null sums": "gicp_sums: null argument",
        "n 0": "gicp_sums: empty input",
        "n 0x7fff0001": "gicp_sums: cloud too large",
        "nt 0": "gicp_sums: empty input",
        "nt 0x7fff0001": "gicp_sums: cloud too large",
        "epsilon 0.0": "gicp_sums: epsilon must be in (0, 1]",
        "epsilon 2.0": "gicp_sums: epsilon must be in (0, 1]",
        "epsilon nan": "gicp_sums: epsilon must be in (0, 1]",
        "normals_k 2, normals missing": "gicp_sums: normals_k must be in 3..64",
        "normals_k 2, source normals missing": "gicp_sums: normals_k must be in 3..64",
        "normals_k 2, normals given": OK,
        "normals_k 65, normals missing": "gicp_sums: normals_k must be in 3..64",
        "normals_k 65, source normals missing": "gicp_sums: normals_k must be in 3..64",
        "normals_k 65, normals given": OK,
        "idx[3] nt": ("gicp_sums: index out of range", None),
        "idx[3] -1": ("gicp_sums: index out of range", None),
        "null sums and epsilon 0.0": "gicp_sums: epsilon must be in (0, 1]",
    },
    "symm_sums": {
        "valid": OK,
        "null c": "",
        "null src": "symm_sums: null argument",
        "null tgt": "symm_sums: null argument",
        "null idx": "symm_sums: null argument",
        "null sp": "symm_sums: null argument",
        "null sums": "symm_sums: null argument",
        "n 0": "symm_sums: empty input",
        "n 0x7fff0001": "symm_sums: cloud too large",
        "nt 0": "symm_sums: empty input",
        "nt 0x7fff0001": "symm_sums: cloud too large",
        "align_normals 2": "symm_sums: align_normals must be 0 or 1",
        "normals_k 2, normals missing": "symm_sums: normals_k must be in 3..64",
        "normals_k 2, source normals missing": "symm_sums: normals_k must be in 3..64",
        "normals_k 2, normals given": OK,
        "normals_k 65, normals missing": "symm_sums: normals_k must be in 3..64",
        "normals_k 65, source normals missing": "symm_sums: normals_k must be in 3..64",
        "normals_k 65, normals given": OK,
        "idx[3] nt": ("symm_sums: index out of range", None),
        "idx[3] -1": ("symm_sums: index out of range", None),
        "null sums and align_normals 2": "symm_sums: align_normals must be 0 or 1",
    },
    "symm_robust_sums": {
        "valid": OK,
        "null c": "",
        "null src": "symm_robust_sums: null argument",
        "null tgt": "symm_robust_sums: null argument",
        "null idx": "symm_robust_sums: null argument",
        "null sp": "symm_robust_sums: null argument",
        "null rp": "symm_robust_sums: null argument",
        "null sums": "symm_robust_sums: null argument",
        "null info": "symm_robust_sums: null argument",
        "n 0": "symm_robust_sums: empty input",
        "n 0x7fff0001": "symm_robust_sums: cloud too large",
        "nt 0": "symm_robust_sums: empty input",
        "nt 0x7fff0001": "symm_robust_sums: cloud too large",
        "metric 2": "symm_robust_sums: unknown metric",
        "metric point": "symm_robust_sums: the metric must be KSS_METRIC_PLANE",
        "loss 4": "symm_robust_sums: unknown loss",
        "loss -1": "symm_robust_sums: unknown loss",
        "scale -1": "symm_robust_sums: scale must be finite and >= 0",
        "scale inf": "symm_robust_sums: scale must be finite and >= 0",
        "scale nan": "symm_robust_sums: scale must be finite and >= 0",
        "scale 0, tune 0": "symm_robust_sums: tune must be finite and > 0",
        "scale 0, tune nan": "symm_robust_sums: tune must be finite and > 0",
        "min_scale -1": "symm_robust_sums: min_scale must be >= 0",
        "align_normals 2": "symm_robust_sums: align_normals must be 0 or 1",
        "normals_k 2, normals missing": "symm_robust_sums: normals_k must be in 3..64",
        "normals_k 2, source normals missing": "symm_robust_sums: normals_k must be in 3..64",
        "normals_k 2, normals given": OK,
        "normals_k 65, normals missing": "symm_robust_sums: normals_k must be in 3..64",
        "normals_k 65, source normals missing": "symm_robust_sums: normals_k must be in 3..64",
        "normals_k 65, normals given": OK,
        "idx[3] nt": ("symm_robust_sums: index out of range", None),
        "idx[3] -1": ("symm_robust_sums: index out of range", None),
        "null sums and align_normals 2": "symm_robust_sums: align_normals must be 0 or 1",
        "null sums and loss 4": "symm_robust_sums: unknown loss",
    },
    "icp_p2l": {
        "valid": OK,
        "null c": "",
        "null src": ("icp_p2l: null cloud", "icp_p2l: null argument"),
        "null tgt": ("icp_p2l: null cloud", "icp_p2l: null argument"),
        "null p": "icp_p2l: null argument",
        "null res": "icp_p2l: null argument",
        "ns 0": "icp_p2l: empty cloud",
        "ns 0x7fff0001": "icp_p2l: cloud too large",
        "nt 0": "icp_p2l: empty cloud",
        "nt 0x7fff0001": "icp_p2l: cloud too large",
        "allreduce set": "icp_p2l: the source-row split (allreduce) is not available for point-to-plane",
        "null res and allreduce set": "icp_p2l: null argument",
    },
    "icp_trimmed": {
        "valid": OK,
        "null c": "",
        "null src": "icp_trimmed: null argument",
        "null tgt": "icp_trimmed: null argument",
        "null p": "icp_trimmed: null argument",
        "null tp": "icp_trimmed: null argument",
        "null res": "icp_trimmed: null argument",
        "ns 0": "icp_trimmed: empty cloud",
        "ns 0x7fff0001": "icp_trimmed: cloud too large",
        "nt 0": "icp_trimmed: empty cloud",
        "nt 0x7fff0001": "icp_trimmed: cloud too large",
        "allreduce set": "icp_trimmed: the source-row split (allreduce) is not available for trimmed ICP",
        "overlap 0.0": "icp_trimmed: overlap must be in (0, 1]",
        "overlap 1.5": "icp_trimmed: overlap must be in (0, 1]",
        "overlap nan": "icp_trimmed: overlap must be in (0, 1]",
        "metric 2": "icp_trimmed: unknown metric",
        "metric point, normals given": "icp_trimmed: the point metric takes no normals",
        "null res and metric 2": "icp_trimmed: null argument",
    },
    "icp_sim": {
        "valid": OK,
        "null c": "",
        "null src": "icp_sim: null argument",
        "null tgt": "icp_sim: null argument",
        "null p": "icp_sim: null argument",
        "null simp": "icp_sim: null argument",
        "null res": "icp_sim: null argument",
        "ns 0": "icp_sim: empty cloud",
        "ns 0x7fff0001": "icp_sim: cloud too large",
        "nt 0": "icp_sim: empty cloud",
        "nt 0x7fff0001": "icp_sim: cloud too large",
        "allreduce set": "icp_sim: the source-row split (allreduce) is not available for trimmed ICP",
        "overlap 0.0": "icp_sim: overlap must be in (0, 1]",
        "overlap 1.5": "icp_sim: overlap must be in (0, 1]",
        "overlap nan": "icp_sim: overlap must be in (0, 1]",
        "scale_min 0": "icp_sim: the scale bounds must satisfy 0 < scale_min <= 1 <= scale_max < inf",
        "scale_min 1.5": "icp_sim: the scale bounds must satisfy 0 < scale_min <= 1 <= scale_max < inf",
        "scale_min nan": "icp_sim: the scale bounds must satisfy 0 < scale_min <= 1 <= scale_max < inf",
        "scale_max 0.5": "icp_sim: the scale bounds must satisfy 0 < scale_min <= 1 <= scale_max < inf",
        "scale_max inf": "icp_sim: the scale bounds must satisfy 0 < scale_min <= 1 <= scale_max < inf",
        "scale_max nan": "icp_sim: the scale bounds must satisfy 0 < scale_min <= 1 <= scale_max < inf",
        "null res and scale_min 0.0": "icp_sim: the scale bounds must satisfy 0 < scale_min <= 1 <= scale_max < inf",
    },
    "icp_robust": {
        "valid": OK,
        "null c": "",
        "null src": "icp_robust: null argument",
        "null tgt": "icp_robust: null argument",
        "null p": "icp_robust: null argument",
        "null rp": "icp_robust: null argument",
        "null res": "icp_robust: null argument",
        "ns 0": "icp_robust: empty cloud",
        "ns 0x7fff0001": "icp_robust: cloud too large",
        "nt 0": "icp_robust: empty cloud",
        "nt 0x7fff0001": "icp_robust: cloud too large",
        "allreduce set": "icp_robust: the source-row split (allreduce) is not available for robust ICP",
        "metric 2": "icp_robust: unknown metric",
        "metric point, normals given": "icp_robust: the point metric takes no normals",
        "loss 4": "icp_robust: unknown loss",
        "loss -1": "icp_robust: unknown loss",
        "scale -1": "icp_robust: scale must be finite and >= 0",
        "scale inf": "icp_robust: scale must be finite and >= 0",
        "scale nan": "icp_robust: scale must be finite and >= 0",
        "scale 0, tune 0": "icp_robust: tune must be finite and > 0",
        "scale 0, tune nan": "icp_robust: tune must be finite and > 0",
        "min_scale -1": "icp_robust: min_scale must be >= 0",
        "null res and loss 4": "icp_robust: unknown loss",
    },
    "icp_gicp": {
        "valid": OK,
        "null c": "",
        "null src": "icp_gicp: null argument",
        "null tgt": "icp_gicp: null argument",
        "null p": "icp_gicp: null argument",
        "null gp": "icp_gicp: null argument",
        "null res": "icp_gicp: null argument",
        "ns 0": "icp_gicp: empty cloud",
        "ns 0x7fff0001": "icp_gicp: cloud too large",
        "nt 0": "icp_gicp: empty cloud",
        "nt 0x7fff0001": "icp_gicp: cloud too large",
        "allreduce set": "icp_gicp: the source-row split (allreduce) is not available for generalized ICP",
        "epsilon 0.0": "icp_gicp: epsilon must be in (0, 1]",
        "epsilon 2.0": "icp_gicp: epsilon must be in (0, 1]",
        "epsilon nan": "icp_gicp: epsilon must be in (0, 1]",
        "normals_k 2, normals missing": "icp_gicp: normals_k must be in 3..64",
        "normals_k 2, source normals missing": "icp_gicp: normals_k must be in 3..64",
        "normals_k 2, normals given": OK,
        "normals_k 65, normals missing": "icp_gicp: normals_k must be in 3..64",
        "normals_k 65, source normals missing": "icp_gicp: normals_k must be in 3..64",
        "normals_k 65, normals given": OK,
        "null res and epsilon 0.0": "icp_gicp: epsilon must be in (0, 1]",
    },
    "icp_symm": {
        "valid": OK,
        "null c": "",
        "null src": "icp_symm: null argument",
        "null tgt": "icp_symm: null argument",
        "null p": "icp_symm: null argument",
        "null sp": "icp_symm: null argument",
        "null res": "icp_symm: null argument",
        "ns 0": "icp_symm: empty cloud",
        "ns 0x7fff0001": "icp_symm: cloud too large",
        "nt 0": "icp_symm: empty cloud",
        "nt 0x7fff0001": "icp_symm: cloud too large",
        "allreduce set": "icp_symm: the source-row split (allreduce) is not available for symmetric ICP",
        "align_normals 2": "icp_symm: align_normals must be 0 or 1",
        "normals_k 2, normals missing": "icp_symm: normals_k must be in 3..64",
        "normals_k 2, source normals missing": "icp_symm: normals_k must be in 3..64",
        "normals_k 2, normals given": OK,
        "normals_k 65, normals missing": "icp_symm: normals_k must be in 3..64",
        "normals_k 65, source normals missing": "icp_symm: normals_k must be in 3..64",
        "normals_k 65, normals given": OK,
        "null res and align_normals 2": "icp_symm: align_normals must be 0 or 1",
    },
    "icp_symm_robust": {
        "valid": OK,
        "null c": "",
        "null src": "icp_symm_robust: null argument",
        "null tgt": "icp_symm_robust: null argument",
        "null p": "icp_symm_robust: null argument",
        "null sp": "icp_symm_robust: null argument",
        "null rp": "icp_symm_robust: null argument",
        "null res": "icp_symm_robust: null argument",
        "ns 0": "icp_symm_robust: empty cloud",
        "ns 0x7fff0001": "icp_symm_robust: cloud too large",
        "nt 0": "icp_symm_robust: empty cloud",
        "nt 0x7fff0001": "icp_symm_robust: cloud too large",
        "allreduce set": "icp_symm_robust: the source-row split (allreduce) is not available for symmetric ICP",
        "metric 2": "icp_symm_robust: unknown metric",
        "metric point": "icp_symm_robust: the metric must be KSS_METRIC_PLANE",
        "loss 4": "icp_symm_robust: unknown loss",
        "loss -1": "icp_symm_robust: unknown loss",
        "scale -1": "icp_symm_robust: scale must be finite and >= 0",
        "scale inf": "icp_symm_robust: scale must be finite and >= 0",
        "scale nan": "icp_symm_robust: scale must be finite and >= 0",
        "scale 0, tune 0": "icp_symm_robust: tune must be finite and > 0",
        "scale 0, tune nan": "icp_symm_robust: tune must be finite and > 0",
        "min_scale -1": "icp_symm_robust: min_scale must be >= 0",
        "align_normals 2": "icp_symm_robust: align_normals must be 0 or 1",
        "normals_k 2, normals missing": "icp_symm_robust: normals_k must be in 3..64",
        "normals_k 2, source normals missing": "icp_symm_robust: normals_k must be in 3..64",
        "normals_k 2, normals given": OK,
        "normals_k 65, normals missing": "icp_symm_robust: normals_k must be in 3..64",
        "normals_k 65, source normals missing": "icp_symm_robust: normals_k must be in 3..64",
        "normals_k 65, normals given": OK,
        "null res and align_normals 2": "icp_symm_robust: align_normals must be 0 or 1",
        "null res and loss 4": "icp_symm_robust: unknown loss",
    },
    "icp_o2o": {
        "valid": OK,
        "null c": "",
        "null src": "icp_o2o: null argument",
        "null tgt": "icp_o2o: null argument",
        "null p": "icp_o2o: null argument",
        "null op": "icp_o2o: null argument",
        "null res": "icp_o2o: null argument",
        "ns 0": "icp_o2o: empty cloud",
        "ns 0x7fff0001": "icp_o2o: cloud too large",
        "nt 0": "icp_o2o: empty cloud",
        "nt 0x7fff0001": "icp_o2o: cloud too large",
        "allreduce set": "icp_o2o: the source-row split (allreduce) is not available for trimmed ICP",
        "overlap 0.0": "icp_o2o: overlap must be in (0, 1]",
        "overlap 1.5": "icp_o2o: overlap must be in (0, 1]",
        "overlap nan": "icp_o2o: overlap must be in (0, 1]",
        "metric 2": "icp_o2o: unknown metric",
        "metric point, normals given": "icp_o2o: the point metric takes no normals",
        "null res and metric 2": "icp_o2o: null argument",
    },
    "icp_recip": {
        "valid": OK,
        "null c": "",
        "null src": "icp_recip: null argument",
        "null tgt": "icp_recip: null argument",
        "null p": "icp_recip: null argument",
        "null rcp": "icp_recip: null argument",
        "null res": "icp_recip: null argument",
        "ns 0": "icp_recip: empty cloud",
        "ns 0x7fff0001": "icp_recip: cloud too large",
        "nt 0": "icp_recip: empty cloud",
        "nt 0x7fff0001": "icp_recip: cloud too large",
        "allreduce set": "icp_recip: the source-row split (allreduce) is not available for trimmed ICP",
        "overlap 0.0": "icp_recip: overlap must be in (0, 1]",
        "overlap 1.5": "icp_recip: overlap must be in (0, 1]",
        "overlap nan": "icp_recip: overlap must be in (0, 1]",
        "metric 2": "icp_recip: unknown metric",
        "metric point, normals given": "icp_recip: the point metric takes no normals",
        "null res and metric 2": "icp_recip: null argument",
    },
    "icp_p2l_batch": {
        "valid": OK,
        "null c": "",
        "null src": "icp_p2l_batch: null argument",
        "null src_off": "icp_p2l_batch: bad batch",
        "null tgt": "icp_p2l_batch: null argument",
        "null tgt_off": "icp_p2l_batch: bad batch",
        "null p": "icp_p2l_batch: null argument",
        "null res": "icp_p2l_batch: null argument",
        "allreduce set": "icp_p2l_batch: the source-row split (allreduce) is not available for point-to-plane",
        "npairs 0": "icp_p2l_batch: bad batch",
        "empty source pair": "icp_p2l_batch: empty pair",
        "empty target pair": "icp_p2l_batch: empty pair",
        "pair too large": "icp_p2l_batch: cloud too large",
        "batch too large": "icp_p2l_batch: batch too large",
        "null res and allreduce set": "icp_p2l_batch: null argument",
    },
    "icp_trimmed_batch": {
        "valid": OK,
        "null c": "",
        "null src": "icp_trimmed_batch: null argument",
        "null src_off": "icp_trimmed_batch: bad batch",
        "null tgt": "icp_trimmed_batch: null argument",
        "null tgt_off": "icp_trimmed_batch: bad batch",
        "null p": "icp_trimmed_batch: null argument",
        "null tp": "icp_trimmed_batch: null argument",
        "null res": "icp_trimmed_batch: null argument",
        "allreduce set": "icp_trimmed_batch: the source-row split (allreduce) is not available for trimmed ICP",
        "npairs 0": "icp_trimmed_batch: bad batch",
        "empty source pair": "icp_trimmed_batch: empty pair",
        "empty target pair": "icp_trimmed_batch: empty pair",
        "pair too large": "icp_trimmed_batch: cloud too large",
        "batch too large": "icp_trimmed_batch: batch too large",
        "overlap 0.0": OK,
        "overlap 1.5": OK,
        "overlap nan": OK,
        "overlap 0.0, no overlaps array": "icp_trimmed_batch: overlap must be in (0, 1]",
        "overlap 1.5, no overlaps array": "icp_trimmed_batch: overlap must be in (0, 1]",
        "overlap nan, no overlaps array": "icp_trimmed_batch: overlap must be in (0, 1]",
        "overlaps[1] 0.0": "icp_trimmed_batch: overlap must be in (0, 1]",
        "overlaps[1] 1.5": "icp_trimmed_batch: overlap must be in (0, 1]",
        "overlaps[1] nan": "icp_trimmed_batch: overlap must be in (0, 1]",
        "metric 2": "icp_trimmed_batch: unknown metric",
        "metric point, normals given": "icp_trimmed_batch: the point metric takes no normals",
        "null res and metric 2": "icp_trimmed_batch: null argument",
    },
    "icp_sim_batch": {
        "valid": OK,
        "null c": "",
        "null src": "icp_sim_batch: null argument",
        "null src_off": "icp_sim_batch: bad batch",
        "null tgt": "icp_sim_batch: null argument",
        "null tgt_off": "icp_sim_batch: bad batch",
        "null p": "icp_sim_batch: null argument",
        "null simp": "icp_sim_batch: null argument",
        "null res": "icp_sim_batch: null argument",
        "allreduce set": "icp_sim_batch: the source-row split (allreduce) is not available for trimmed ICP",
        "npairs 0": "icp_sim_batch: bad batch",
        "empty source pair": "icp_sim_batch: empty pair",
        "empty target pair": "icp_sim_batch: empty pair",
        "pair too large": "icp_sim_batch: cloud too large",
        "batch too large": "icp_sim_batch: batch too large",
        "overlap 0.0": OK,
        "overlap 1.5": OK,
        "overlap nan": OK,
        "overlap 0.0, no overlaps array": "icp_sim_batch: overlap must be in (0, 1]",
        "overlap 1.5, no overlaps array": "icp_sim_batch: overlap must be in (0, 1]",
        "overlap nan, no overlaps array": "icp_sim_batch: overlap must be in (0, 1]",
        "overlaps[1] 0.0": "icp_sim_batch: overlap must be in (0, 1]",
        "overlaps[1] 1.5": "icp_sim_batch: overlap must be in (0, 1]",
        "overlaps[1] nan": "icp_sim_batch: overlap must be in (0, 1]",
        "scale_min 0": "icp_sim_batch: the scale bounds must satisfy 0 < scale_min <= 1 <= scale_max < inf",
        "scale_min 1.5": "icp_sim_batch: the scale bounds must satisfy 0 < scale_min <= 1 <= scale_max < inf",
        "scale_min nan": "icp_sim_batch: the scale bounds must satisfy 0 < scale_min <= 1 <= scale_max < inf",
        "scale_max 0.5": "icp_sim_batch: the scale bounds must satisfy 0 < scale_min <= 1 <= scale_max < inf",
        "scale_max inf": "icp_sim_batch: the scale bounds must satisfy 0 < scale_min <= 1 <= scale_max < inf",
        "scale_max nan": "icp_sim_batch: the scale bounds must satisfy 0 < scale_min <= 1 <= scale_max < inf",
        "null res and scale_min 0.0": "icp_sim_batch: the scale bounds must satisfy 0 < scale_min <= 1 <= scale_max < inf",
    },
    "icp_robust_batch": {
        "valid": OK,
        "null c": "",
        "null src": "icp_robust_batch: null argument",
        "null src_off": "icp_robust_batch: bad batch",
        "null tgt": "icp_robust_batch: null argument",
        "null tgt_off": "icp_robust_batch: bad batch",
        "null p": "icp_robust_batch: null argument",
        "null rp": "icp_robust_batch: null argument",
        "null res": "icp_robust_batch: null argument",
        "allreduce set": "icp_robust_batch: the source-row split (allreduce) is not available for robust ICP",
        "npairs 0": "icp_robust_batch: bad batch",
        "empty source pair": "icp_robust_batch: empty pair",
        "empty target pair": "icp_robust_batch: empty pair",
        "pair too large": "icp_robust_batch: cloud too large",
        "batch too large": "icp_robust_batch: batch too large",
        "metric 2": "icp_robust_batch: unknown metric",
        "metric point, normals given": "icp_robust_batch: the point metric takes no normals",
        "loss 4": "icp_robust_batch: unknown loss",
        "loss -1": "icp_robust_batch: unknown loss",
        "scale -1": "icp_robust_batch: scale must be finite and >= 0",
        "scale inf": "icp_robust_batch: scale must be finite and >= 0",
        "scale nan": "icp_robust_batch: scale must be finite and >= 0",
        "scale 0, tune 0": "icp_robust_batch: tune must be finite and > 0",
        "scale 0, tune nan": "icp_robust_batch: tune must be finite and > 0",
        "min_scale -1": "icp_robust_batch: min_scale must be >= 0",
        "scales[1] -1": "icp_robust_batch: a scale must be finite and >= 0",
        "scales[1] inf": "icp_robust_batch: a scale must be finite and >= 0",
        "scales[1] nan": "icp_robust_batch: a scale must be finite and >= 0",
        "scales[1] 0, tune 0": "icp_robust_batch: tune must be finite and > 0",
        "null res and loss 4": "icp_robust_batch: unknown loss",
    },
    "icp_gicp_batch": {
        "valid": OK,
        "null c": "",
        "null src": "icp_gicp_batch: null argument",
        "null src_off": "icp_gicp_batch: bad batch",
        "null tgt": "icp_gicp_batch: null argument",
        "null tgt_off": "icp_gicp_batch: bad batch",
        "null p": "icp_gicp_batch: null argument",
        "null gp": "icp_gicp_batch: null argument",
        "null res": "icp_gicp_batch: null argument",
        "allreduce set": "icp_gicp_batch: the source-row split (allreduce) is not available for generalized ICP",
        "npairs 0": "icp_gicp_batch: bad batch",
        "empty source pair": "icp_gicp_batch: empty pair",
        "empty target pair": "icp_gicp_batch: empty pair",
        "pair too large": "icp_gicp_batch: cloud too large",
        "batch too large": "icp_gicp_batch: batch too large",
        "epsilon 0.0": "icp_gicp_batch: epsilon must be in (0, 1]",
        "epsilon 2.0": "icp_gicp_batch: epsilon must be in (0, 1]",
        "epsilon nan": "icp_gicp_batch: epsilon must be in (0, 1]",
        "epsilons[1] 0.0": "icp_gicp_batch: every epsilon must be in (0, 1]",
        "epsilons[1] 2.0": "icp_gicp_batch: every epsilon must be in (0, 1]",
        "normals_k 2, normals missing": "icp_gicp_batch: normals_k must be in 3..64",
        "normals_k 2, source normals missing": "icp_gicp_batch: normals_k must be in 3..64",
        "normals_k 2, normals given": OK,
        "normals_k 65, normals missing": "icp_gicp_batch: normals_k must be in 3..64",
        "normals_k 65, source normals missing": "icp_gicp_batch: normals_k must be in 3..64",
        "normals_k 65, normals given": OK,
        "null res and epsilon 0.0": "icp_gicp_batch: epsilon must be in (0, 1]",
    },
    "icp_symm_batch": {
        "valid": OK,
        "null c": "",
        "null src": "icp_symm_batch: null argument",
        "null src_off": "icp_symm_batch: bad batch",
        "null tgt": "icp_symm_batch: null argument",
        "null tgt_off": "icp_symm_batch: bad batch",
        "null p": "icp_symm_batch: null argument",
        "null sp": "icp_symm_batch: null argument",
        "null res": "icp_symm_batch: null argument",
        "allreduce set": "icp_symm_batch: the source-row split (allreduce) is not available for symmetric ICP",
        "npairs 0": "icp_symm_batch: bad batch",
        "empty source pair": "icp_symm_batch: empty pair",
        "empty target pair": "icp_symm_batch: empty pair",
        "pair too large": "icp_symm_batch: cloud too large",
        "batch too large": "icp_symm_batch: batch too large",
        "align_normals 2": "icp_symm_batch: align_normals must be 0 or 1",
        "aligns[1] 2": "icp_symm_batch: every align must be 0 or 1",
        "normals_k 2, normals missing": "icp_symm_batch: normals_k must be in 3..64",
        "normals_k 2, source normals missing": "icp_symm_batch: normals_k must be in 3..64",
        "normals_k 2, normals given": OK,
        "normals_k 65, normals missing": "icp_symm_batch: normals_k must be in 3..64",
        "normals_k 65, source normals missing": "icp_symm_batch: normals_k must be in 3..64",
        "normals_k 65, normals given": OK,
        "null res and align_normals 2": "icp_symm_batch: align_normals must be 0 or 1",
    },
    "icp_symm_robust_batch": {
        "valid": OK,
        "null c": "",
        "null src": "icp_symm_robust_batch: null argument",
        "null src_off": "icp_symm_robust_batch: bad batch",
        "null tgt": "icp_symm_robust_batch: null argument",
        "null tgt_off": "icp_symm_robust_batch: bad batch",
        "null p": "icp_symm_robust_batch: null argument",
        "null sp": "icp_symm_robust_batch: null argument",
        "null rp": "icp_symm_robust_batch: null argument",
        "null res": "icp_symm_robust_batch: null argument",
        "allreduce set": "icp_symm_robust_batch: the source-row split (allreduce) is not available for symmetric ICP",
        "npairs 0": "icp_symm_robust_batch: bad batch",
        "empty source pair": "icp_symm_robust_batch: empty pair",
        "empty target pair": "icp_symm_robust_batch: empty pair",
        "pair too large": "icp_symm_robust_batch: cloud too large",
        "batch too large": "icp_symm_robust_batch: batch too large",
        "metric 2": "icp_symm_robust_batch: unknown metric",
        "metric point": "icp_symm_robust_batch: the metric must be KSS_METRIC_PLANE",
        "loss 4": "icp_symm_robust_batch: unknown loss",
        "loss -1": "icp_symm_robust_batch: unknown loss",
        "scale -1": "icp_symm_robust_batch: scale must be finite and >= 0",
        "scale inf": "icp_symm_robust_batch: scale must be finite and >= 0",
        "scale nan": "icp_symm_robust_batch: scale must be finite and >= 0",
        "scale 0, tune 0": "icp_symm_robust_batch: tune must be finite and > 0",
        "scale 0, tune nan": "icp_symm_robust_batch: tune must be finite and > 0",
        "min_scale -1": "icp_symm_robust_batch: min_scale must be >= 0",
        "scales[1] -1": "icp_symm_robust_batch: a scale must be finite and >= 0",
        "scales[1] inf": "icp_symm_robust_batch: a scale must be finite and >= 0",
        "scales[1] nan": "icp_symm_robust_batch: a scale must be finite and >= 0",
        "scales[1] 0, tune 0": "icp_symm_robust_batch: tune must be finite and > 0",
        "align_normals 2": "icp_symm_robust_batch: align_normals must be 0 or 1",
        "aligns[1] 2": "icp_symm_robust_batch: every align must be 0 or 1",
        "normals_k 2, normals missing": "icp_symm_robust_batch: normals_k must be in 3..64",
        "normals_k 2, source normals missing": "icp_symm_robust_batch: normals_k must be in 3..64",
        "normals_k 2, normals given": OK,
        "normals_k 65, normals missing": "icp_symm_robust_batch: normals_k must be in 3..64",
        "normals_k 65, source normals missing": "icp_symm_robust_batch: normals_k must be in 3..64",
        "normals_k 65, normals given": OK,
        "null res and align_normals 2": "icp_symm_robust_batch: align_normals must be 0 or 1",
        "null res and loss 4": "icp_symm_robust_batch: unknown loss",
    },
    "icp_o2o_batch": {
        "valid": OK,
        "null c": "",
        "null src": "icp_o2o_batch: null argument",
        "null src_off": "icp_o2o_batch: bad batch",
        "null tgt": "icp_o2o_batch: null argument",
        "null tgt_off": "icp_o2o_batch: bad batch",
        "null p": "icp_o2o_batch: null argument",
        "null op": "icp_o2o_batch: null argument",
        "null res": "icp_o2o_batch: null argument",
        "allreduce set": "icp_o2o_batch: the source-row split (allreduce) is not available for trimmed ICP",
        "npairs 0": "icp_o2o_batch: bad batch",
        "empty source pair": "icp_o2o_batch: empty pair",
        "empty target pair": "icp_o2o_batch: empty pair",
        "pair too large": "icp_o2o_batch: cloud too large",
        "batch too large": "icp_o2o_batch: batch too large",
        "overlap 0.0": OK,
        "overlap 1.5": OK,
        "overlap nan": OK,
        "overlap 0.0, no overlaps array": "icp_o2o_batch: overlap must be in (0, 1]",
        "overlap 1.5, no overlaps array": "icp_o2o_batch: overlap must be in (0, 1]",
        "overlap nan, no overlaps array": "icp_o2o_batch: overlap must be in (0, 1]",
        "overlaps[1] 0.0": "icp_o2o_batch: overlap must be in (0, 1]",
        "overlaps[1] 1.5": "icp_o2o_batch: overlap must be in (0, 1]",
        "overlaps[1] nan": "icp_o2o_batch: overlap must be in (0, 1]",
        "metric 2": "icp_o2o_batch: unknown metric",
        "metric point, normals given": "icp_o2o_batch: the point metric takes no normals",
        "null res and metric 2": "icp_o2o_batch: null argument",
    },
}


@pytest.mark.parametrize("sym", SYMBOLS)
def test_argument_errors(pkg, ctx, sym):
    dev = sym.endswith("_dev")
    base = sym[len("kss_"):-len("_dev")] if dev else sym[len("kss_"):]
    want = EXPECT[base]
    got = collect(pkg, ctx, sym)
    applicable = {l for l, w in want.items() if not (isinstance(w, tuple) and w[dev] is None)}
    assert set(got) == applicable, sorted(set(got) ^ applicable)
    wrong = []
    for label, (rc, text) in got.items():
        w = want[label]
        w = w[dev] if isinstance(w, tuple) else w
        print("%-28s %-44s -> %d %r" % (sym, label, rc, text))
        if w == OK:
            ok = rc == OK
        elif label == "null c":
            ok = rc == ERR_ARG   # (no context to hold a text)
        else:
            ok = rc == ERR_ARG and text == w
        if not ok:
            wrong.append((label, rc, text, w))
    assert not wrong, wrong
