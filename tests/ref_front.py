"""Shared by tests/golden/make_ref_front.py and the ref-front tests: the inputs of tests/golden/ref_front.npz, the file
format of oracle/_ref/kss_ref_front (the reference's own initRegistration_KSS and PCR_QM classes, compiled: see
oracle/ref_front.cpp) and the same records computed by the oracle.

A front record is a dict of float64/int64 arrays:
  g, stats (x/y/z_middle_S, x/y/z_middle, scale), angle, value [g,g,g], angle_list [nl,3], preshaped [ns,3],
  posed [ns,3] (initRegistration_Rotation(S)), posed_list [min(3,nl),ns,3] (initRegistration_Rotation_Angle(S, angleList[i])),
  qm (MSE, RMSE, MAE of posed against T)."""
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINARY = os.path.join(ROOT, "oracle", "_ref", "kss_ref_front")
FIXTURE = os.path.join(ROOT, "tests", "golden", "ref_front.npz")
REF_DATA = os.path.join(ROOT, "tests", "golden", "ref_data", "registration")
FIELDS = ("g", "stats", "angle", "value", "angle_list", "preshaped", "posed", "posed_list", "qm")
QM_SIZES = ((1, 1), (1, 300), (255, 257), (257, 255), (1000, 64))


def _synth():
    import __graft_entry__ as graft
    return graft.load_package().synth


def bumpy_pair(seed_s, ns, seed_t, nt, axis=(1.0, 2.0, 3.0), rad=1.1, gain=1.3, off_s=0.0, off_t=0.0):
    """S = bumpy(seed_s, ns) * gain + off_s;  T = bumpy(seed_t, nt) rotated rad about axis, + off_t."""
    sy = _synth()
    S = sy.bumpy(seed_s, ns) * gain + off_s
    T = sy.bumpy(seed_t, nt) @ sy.rot_axis_angle(axis, rad).T + off_t
    return np.ascontiguousarray(S), np.ascontiguousarray(T)


def _load_cloud(name):
    return np.loadtxt(os.path.join(REF_DATA, name), skiprows=1, dtype=np.float64)


def front_cases():
    """[(name, S, T, step)]: the six inputs of the fixture."""
    sy = _synth()
    out = [("c1", *bumpy_pair(1, 400, 11, 500), 8.0),
           ("c2", *bumpy_pair(2, 257, 12, 300, off_s=50.0, off_t=25.0), 6.0),
           ("c3", *bumpy_pair(3, 128, 13, 129, off_s=-3.0, off_t=-1.5), 12.0),
           ("c4", np.ascontiguousarray(_load_cloud("Bunny.gird")[::7][:400]),
            np.ascontiguousarray(_load_cloud("Bunny.wlop")[::11][:450]), 8.0),
           ("c5", *bumpy_pair(5, 200, 6, 255, axis=(0.0, 1.0, 1.0), rad=2.0, gain=1.0), 16.0),
           ("c6", sy.bumpy(9, 129), np.array([[0.75, 0.0, 0.0]]), 6.0)]
    return out


def qm_cases():
    """[(name, A, T)]: prefixes of two pools.  The template pool is the first front case's target; the aligned pool is
    1000 points of the same surface, a little larger and off it."""
    sy = _synth()
    _, _, tmpl, _ = front_cases()[0]
    pool = (sy.bumpy(100, 1000) * 1.05) @ sy.rot_axis_angle((1.0, 2.0, 3.0), 1.1).T + np.array([0.02, -0.01, 0.03])
    return [("q%dx%d" % (na, nt), np.ascontiguousarray(pool[:na]), np.ascontiguousarray(tmpl[:nt])) for na, nt in QM_SIZES]


def have_binary():
    return os.path.exists(BINARY)


def _run(mode, head, arrays):
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as f:
            f.write(head)
            for a in arrays:
                f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        subprocess.run([BINARY, mode, fin, fout], check=True, stdout=subprocess.DEVNULL)
        with open(fout, "rb") as f:
            return f.read()


def ref_front(S, T, step):
    """A front record from the compiled reference."""
    S, T = np.asarray(S, np.float64).reshape(-1, 3), np.asarray(T, np.float64).reshape(-1, 3)
    head = np.array([len(S), len(T)], np.int64).tobytes() + np.array([step], np.float64).tobytes()
    raw = _run("front", head, [S, T])
    g, nl, ns, nra = (int(v) for v in np.frombuffer(raw[:32], np.int64))
    body = np.frombuffer(raw[32:], np.float64)
    assert ns == len(S) and nra == min(3, nl)
    assert body.size == 7 + 3 + g ** 3 + 3 * nl + 3 * ns * (2 + nra) + 3, (body.size, g, nl, ns, nra)
    rec, pos = {"g": np.int64(g)}, 0
    for key, shape in (("stats", (7,)), ("angle", (3,)), ("value", (g, g, g)), ("angle_list", (nl, 3)),
                       ("preshaped", (ns, 3)), ("posed", (ns, 3)), ("posed_list", (nra, ns, 3)), ("qm", (3,))):
        k = int(np.prod(shape))
        rec[key] = body[pos:pos + k].reshape(shape).copy()
        pos += k
    return rec


def ref_qm(A, T):
    A, T = np.asarray(A, np.float64).reshape(-1, 3), np.asarray(T, np.float64).reshape(-1, 3)
    raw = _run("qm", np.array([len(A), len(T)], np.int64).tobytes(), [A, T])
    out = np.frombuffer(raw, np.float64).copy()
    assert out.shape == (3,)
    return out


def oracle_front(O, S, T, step):
    """The same record from oracle/kss_oracle.c: preshape_stats, similarity_apply, rotation_search, pose_apply, pcr_qm."""
    ps = O.preshape_stats(S, T)
    pre = O.similarity_apply(S, ps)
    rs = O.rotation_search(pre, T, step)
    posed = O.pose_apply(S, ps, rs["angle"])
    alist = rs["angle_list"]
    plist = [O.pose_apply(S, ps, a) for a in alist[:3]]
    return {"g": np.int64(rs["g"]), "stats": np.array(list(ps.c_tgt) + list(ps.shift) + [ps.scale]),
            "angle": np.array(rs["angle"]), "value": rs["value"], "angle_list": alist, "preshaped": pre, "posed": posed,
            "posed_list": np.array(plist).reshape(len(plist), len(pre), 3), "qm": O.pcr_qm(posed, T)}


def same_bits(a, b):
    """Equal shape and bit patterns (so -0.0 != 0.0 and a NaN equals only the same NaN)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _shapes(ns, nt, g, nl):
    return (("S", (ns, 3)), ("T", (nt, 3)), ("step", ()), ("g", ()), ("stats", (7,)), ("angle", (3,)), ("value", (g, g, g)),
            ("angle_list", (nl, 3)), ("preshaped", (ns, 3)), ("posed", (ns, 3)), ("posed_list", (min(3, nl), ns, 3)), ("qm", (3,)))


def pack_front(S, T, step, rec):
    """(dims, flat): one float64 vector per case -- a cloud that occurs twice in a record is then stored about once."""
    dims = np.array([len(S), len(T), int(rec["g"]), len(rec["angle_list"])], np.int64)
    parts = dict(rec, S=S, T=T, step=step)
    flat = np.concatenate([np.asarray(parts[k], np.float64).reshape(-1) for k, _ in _shapes(*dims)])
    return dims, flat


def unpack_front(dims, flat):
    out, pos = {}, 0
    for key, shape in _shapes(*(int(d) for d in dims)):
        k = int(np.prod(shape))
        out[key] = flat[pos:pos + k].reshape(shape).copy()
        pos += k
    assert pos == flat.size
    out["g"] = np.int64(out["g"])
    return out


def load_fixture():
    """({name: (S, T, step, record)}, {name: (A, T, qm)}) from tests/golden/ref_front.npz."""
    z = np.load(FIXTURE)
    front = {}
    for name in (str(n) for n in z["front_names"]):
        d = unpack_front(z[name + "_dims"], z[name])
        front[name] = (d.pop("S"), d.pop("T"), float(d.pop("step")), d)
    tmpl = front[str(z["front_names"][0])][1]
    qm = {}
    for name, (na, nt), res in zip((str(n) for n in z["qm_names"]), z["qm_sizes"], z["qm_results"]):
        qm[name] = (z["qm_A"][:na].copy(), tmpl[:nt].copy(), res)
    return front, qm
