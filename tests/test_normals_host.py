"""CPU tests of the normals reference (tests/normals_ref.py): the oracle's copy of PCL's closed form meets every rule of
check() on every input that tests/test_gpu_normals.py gives the device, the constant C comes from the oracle alone, the judged
shares are conditions (so no input can hide its points behind the conditioning), and the float covariance restatement and the
numpy k-NN are checked against independent computations."""
import numpy as np
import pytest

import normals_ref as N

F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def ref(pkg, O):
    return N.reference(pkg.synth, O)


def _ratio(tr, normals):
    """sin / B on the rows judged and finite (0 elsewhere)"""
    ok = tr["judged"] & np.isfinite(normals).all(axis=1)
    with np.errstate(all="ignore"):
        return np.where(ok, N.sin_to_v0(normals, tr) / tr["B"], 0.0)


@pytest.mark.parametrize("name", N.NAMES)
def test_oracle_meets_every_rule(ref, name):
    c, tr, no = ref[name]
    share = float(tr["judged"].mean())
    r = N.rules(c.P, c.k, no, N.C, tr=tr)
    print("%s: n %d k %d judged share %.4f fallback share %.3f non-finite rows %d largest sin / B %.3f offenders %s" % (
        name, len(c.P), c.k, share, tr["fb"].mean(), int((~np.isfinite(no).all(axis=1)).sum()), _ratio(tr, no).max(),
        {x: len(v) for x, v in r.items()}))
    assert len(N.check(c.P, c.k, no, N.C, tr=tr, only=c.only)) == 0
    if c.share is not None:
        assert share >= c.share
    if c.group == "degenerate" and name != "origin_point":
        assert not tr["judged"].any()
    if name in ("plane_exact", "lattice"):
        assert tr["fb"].all()


def test_c_is_twice_the_oracles_worst(ref):
    """C is measured on the oracle, never on the kernel."""
    worst = {name: float(_ratio(tr, no).max()) for name, (c, tr, no) in ref.items()}
    c_ref = max(worst.values())
    print("C_REF %.4f at %s; C %.1f" % (c_ref, max(worst, key=worst.get), N.C))
    assert 1.0 <= c_ref <= N.C / 2.0
    assert N.C <= 2.0 * c_ref + 1.0            # "rounded up", not padded


def test_measured_shares_are_the_oracles_own(ref):
    for key, name in (("k3", "bumpy4_k3"), ("k4", "bumpy4_k4"), ("k5", "bumpy4_k5"), ("plus10", "bumpy4_plus10")):
        assert abs(float(ref[name][1]["judged"].mean()) - N.SHARE[key]) <= 1e-3, name


def test_cov32_against_two_pass_float64(pkg, O):
    """Where nothing cancels -- a centred cloud whose every neighbourhood is the whole cloud (k = n = 64) -- every entry is within
    1e-5 of the covariance's largest: 64 roundings of 2^-24 are 3.8e-6.  On a surface (k = 20 of 6000 points) the means are not
    small and the entries carry the roundings of the second moments instead: within 1e-5 of the largest second moment."""
    P = pkg.synth.bumpy(6, 64)
    P = P - P.mean(axis=0)
    for P, k, centred in ((P, 64, True), (pkg.synth.bumpy(4, 6000), 20, False)):
        m, _ = N.cov32(P, k, O.knn_brute)
        idx, _ = O.knn_brute(P, P, k)
        Q = P.astype(F32).astype(F64)[idx]                       # [n, k, 3]
        d = Q - Q.mean(axis=1, keepdims=True)
        cov = np.einsum("nki,nkj->nij", d, d) / k
        second = np.einsum("nki,nkj->nij", Q, Q) / k
        scale = np.abs(cov if centred else second).reshape(len(P), 9).max(axis=1)
        err = np.abs(m.astype(F64) - cov).reshape(len(P), 9).max(axis=1) / scale
        print("cov32 vs two-pass f64, n %d k %d: largest entry error / scale %.2e" % (len(P), k, err.max()))
        assert err.max() <= 1e-5
        assert m.dtype == F32 and np.array_equal(m, m.transpose(0, 2, 1))


def test_numpy_knn_is_the_oracles(pkg, O, ref):
    """ascending (d2, index): the lattice is all ties"""
    for P, k in ((ref["lattice"][0].P, 20), (pkg.synth.bumpy(3, 300), 33), (ref["coincident"][0].P, 7)):
        i0, d0 = N.knn_numpy(P, P, k)
        i1, d1 = O.knn_brute(P, P, k)
        assert np.array_equal(i0, i1) and np.array_equal(d0.view(np.uint32), d1.view(np.uint32))
    a, ka = N.cov32(pkg.synth.bumpy(3, 21), 20)
    b, kb = N.cov32(pkg.synth.bumpy(3, 21), 20, O.knn_brute)
    assert ka == kb == 20 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert N.cov32(pkg.synth.bumpy(3, 4), 20)[1] == 4        # k is clamped to n


def test_check_bites(ref):
    """Each rule fires on a normal set spoilt in its own way (the oracle's output, then one defect)."""
    c, tr, no = ref["bumpy4_k20"]
    rows = np.arange(0, len(no), 7)

    def spoilt(f):
        x = no.copy()
        x[rows] = f(x[rows])
        return N.rules(c.P, c.k, x, N.C, tr=tr)

    r = spoilt(lambda x: -x)                                 # flip inverted
    assert np.array_equal(r["c"], rows) and np.array_equal(r["d"], rows) and len(r["a"]) == len(r["b"]) == 0
    r = spoilt(lambda x: x * (1.0 + 2e-6))                   # not unit length
    assert np.array_equal(r["a"], rows) and len(r["b"]) == 0
    bad = no.copy()
    bad[rows, 1] = np.nan                                    # half a NaN
    r = N.rules(c.P, c.k, bad, N.C, tr=tr)
    assert np.array_equal(r["a"], rows) and np.array_equal(r["b"], rows)
    bad = no.copy()
    bad[rows] = np.nan                                       # a judged row may not be NaN
    r = N.rules(c.P, c.k, bad, N.C, tr=tr)
    assert len(r["a"]) == 0 and np.array_equal(r["b"], rows)
    t = np.cross(no[rows], [0.3, -0.5, 0.81])                # turned by 1e-4 rad: five hundred times the typical bound
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    bad = no.copy()
    bad[rows] = np.cos(1e-4) * no[rows] + np.sin(1e-4) * t
    r = N.rules(c.P, c.k, bad, N.C, tr=tr)
    assert len(r["a"]) == 0 and len(r["b"]) >= 0.99 * len(rows)
    assert len(N.apart(c.P, c.k, bad, no, N.C, tr=tr)) >= 0.99 * len(rows)
    assert len(N.apart(c.P, c.k, no, no, N.C, tr=tr)) == 0
    # rule (e): one ulp on a row of the trig-free set
    c, tr, no = ref["bumpy4_plus10"]
    sure = np.flatnonzero(tr["sure"])
    assert len(sure) > 1000 and len(N.fallback_differs(no, no, tr)) == 0
    bad = no.copy()
    bad[sure[::3], 2] = np.nextafter(bad[sure[::3], 2], 2.0)
    bad[~tr["sure"]] = 0.0
    assert np.array_equal(N.fallback_differs(bad, no, tr), sure[::3])
