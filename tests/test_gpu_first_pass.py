"""GPU tests of the first pass of a single pair (kss_grid.hip: block_walk_first, one round of 512 walkers) and of the
one-atomic cell-list build (the count hands out the slots, the scan zeroes the counters): neither may move a bit.

  - kss_nn through the cell list equals the brute-force sweep, index and distance bits, on pairs of 3 to 10 rows (one with a
    ragged last row), on exact ties, on sources outside the target's box, on sources far enough away for the shells and the
    list fallback, and with a non-finite source;
  - a 5-iteration registration of every pair gives the same record with the two-stage first pass (default), with the plain
    pass first (KSS_FIRST_PASS=0) and with one launch per pass (KSS_CHAIN=0);
  - two registrations of different sizes back to back on one context leave the cell counters zero at rest
    (KSS_COUNTS_CHECK=1 checks them before every build) and the second equals a fresh context's.

The rule itself is restated and checked on the CPU in tests/test_first_pass_prune.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

PAIRS = ("n1100", "n2600", "n5000", "lattice", "outside", "far", "nonfinite")


def make_pair(S, name):
    """(source, target) float32 of the named pair; S = the package's synth module"""
    if name in ("n1100", "n2600", "n5000"):   # 3, 6 and 10 rows of 512 sources; 2600 = 5 * 512 + 40: a ragged last row
        n = int(name[1:])
        return S.make_pair(400 + n % 97, n, R=S.rot_axis_angle([0.2, 0.1, 1.0], np.deg2rad(8.0)), t=(0.02, -0.01, 0.03), shape="bumpy")
    if name == "lattice":   # 12^3 lattice, sources on the mid-points of its cells: eight equidistant targets each, in exact arithmetic
        g = np.arange(12, dtype=np.float32)
        tgt = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
        tgt = tgt[np.random.default_rng(12).permutation(len(tgt))]
        src = tgt[(tgt < 11).all(axis=1)] + np.float32(0.5)
        return src.astype(np.float32), tgt.astype(np.float32)
    if name == "outside":   # shifted by a good part of the target's extent: some sources inside its box, some outside
        tgt = S.bumpy(21, 3000).astype(np.float32)
        src = (S.bumpy(22, 1700) + np.array([0.45, -0.3, 0.2])).astype(np.float32)
        box = ((src < tgt.min(axis=0)) | (src > tgt.max(axis=0))).any(axis=1)
        assert 100 < box.sum() < len(src) - 100
        return src, tgt
    if name == "far":   # blown up: further shells; shifted far away: no shell resolves them, the brute-force list does
        tgt = S.bumpy(23, 3000).astype(np.float32)
        src = np.concatenate([S.bumpy(24, 900) * 1.6, S.bumpy(25, 700) + np.array([7.0, -3.0, 2.0])]).astype(np.float32)
        return src, tgt
    if name == "nonfinite":
        src, tgt = S.make_pair(431, 1500, R=S.rot_axis_angle([0, 0, 1], np.deg2rad(5.0)), shape="bumpy")
        src = src.copy()
        src[700] = np.nan
        return src, tgt
    raise KeyError(name)


@pytest.mark.parametrize("name", PAIRS)
def test_first_pass_nn_equals_brute_force(ctx, pkg, name):
    src, tgt = make_pair(pkg.synth, name)
    try:
        ctx.set_nn_mode(pkg.NN_BRUTE)
        bi, bd = ctx.nn(src, tgt)
        ctx.set_nn_mode(pkg.NN_GRID)
        gi, gd = ctx.nn(src, tgt)
    finally:
        ctx.set_nn_mode(pkg.NN_AUTO)
    ok = np.isfinite(src).all(axis=1)   # (a non-finite source matches nothing: its two outputs are not written)
    assert ok.sum() >= len(src) - 1
    assert np.array_equal(gi[ok], bi[ok])
    assert np.array_equal(gd[ok].view(np.uint32), bd[ok].view(np.uint32))


def _record(r):
    return [r["T"].tobytes().hex(), float(r["fitness"]).hex(), float(r["last_mse"]).hex(), int(r["iterations"]), int(r["state"])]


def run_records():
    """(child process) 5-iteration registration of every pair -> one JSON line"""
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    pkg = g.load_package()
    ctx = pkg.Context(0)
    out = {}
    for name in PAIRS:
        src, tgt = make_pair(pkg.synth, name)
        out[name] = _record(ctx.icp(src, tgt, ctx.icp_params(nn_mode=pkg.NN_GRID, max_iterations=5, fixed_iterations=1)))
    ctx.close()
    print("RESULT" + json.dumps(out))


def run_back_to_back():
    """(child process) 10-row pair, then the 3-row pair, then the 6-row pair on one context; the 3-row pair on a fresh one"""
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    pkg = g.load_package()
    out = {}
    ctx = pkg.Context(0)
    for name in ("n5000", "n1100", "n2600"):   # (the third build checks what the second left)
        src, tgt = make_pair(pkg.synth, name)
        out[name] = _record(ctx.icp(src, tgt, ctx.icp_params(nn_mode=pkg.NN_GRID, max_iterations=5, fixed_iterations=1)))
    ctx.close()
    ctx = pkg.Context(0)
    src, tgt = make_pair(pkg.synth, "n1100")
    out["fresh"] = _record(ctx.icp(src, tgt, ctx.icp_params(nn_mode=pkg.NN_GRID, max_iterations=5, fixed_iterations=1)))
    ctx.close()
    print("RESULT" + json.dumps(out))


def _child(fn, extra):
    env = dict(os.environ, **extra)
    for k in ("KSS_FIRST_PASS", "KSS_CHAIN", "KSS_COUNTS_CHECK"):
        if k not in extra:
            env.pop(k, None)
    code = "import sys; sys.path.insert(0, %r); import test_gpu_first_pass as M; M.%s()" % (HERE, fn)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, fn + str(extra) + r.stdout + r.stderr
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT")][0][6:])


@pytest.fixture(scope="module")
def default_records():
    return _child("run_records", {})


@pytest.mark.parametrize("switch", ["KSS_FIRST_PASS", "KSS_CHAIN"])
def test_registration_records_do_not_depend_on_the_switches(default_records, switch):
    other = _child("run_records", {switch: "0"})
    assert set(other) == set(PAIRS)
    for name in PAIRS:
        assert other[name] == default_records[name], (switch, name)
        assert default_records[name][3] == 5, name


def test_back_to_back_registrations_leave_the_counters_zero(default_records):
    out = _child("run_back_to_back", {"KSS_COUNTS_CHECK": "1"})
    assert out["fresh"] == out["n1100"]
    for name in ("n5000", "n1100", "n2600"):
        assert out[name] == default_records[name], name
