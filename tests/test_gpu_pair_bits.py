"""The bits of the pair metrics against a recording (tests/golden/pair_metric_bits.npz, made by tests/golden/make_pair_metric_bits.py
on the build before the rows kernels were folded into two templates).  The other suites prove batch = single pair
and single pair ~ restatement; this one proves that the bits did not move in both at once: every sums record (all metrics, one
lane to a grid-stride loop that wraps) and every single-pair ICP result under every nn_mode is recomputed and compared bit for bit."""

import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_pair_metric_bits", os.path.join(GOLDEN, "make_pair_metric_bits.py"))
GEN = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(GEN)

with np.load(GEN.PATH) as _z:
    RECORDED = {k: _z[k] for k in _z.files}
NAMES = sorted(k for k in RECORDED if not k.startswith("input/"))


@pytest.fixture(scope="module")
def recomputed(pkg, ctx):
    inp = {k: v for k, v in RECORDED.items() if k.startswith("input/")}
    return GEN.records(pkg, ctx, inp)


def test_recording_is_complete(recomputed):
    """5 sums methods in 9 forms at 5 source counts, 8 ICP forms under 3 nn_modes: nothing recorded that is not recomputed, nothing
    recomputed that is not recorded."""
    assert len(NAMES) == 9 * len(GEN.SUMS_N) + 8 * 3
    assert sorted(recomputed) == NAMES


@pytest.mark.parametrize("name", NAMES)
def test_bits_match_recording(recomputed, name):
    got, want = recomputed[name], RECORDED[name]
    assert got.dtype == np.uint64 and want.dtype == np.uint64
    diff = np.flatnonzero(got != want) if got.shape == want.shape else None
    print("%s: %d words, %s differ" % (name, len(want), "shapes" if diff is None else len(diff)))
    assert got.shape == want.shape
    assert len(diff) == 0, (name, diff[:8], got.view(np.float64)[diff[:8]], want.view(np.float64)[diff[:8]])
