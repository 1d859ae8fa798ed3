"""The last pass's info record and the trace count at every ending of the pair-metric loop, one trimmed and one robust form (plane
metric, where a singular system can occur) on a 300 x 280 pair: two row workgroups with a ragged tail, brute-force NN.  The single
call and the batch of one run the same host loop with different kernel families: everything they return is
compared bit for bit, and what each ending must leave behind is asserted on both."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
NS, NT = 300, 280
NO_CORRESPONDENCES = 5
ENDINGS = ["max_iterations_0", "too_few_at_pass_1", "degenerate", "converged"]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == F64 else np.uint32)


@pytest.fixture(scope="module")
def clouds(pkg, ctx):
    """ending -> (src, tgt, target normals); the planar target with one normal makes the plane system singular."""
    S = pkg.synth
    src, tgt = S.make_pair(21, NS, R=S.rot_axis_angle([0.2, 0.1, 1.0], np.deg2rad(5.0)), t=(0.02, -0.01, 0.03), shape="bumpy")
    tgt = np.ascontiguousarray(tgt[:NT])
    healthy = (src, tgt, ctx.normals(tgt.astype(F64), 20).astype(F32))
    gx, gy = np.meshgrid(np.linspace(-1, 1, 20), np.linspace(-1, 1, 14))
    flat = np.stack([gx.ravel(), gy.ravel(), np.zeros(NT)], 1).astype(F32)
    above = (flat[np.arange(NS) % NT] + np.array([0.01, -0.02, 0.05])).astype(F32)
    planar = (above, flat, np.tile(np.array([0, 0, 1], F32), (NT, 1)))
    assert len(src) == NS and len(tgt) == NT and len(above) == NS
    return {e: planar if e == "degenerate" else healthy for e in ENDINGS}


def _params(ctx, ending):
    if ending == "max_iterations_0":
        return ctx.icp_params(max_iterations=0)
    if ending == "too_few_at_pass_1":
        return ctx.icp_params(min_correspondences=NS + 1)   # more than there are sources
    return ctx.icp_params(max_iterations=200)   # (the trace below holds 256 passes)


def _trimmed(pkg, ctx, src, tgt, nrm, ending):
    single = ctx.icp_trimmed(src, tgt, nrm, 0.7, pkg.METRIC_PLANE, params=_params(ctx, ending), trace_cap=256)
    res, info, extra = ctx.icp_trimmed_batch(src, [0, NS], tgt, [0, NT], nrm, None, 0.7, pkg.METRIC_PLANE, params=_params(ctx, ending),
                                             trace_cap=256)
    return single, single["trim_info"], "trace_trim", res[0], info[0], extra


def _robust(pkg, ctx, src, tgt, nrm, ending):
    def rp():
        return pkg.robust_params(pkg.LOSS_HUBER, pkg.METRIC_PLANE, scale=0.0)
    single = ctx.icp_robust(src, tgt, nrm, rp=rp(), params=_params(ctx, ending), trace_cap=256)
    res, info, extra = ctx.icp_robust_batch(src, [0, NS], tgt, [0, NT], nrm, rp=rp(), params=_params(ctx, ending), trace_cap=256)
    return single, single["robust_info"], "trace_robust", res[0], info[0], extra


@pytest.mark.parametrize("ending", ENDINGS)
@pytest.mark.parametrize("form", [_trimmed, _robust], ids=["trimmed", "robust"])
def test_info_and_trace_at_every_ending(pkg, ctx, clouds, form, ending):
    src, tgt, nrm = clouds[ending]
    single, s_info, tname, r, b_info, extra = form(pkg, ctx, src, tgt, nrm, ending)
    n_trace = len(single["trace_sums"])
    print("%s, %s: %d passes, state %d, converged %d, %d traced, info %s" % (form.__name__, ending, single["iterations"], single["state"],
                                                                             single["converged"], n_trace, s_info))
    # the single call against the batch of one, exactly
    assert r.iterations == single["iterations"] and r.state == single["state"] and bool(r.converged) == single["converged"]
    assert np.array_equal(_bits(r.matrix()), _bits(single["T"]))
    assert np.array_equal(_bits(np.array([r.last_mse])), _bits(np.array([single["last_mse"]])))
    assert abs(r.fitness - single["fitness"]) <= 2.0 * NS * 2.0 ** -53 * single["fitness"]   # two orders of one f64 sum of NS terms
    assert np.array_equal(_bits(b_info), _bits(s_info))
    for k in ("trace_sums", "trace_Tk", tname):
        assert extra[k].shape == single[k].shape and np.array_equal(_bits(extra[k]), _bits(single[k])), k
    assert len(single[tname]) == n_trace
    # what the ending leaves behind
    if ending == "converged":
        assert single["converged"] and single["iterations"] >= 1 and n_trace == single["iterations"]
        assert np.array_equal(_bits(single[tname][-1]), _bits(s_info))          # the last traced pass is the last pass
        return
    assert single["iterations"] == 0 and not single["converged"] and n_trace == 0   # (a pass is traced once its step is made)
    assert np.array_equal(single["T"], np.eye(4, dtype=F32))
    if ending == "max_iterations_0":
        assert np.array_equal(_bits(s_info), _bits(np.zeros(4)))                # no pass ran: the record as it was zeroed at entry
    else:
        assert single["state"] == (pkg.STATE_DEGENERATE if ending == "degenerate" else NO_CORRESPONDENCES)
        assert s_info[0] > 0                                                    # pass 1 ran: m candidates
