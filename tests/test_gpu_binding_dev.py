"""The _dev wrappers of binding.Context that no other GPU test calls -- p2l_sums_dev, icp_sim_dev, icp_sim_batch_dev -- give the
bits of their host forms on the same clouds (a host entry and its _dev twin enter one function: DESIGN.md 2.27, 2.32).  64 sources
against 80 targets; the batch two ragged pairs of 64 / 48 sources against 80 / 56 targets."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == F64 else np.uint32)


def _pair(seed, ns, nt):
    """ns sources that are targets shrunk by 3 % and shifted: similarity ICP has a scale to find"""
    rng = np.random.default_rng(seed)
    tgt = rng.uniform(-1, 1, (nt, 3)).astype(F32)
    src = (tgt[rng.permutation(nt)[:ns]] * F32(0.97) + F32(0.01)).astype(F32)
    return src, tgt


def _same(res, T, fitness, last_mse, iterations, converged, state):
    assert np.array_equal(_bits(res.matrix()), _bits(T))
    assert np.array_equal(_bits(np.array([res.fitness, res.last_mse])), _bits(np.array([fitness, last_mse], F64)))
    assert (res.iterations, bool(res.converged), res.state) == (iterations, bool(converged), state)


def test_p2l_sums_dev(pkg, ctx):
    import torch
    src, tgt = _pair(1, 64, 80)
    rng = np.random.default_rng(2)
    nrm = rng.normal(size=(80, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F32)
    idx = rng.integers(0, 80, 64).astype(np.int32)
    host = ctx.p2l_sums(src, tgt, nrm, idx, 0.25)
    s, t, n, i = (torch.from_numpy(x).cuda() for x in (src, tgt, nrm, idx))
    torch.cuda.synchronize()
    dev = ctx.p2l_sums_dev(s.data_ptr(), t.data_ptr(), n.data_ptr(), i.data_ptr(), 64, 80, 0.25)
    assert dev.shape == (pkg.P2L_NSUMS,) and 0 < dev[0] <= 64
    assert np.array_equal(_bits(dev), _bits(host))


def test_icp_sim_dev(pkg, ctx):
    import torch
    src, tgt = _pair(3, 64, 80)
    host = ctx.icp_sim(src, tgt, sp=pkg.sim_params(overlap=0.9))
    s, t = (torch.from_numpy(x).cuda() for x in (src, tgt))
    torch.cuda.synchronize()
    res, info = ctx.icp_sim_dev(s.data_ptr(), 64, t.data_ptr(), 80, ctx.icp_params(), sp=pkg.sim_params(overlap=0.9))
    assert res.iterations >= 1 and info.shape == (pkg.SIM_NINFO,) and info[5] > 0
    _same(res, host["T"], host["fitness"], host["last_mse"], host["iterations"], host["converged"], host["state"])
    assert np.array_equal(_bits(info), _bits(host["sim_info"]))


def test_icp_sim_batch_dev(pkg, ctx):
    import torch
    (s0, t0), (s1, t1) = _pair(4, 64, 80), _pair(5, 48, 56)
    src, tgt = np.concatenate([s0, s1]), np.concatenate([t0, t1])
    so, to = np.array([0, 64, 112], np.int64), np.array([0, 80, 136], np.int64)
    overlaps = np.array([0.9, 1.0])
    host, host_info, _ = ctx.icp_sim_batch(src, so, tgt, to, overlaps=overlaps)
    s, t = (torch.from_numpy(x).cuda() for x in (src, tgt))
    torch.cuda.synchronize()
    res, info = ctx.icp_sim_batch_dev(s.data_ptr(), so, t.data_ptr(), to, ctx.icp_params(), overlaps=overlaps)
    assert isinstance(res, list) and len(res) == 2 and info.shape == (2, pkg.SIM_NINFO)
    for r, h in zip(res, host):
        assert r.iterations >= 1
        _same(r, h.matrix(), h.fitness, h.last_mse, h.iterations, h.converged, h.state)
    assert np.array_equal(_bits(info), _bits(host_info))
