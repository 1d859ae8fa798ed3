"""What Context.icp_vgicp_batch / icp_vgicp_batch_dev hand to their C symbols, without a GPU: through the recording proxy and the
inputs of tests/test_binding_calls.py (imported, not edited: its ragged batch of 5 + 3 points as two scans, its fake map handle)."""
import numpy as np
import pytest

import test_binding_calls as B


@pytest.fixture(scope="module")
def world(pkg):
    return B.World(pkg.binding, pkg.load_library())


CASES = {
    "icp_vgicp_batch": (lambda c, w: c.icp_vgicp_batch(w.src_all, w.so, w.map, src_normals_all=w.snrm_all, epsilons=w.epsilons, gp=w.gp(),
                                                       params=w.p(), trace_cap=2),
                        lambda c, w: c.icp_vgicp_batch(w.src_all, w.so, w.map)),
    "icp_vgicp_batch_dev": (lambda c, w: c.icp_vgicp_batch_dev(w.d_src, w.so, w.d_snrm, w.map, w.p(), epsilons=w.epsilons, gp=w.gp()),
                            lambda c, w: c.icp_vgicp_batch_dev(w.d_src, w.so, None, w.map, w.p())),
}


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("name", sorted(CASES))
def test_one_call_to_its_own_symbol(world, name, kind):
    """Exactly one compute call, to kss_<method>, with the 11 arguments the symbol declares, each accepted by its argtype."""
    world.proxy.faults = []
    calls, out, _ = B.run(world, CASES[name][kind])
    assert world.proxy.faults == []
    assert [c["symbol"] for c in calls] == ["kss_" + name]
    args = calls[0]["args"]
    assert len(args) == 11
    dev = name.endswith("_dev")
    full = kind == 0
    assert args[1] == ("d_src" if dev else "src_all") and args[2] == "so"
    assert args[3] == ((("d_snrm" if dev else "snrm_all")) if full else None)
    assert args[4] == 2 and args[5] == "vmap"
    assert args[6]["byref"] == "IcpParams" and args[7]["byref"] == "GicpParams"
    assert args[6]["trace_cap"] == (2 if full and not dev else 0)
    assert args[7]["epsilon"] == (2e-3 if full else 1e-3)
    assert args[8] == ("epsilons" if full else None)
    assert args[9] == "fresh buffer" and args[10] == "fresh buffer"
    if dev:
        assert out == {"tuple": [{"list": ["IcpResult", "IcpResult"]}, {"ndarray": [2, 4], "dtype": "float64"}]}
    else:
        assert set(out) == {"list"} and len(out["list"]) == 2
        keys = {"T", "iterations", "converged", "state", "fitness", "last_mse", "info", "pair_id"}
        assert set(out["list"][1]["dict"]) == keys
        assert set(out["list"][0]["dict"]) == (keys | {"trace_sums", "trace_Tk"} if full else keys)
        assert out["list"][0]["dict"]["info"] == {"ndarray": [4], "dtype": "float64"}


@pytest.mark.parametrize("rc", [0, -1])
@pytest.mark.parametrize("name", sorted(CASES))
def test_detach(world, name, rc):
    """After the call -- returned, or raised as KssError -- no params struct still points at the call's arrays."""
    calls, out, structs = B.run(world, CASES[name][0], rc)
    assert len(calls) == 1
    assert (out == "KssError -1") == (rc != 0)
    assert len(structs) >= 2
    for st in structs:
        assert [f for f in B._ptr_fields(st) if getattr(st, f)] == [], (name, type(st).__name__)
        if hasattr(st, "trace_cap"):
            assert st.trace_cap == 0


def test_value_errors(world):
    c, w = world.ctx, world
    with pytest.raises(ValueError) as e:
        c.icp_vgicp_batch(w.src_all, w.so, w.map, src_normals_all=w.nrm_all)
    assert str(e.value) == "source normals must have one row per point"
    for call in (lambda: c.icp_vgicp_batch(w.src_all, w.so, w.map, epsilons=np.zeros(3)),
                 lambda: c.icp_vgicp_batch_dev(w.d_src, w.so, None, w.map, w.p(), epsilons=np.zeros(3))):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == "epsilons must hold one entry per pair"


def test_methods_sit_outside_the_recorded_span(pkg):
    """tests/test_binding_calls.py demands a recorded case for every public method between icp() and icp_dev(): these two come later."""
    src = open(pkg.binding.__file__.replace(".pyc", ".py")).read()
    assert src.index("    def icp_vgicp_batch(self") > src.index("    def icp_batch_dev(self")
    assert src.index("    def icp_vgicp_batch_dev(self") > src.index("    def icp_batch_dev(self")
