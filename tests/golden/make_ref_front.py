#!/usr/bin/env python3
"""Records the compiled reference front end into tests/golden/ref_front.npz (data only: inputs and results).

Runs oracle/_ref/kss_ref_front -- the reference's own initRegistration_KSS and PCR_QM classes behind oracle/ref_front.cpp,
built by `make -C oracle -f Makefile.ref` where the reference tree exists -- on the six front inputs and the five PCR_QM
inputs of tests/ref_front.py, and stores every input next to its record.  Run where that binary has been built:

    python tests/golden/make_ref_front.py

Keys: front_names; per front case <name>_dims (ns, nt, g, nl) and <name>, one float64 vector holding S, T, step and the
record's fields in the order of tests/ref_front.py:_shapes; qm_names, qm_sizes, qm_results and qm_A: PCR_QM case i aligns
qm_A[:na] to the first nt points of the first front case's target.  A one-point source is deliberately absent: the
reference divides by its zero mean radius (initRegistrationKSS.hpp:209) and records inf/NaN."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import ref_front as RF  # noqa: E402

LIMIT = 300 * 1000


def main():
    if not RF.have_binary():
        sys.exit("build oracle/_ref/kss_ref_front first (make -C oracle -f Makefile.ref)")
    out = {}
    names = []
    for name, S, T, step in RF.front_cases():
        rec = RF.ref_front(S, T, step)
        for v in rec.values():
            assert np.isfinite(v).all(), name
        out[name + "_dims"], out[name] = RF.pack_front(S, T, step, rec)
        names.append(name)
        print(name, "ns=%d nt=%d step=%g g=%d nl=%d angle=%s" % (len(S), len(T), step, rec["g"], len(rec["angle_list"]), rec["angle"]))
    qm = RF.qm_cases()
    tmpl = RF.front_cases()[0][2]
    pool = max((A for _, A, _ in qm), key=len)
    for name, A, T in qm:
        assert RF.same_bits(A, pool[:len(A)]) and RF.same_bits(T, tmpl[:len(T)])
        print(name, RF.ref_qm(A, T))
    out["qm_A"] = pool
    out["qm_sizes"] = np.array([[len(A), len(T)] for _, A, T in qm], np.int64)
    out["qm_results"] = np.array([RF.ref_qm(A, T) for _, A, T in qm])
    out["front_names"], out["qm_names"] = np.array(names), np.array([n for n, _, _ in qm])
    np.savez_compressed(RF.FIXTURE, **out)
    size = os.path.getsize(RF.FIXTURE)
    print("%s: %d bytes" % (RF.FIXTURE, size))
    assert size < LIMIT, size


if __name__ == "__main__":
    main()
