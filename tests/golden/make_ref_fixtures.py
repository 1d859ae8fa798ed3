#!/usr/bin/env python3
"""Packs the reference's own registration DATA files into two .npz fixtures (data only: point coordinates).

Source: /root/reference/PS_AIS_Simplification/data/registration/*.{gird,wlop} (10 pairs; ground-truth rotations in
transfer.txt, plain-ICP outcome list in ICP.txt -- both already copied as text next to this script's output) and
data/registration_scale/*.{gird,wlop} (13 pairs, source also scaled and translated: transferPC.hpp:100-138, parameters
not recorded by the reference).  Format of the inputs: first line N, then N lines "x y z" (Main_KSS_List.cpp:65-94).
<name>.gird = source (rotated grid resampling), <name>.wlop = target (WLOP resampling), transferPC.hpp:140-160.
Run in the build container (the reference tree does not travel):  python tests/golden/make_ref_fixtures.py

Each fixture is written as parts, <sub>_all.part<k>.npz, so that no file exceeds 1 MiB: an array of more than
CHUNK_ROWS rows is stored as row blocks "<key>.0", "<key>.1", ..., and the blocks are packed into parts of at most
PART_BYTES uncompressed bytes.  tests/test_oracle.py:_ref_npz reassembles them.
"""
import os

import numpy as np

REF = "/root/reference/PS_AIS_Simplification/data"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref_data")
CHUNK_ROWS = 24000
PART_BYTES = 960000


def write_parts(out_dir, sub, names, arrays):
    """Writes `names` and the dict `arrays` (key -> array, in order) as <sub>_all.part<k>.npz files under 1 MiB each."""
    blocks = []
    for key, a in arrays.items():
        if len(a) <= CHUNK_ROWS:
            blocks.append((key, a))
        else:
            blocks += [("%s.%d" % (key, i), a[lo:lo + CHUNK_ROWS]) for i, lo in enumerate(range(0, len(a), CHUNK_ROWS))]
    parts, cur, size = [], {"names": np.array(names)}, 0
    for key, a in blocks:
        if cur and size + a.nbytes > PART_BYTES:
            parts.append(cur)
            cur, size = {}, 0
        cur[key] = a
        size += a.nbytes
    parts.append(cur)
    for k, part in enumerate(parts):
        np.savez_compressed(os.path.join(out_dir, "%s_all.part%d.npz" % (sub, k)), **part)
    return len(parts)


def pack(sub):
    d = os.path.join(REF, sub)
    names = sorted({f[:-5] for f in os.listdir(d) if f.endswith(".gird")})
    arrays = {}
    for n in names:
        for ext in ("gird", "wlop"):
            a = np.loadtxt(os.path.join(d, n + "." + ext), skiprows=1, dtype=np.float64)
            cnt = int(open(os.path.join(d, n + "." + ext)).readline().split()[0])
            assert a.shape == (cnt, 3), (n, ext, a.shape, cnt)
            arrays["%s_%s" % (n, ext)] = a
    write_parts(OUT, sub, names, arrays)
    return names


if __name__ == "__main__":
    for sub in ("registration", "registration_scale"):
        print(sub, pack(sub))
