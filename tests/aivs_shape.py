"""Which path of the AIVS sampler does a cloud drive?  A numpy restatement of the box grid, and the designed clouds.

No GPU and no oracle in here.  `aivs_fps_box` (kss-icp_amd/csrc/kss_aivs.hip) samples one box on one of three paths:

  fast              the box holds m <= FAST_MAX own points and at most L2_CAP already-sampled neighbour points lie in
                    its search cube (`aivs_fps_fast`: own points in registers, four slots of WAVE lanes);
  general, list     m > FAST_MAX, or the fast path gave up, and at most L2_CAP neighbour samples in reach (`l2[]` in LDS);
  general, re-scan  more than L2_CAP neighbour samples in reach: the neighbour boxes are walked again for every own point.

Each has a "seed the box centre" form (no neighbour sample in reach) and a "no seed" form.  `box_stats` restates the grid
of `aivs_device` / `aivs_box_of` and bounds, per occupied box, the number of neighbour samples in reach, so that a test
can assert which path its input takes before it compares the device with the oracle.

tests/test_aivs_shape_host.py checks every designed cloud's premise on the CPU; tests/test_gpu_aivs_paths.py runs them."""
import collections

import numpy as np

# the thresholds of kss_aivs.hip: the wave width, `m <= 4 * 64` in aivs_fps_box, `constexpr int L2_CAP = 512` there
WAVE = 64
FAST_MAX = 4 * WAVE
L2_CAP = 512

# Method_AIVS_SimPro.hpp:609-632 as `order[8][3]` in aivs_device: the parities (x, y, z) of the 1-based box coordinates
COLOUR_ORDER = ((1, 1, 1), (0, 1, 1), (0, 0, 1), (1, 0, 1), (1, 1, 0), (0, 1, 0), (0, 0, 0), (1, 0, 0))

Grid = collections.namedtuple("Grid", "box_num unit nx ny nz mins R")
BoxStats = collections.namedtuple("BoxStats", "grid box coords centre colour m budget reach_lo reach_hi point_box")


def box_num(n):
    """BallRegion_EstimateBoxScale: boxes along the largest extent, by cloud size."""
    if n < 10000:
        return 10
    if n < 50000:
        return 20
    if n < 100000:
        return 30
    if n < 500000:
        return 40
    if n < 1000000:
        return 50
    return int((n / 8.0) ** (1.0 / 3.0))


def grid_of(P):
    P = np.asarray(P, np.float64).reshape(-1, 3)
    mins, maxs = P.min(axis=0), P.max(axis=0)
    ext = np.abs(maxs - mins)
    bn = box_num(len(P))
    unit = ext.max() / float(bn)
    num = ext / unit
    dims = num.astype(np.int64)
    dims += num > dims                      # the round-up rule
    return Grid(bn, unit, int(dims[0]), int(dims[1]), int(dims[2]), mins, unit * 3.0 / 4.0)


def box_coords(P, g):
    """1-based box coordinates of every point (aivs_box_of): int(f), plus one if int(f) < f or int(f) == 0."""
    f = (np.asarray(P, np.float64).reshape(-1, 3) - g.mins) / g.unit
    c = f.astype(np.int64)                  # truncation; f >= 0
    c += (c < f) | (c == 0)
    return c


def colour_of(coords):
    """Position of a box in the eight-colour order, from the parity of its coordinates."""
    par = np.asarray(coords) % 2
    lut = np.empty(8, np.int64)
    for pos, (px, py, pz) in enumerate(COLOUR_ORDER):
        lut[px * 4 + py * 2 + pz] = pos
    return lut[par[..., 0] * 4 + par[..., 1] * 2 + par[..., 2]]


def _decode(box, g):
    """aivs_box_center's inverse of the linear index (a multiple of nx is the last column of the row before)."""
    bz = box // (g.nx * g.ny) + 1
    in_layer = box % (g.nx * g.ny)
    by = in_layer // g.nx + 1
    bx = in_layer % g.nx
    if bx == 0:
        bx, by = g.nx, by - 1
    return bx, by, bz


def _neighbours(box, g):
    """aivs_neighbor_boxes, the un-wrapped last x column included."""
    z_num = box // (g.nx * g.ny) + 1
    in_layer = box % (g.nx * g.ny)
    y_num = in_layer // g.nx + 1
    x_num = in_layer % g.nx
    xs = [v for v in (x_num - 1, x_num, x_num + 1) if (v != x_num - 1 or x_num > 1) and (v != x_num + 1 or x_num < g.nx)]
    ys = [v for v in (y_num - 1, y_num, y_num + 1) if (v != y_num - 1 or y_num > 1) and (v != y_num + 1 or y_num < g.ny)]
    zs = [v for v in (z_num - 1, z_num, z_num + 1) if (v != z_num - 1 or z_num > 1) and (v != z_num + 1 or z_num < g.nz)]
    out = []
    for x in xs:
        for y in ys:
            for z in zs:
                if (x, y, z) == (x_num, y_num, z_num):
                    continue
                idx = x + (y - 1) * g.nx + (z - 1) * g.nx * g.ny
                if 0 <= idx < g.nx * g.ny * g.nz + 1:
                    out.append(idx)
    return out


def budgets(m, n, point_num):
    """AIVS_BoxSimplification_Points (`sim_num` in aivs_box_info_kernel): m * rate, rounded up past a fraction of 0.2."""
    sim = np.asarray(m, np.float64) * (float(point_num) / float(n))
    t = sim.astype(np.int64)
    return t + (sim - t > 0.2)


def box_stats(P, selection=None, point_num=None):
    """Per occupied box: population m and bounds on the already-sampled neighbour points in its search cube at the
    moment the box is processed.

    reach_hi counts ALL points of the neighbour boxes of earlier colours that lie inside the cube (half side R = 0.75 unit
    around the box centre): no more than these can have been sampled.  With `point_num` given, a neighbour box contributes
    no more than its sampling budget either: its loop stops at `simNum` samples.  reach_lo counts the points in those
    boxes and that cube that are in `selection`, a final selection of the sampler: the accurate cut only removes samples,
    so everything in the final selection had been sampled when the box ran.  Without `selection`, reach_lo is 0.  A box
    of the first colour has both bounds 0.  (Boxes of one colour run side by side; a neighbour of the same colour is
    counted on neither side.)"""
    P = np.asarray(P, np.float64).reshape(-1, 3)
    g = grid_of(P)
    c = box_coords(P, g)
    lin = c[:, 0] + g.nx * (c[:, 1] - 1) + g.nx * g.ny * (c[:, 2] - 1)
    order = np.argsort(lin, kind="stable")
    boxes, first, m = np.unique(lin[order], return_index=True, return_counts=True)
    where = {int(b): (int(s), int(s + k)) for b, s, k in zip(boxes, first, m)}
    sel = np.zeros(len(P), bool)
    if selection is not None:
        sel[np.asarray(selection, np.int64)] = True
    budget = budgets(m, len(P), point_num) if point_num is not None else m.copy()
    budget_by_box = dict(zip(boxes.tolist(), budget.tolist()))
    coords = np.array([_decode(int(b), g) for b in boxes], np.int64).reshape(-1, 3)
    centre = (g.mins + (coords - 1) * g.unit + g.mins + coords * g.unit) / 2
    colour = colour_of(coords)
    colour_by_box = dict(zip(boxes.tolist(), colour.tolist()))
    lo, hi = np.zeros(len(boxes), np.int64), np.zeros(len(boxes), np.int64)
    for k, b in enumerate(boxes.tolist()):
        if colour[k] == 0:
            continue
        for q in _neighbours(b, g):
            if q not in where or colour_by_box[q] >= colour[k]:
                continue
            pts = order[where[q][0]:where[q][1]]
            inside = ((P[pts] <= centre[k] + g.R) & (P[pts] >= centre[k] - g.R)).all(axis=1)
            hi[k] += min(int(inside.sum()), budget_by_box[q])
            lo[k] += int((inside & sel[pts]).sum())
    return BoxStats(g, boxes, coords, centre, colour, m, budget, lo, hi, lin)


# the six classes a path test can rely on: (own points, neighbour samples in reach) -> the path that is CERTAIN to run
CLASSES = ("fast64_list", "fast256_list", "fast64_seed", "fast256_seed", "fast256_overflow", "fast64_overflow",
           "general_seed", "general_list", "general_rescan")


def classes(st):
    """Number of boxes whose path is certain from the bounds, by class name; boxes the bounds leave open count as 'open'.

    *_seed: reach_hi == 0 (nothing can be in reach: the box centre is seeded).  *_list: reach_lo >= 1 and reach_hi <= L2_CAP
    (no seed; the neighbours fit the LDS list).  *_overflow / general_rescan: reach_lo > L2_CAP (the fast path gives up having
    written nothing, and the general path re-scans the neighbour boxes for every own point)."""
    out = dict.fromkeys(CLASSES + ("open",), 0)
    for m, lo, hi in zip(st.m.tolist(), st.reach_lo.tolist(), st.reach_hi.tolist()):
        size = "fast64" if m <= WAVE else "fast256" if m <= FAST_MAX else "general"
        if hi == 0:
            out[size + "_seed"] += 1
        elif lo >= 1 and hi <= L2_CAP:
            out[size + "_list"] += 1
        elif lo > L2_CAP:
            out[size + ("_rescan" if size == "general" else "_overflow")] += 1
        else:
            out["open"] += 1
    return out


def describe(P, selection=None, point_num=None):
    """One line for an assertion message: the grid, the largest box, the worst reach, the class counts."""
    st = box_stats(P, selection, point_num)
    g = st.grid
    return "n=%d grid=%dx%dx%d unit=%.6g max_m=%d max_reach=[%d, %d] classes=%s" % (
        len(P), g.nx, g.ny, g.nz, g.unit, st.m.max(), st.reach_lo.max(), st.reach_hi.max(),
        {k: v for k, v in classes(st).items() if v})


# ---- the designed clouds -------------------------------------------------------------------------------------------
def clustered(seed, nbg, clusters):
    """`nbg` background points uniform in the unit cube, the first two pinned to (0,0,0) and (1,1,1) so that the bounding
    box is the unit cube and unit = 0.1 below 10,000 points; then for every (ncl, s, centre) in `clusters`, ncl Gaussian
    points of standard deviation s * 0.1 around `centre`, clipped to [0.001, 0.999]; all shuffled."""
    rng = np.random.default_rng(seed)
    parts = [rng.random((nbg, 3))]
    parts[0][0] = 0.0
    parts[0][1] = 1.0
    for ncl, s, centre in clusters:
        parts.append(np.clip(np.asarray(centre, np.float64) + s * 0.1 * rng.standard_normal((ncl, 3)), 0.001, 0.999))
    P = np.concatenate(parts)
    return P[rng.permutation(len(P))]


def cloud_a():
    """A cluster on the common corner of eight boxes: about 750 points in each, one of every colour."""
    return clustered(101, 1500, [(6000, 0.10, (0.5, 0.5, 0.5))])


def cloud_b():
    """An off-centre, wider cluster: boxes of every size class around it, with many neighbour samples in reach."""
    return clustered(202, 1200, [(3300, 0.16, (0.512, 0.47, 0.53))])


def cloud_c():
    """Tight clusters (sigma 0.005) well inside single boxes.  Boxes (5,5,5) and (3,7,3) are of the first colour (all
    coordinates odd), so nothing is in reach: 1,200 points for the general path with seed, 200 for the fast path with
    seed and slots up to 3.  The third cluster fills box (4,7,3), of the second colour; the cluster of (3,7,3) sits close
    to their common face, inside the cube of (4,7,3): the fast path without seed, slots up to 3."""
    return clustered(303, 1500, [(1200, 0.05, (0.45, 0.45, 0.45)), (200, 0.05, (0.28, 0.65, 0.25)), (230, 0.05, (0.35, 0.65, 0.25))])


def cloud_d():
    """Cloud B with 600 points overwritten by exact copies of 600 others."""
    P = cloud_b().copy()
    perm = np.random.default_rng(404).permutation(len(P))
    P[perm[:600]] = P[perm[600:1200]]
    return P


def cloud_f_unit_lattice():
    t = np.linspace(0.0, 1.0, 16)
    return np.stack(np.meshgrid(t, t, t, indexing="ij"), axis=-1).reshape(-1, 3)


def cloud_f_int_lattice():
    return np.stack(np.meshgrid(np.arange(20.0), np.arange(20.0), np.arange(10.0), indexing="ij"), axis=-1).reshape(-1, 3)


def cloud_f_int_lattice_permuted():
    P = cloud_f_int_lattice()
    return P[np.random.default_rng(606).permutation(len(P))]


def path_cases(synth):
    """name -> (cloud, point_num) for every single-cloud case; `synth` is the package's generator module."""
    A, B, Cc, D = cloud_a(), cloud_b(), cloud_c(), cloud_d()
    n = len(B)
    tiny = synth.bumpy(10, 64)
    cases = collections.OrderedDict()
    cases["A-corner-cluster-general-seed-list-rescan"] = (A, 3750)
    cases["B-half-fast-noseed-slots123"] = (B, n // 2)
    cases["B-nearfull-fast-overflow-then-rescan"] = (B, n - 100)
    cases["B-full-rate1-overflow"] = (B, n)
    cases["B-over-rate-above-1"] = (B, n + 500)
    cases["C-isolated-general-seed-and-fast-seed"] = (Cc, len(Cc) // 2)
    cases["D-exact-duplicates"] = (D, n // 2)
    cases["E-scaled-1e5"] = (B * 1e5, n // 2)
    cases["E-scaled-1e5-offset-3e6"] = (B * 1e5 + 3e6, n // 2)
    cases["E-scaled-1e6-centre-beyond-9999"] = (B * 1e6, n // 2)
    cases["F-unit-lattice-16"] = (cloud_f_unit_lattice(), 2048)
    cases["F-int-lattice-20x20x10"] = (cloud_f_int_lattice(), 1000)
    cases["F-int-lattice-permuted"] = (cloud_f_int_lattice_permuted(), 3900)
    for k, m in ((2, 1), (3, 1), (4, 2), (5, 3)):
        cases["G-tiny-%d-points" % k] = (tiny[:k], m)
    cases["G-tiny-64-points"] = (tiny, 30)
    return cases
