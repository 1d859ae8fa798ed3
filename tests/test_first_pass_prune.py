"""CPU property test of the first pass's two-stage walk (kss_grid.hip, block_walk_first): a query that
arrives without a candidate walks its own x-row first, takes the best distance found there (grown by the skin) as its pruning
radius and queues the other 8 rows of the 3x3x3 block under block_walk's rule.  The rule is restated here in numpy float32
(same expressions, same order, no fma), followed by the kernel's termination test, shells and fallback; for every query

  - the winner (d2, index) must be the brute-force one in the kernel's own arithmetic (ties -> lowest index), and
  - the bound B it stores for the skip test must not exceed the true distance of any target other than the winner.

This pins the MATHEMATICS -- the kernels themselves are checked bit for bit on the GPU (tests/test_gpu_first_pass.py)."""
import numpy as np

f32 = np.float32
INF = f32(np.inf)
M6 = f32(0.999999)


def dist2(q, P):
    """(dx*dx + dy*dy) + dz*dz in f32, no fma, dx = q - p: point_key's arithmetic"""
    d = (q - P).astype(f32)
    return ((d[:, 0] * d[:, 0]).astype(f32) + (d[:, 1] * d[:, 1]).astype(f32)).astype(f32) + (d[:, 2] * d[:, 2]).astype(f32)


class Grid:
    """choose_cells (kss_engine.hip) and the cell list, in f32"""

    def __init__(self, T, hscale=2.0, rcap=4):
        self.T = T
        mn, mx = T.min(axis=0), T.max(axis=0)
        ext = (mx - mn).astype(f32)
        emax = f32(ext.max())
        h = f32(f32(emax * f32(hscale)) * f32(np.sqrt(f32(f32(3.0) / f32(len(T))))))
        h = max(h, f32(emax / f32(255.5)))
        if not h > 0:
            h = f32(1.0)
        self.o = mn.astype(f32)
        self.h = f32(h)
        self.inv_h = f32(f32(1.0) / self.h)
        self.g = [max(1, min(256, int(np.floor(f32(e / self.h))) + 1)) for e in ext]
        mag = f32(max(np.abs(mn).max(), np.abs(mx).max()))
        self.eps = f32(f32(f32(2e-6) * f32(mag + emax)) + f32(1e-30))
        self.rcap = rcap
        self.cells = {}
        for i, p in enumerate(T):
            self.cells.setdefault(self.cell(p), []).append(i)

    def coord(self, v, k):
        c = int(np.floor(f32(f32(v - self.o[k]) * self.inv_h)))
        return min(max(c, 0), self.g[k] - 1)

    def cell(self, p):
        return (self.coord(p[0], 0), self.coord(p[1], 1), self.coord(p[2], 2))

    def members(self, cx, cy, cz):
        if not (0 <= cx < self.g[0] and 0 <= cy < self.g[1] and 0 <= cz < self.g[2]):
            return []
        return self.cells.get((cx, cy, cz), [])


class Walk:
    """key / m1 / m2 bookkeeping of a walk: best (d2, index), the two smallest distances over the distinct points walked"""

    def __init__(self, q, T):
        self.q, self.T = q, T
        self.key = None
        self.m1 = self.m2 = INF
        self.evals = 0

    def take(self, idx, track=True):
        if not idx:
            return
        idx = np.asarray(idx)
        d = dist2(self.q, self.T[idx])
        self.evals += len(idx)
        for dd, i in zip(d, idx):
            k = (f32(dd), int(i))
            if self.key is None or k < self.key:
                self.key = k
            if track:
                self.m1, self.m2 = min(self.m1, f32(dd)), sorted([self.m1, self.m2, f32(dd)])[1]


def first_pass_query(G, q, skin=0.25, two_stage=True):
    """-> (index or None, d2, B, evaluations of the r = 1 block, own row found a point)"""
    T = G.T
    if not np.isfinite(q).all():
        return None, None, f32(0), 0, False
    cx, cy, cz = G.cell(q)
    W = Walk(q, T)
    rho = INF
    own = False
    if two_stage:
        for dx in (-1, 0, 1):
            W.take(G.members(cx + dx, cy, cz))
        if W.key is not None:
            own = True
            d0 = W.key[0]
            grown = f32(f32(np.sqrt(d0)) + f32(f32(max(skin, 0.0)) * G.h))
            rho = max(d0, f32(grown * grown)) if skin >= 0 else d0
    o, h, eps = G.o, G.h, G.eps

    def gaps(v, c, k):
        lo = max(f32(f32(v - f32(o[k] + f32(f32(c) * h))) - eps), f32(0))
        hi = max(f32(f32(f32(o[k] + f32(f32(c + 1) * h)) - v) - eps), f32(0))
        return lo, hi
    exl, exr = gaps(q[0], cx, 0)
    eyl, eyr = gaps(q[1], cy, 1)
    ezl, ezr = gaps(q[2], cz, 2)
    exl2, exr2 = f32(exl * exl), f32(exr * exr)
    ey2 = [f32(eyl * eyl), f32(0), f32(eyr * eyr)]
    ez2 = [f32(ezl * ezl), f32(0), f32(ezr * ezr)]
    for t in range(9):
        if two_stage and t == 4:
            continue
        z, y = cz + t // 3 - 1, cy + t % 3 - 1
        ok = 0 <= z < G.g[2] and 0 <= y < G.g[1]
        g2 = f32(ey2[t % 3] + ez2[t // 3])
        if not ok or rho < f32(g2 * M6):
            continue
        left = not rho < f32(f32(g2 + exl2) * M6)
        right = not rho < f32(f32(g2 + exr2) * M6)
        if left:
            W.take(G.members(cx - 1, y, z))
        W.take(G.members(cx, y, z))
        if right:
            W.take(G.members(cx + 1, y, z))
    block_evals = W.evals
    # the shell loop of serve_walkers
    done, rfin, face2 = False, 0, INF
    for r in range(1, G.rcap + 1):
        if r > 1:
            for dz in range(-r, r + 1):
                for dy in range(-r, r + 1):
                    for dx in range(-r, r + 1):
                        if max(abs(dx), abs(dy), abs(dz)) == r:
                            W.take(G.members(cx + dx, cy + dy, cz + dz), track=False)
        best = W.key[0] if W.key is not None else INF   # (no candidate: key = ~0, whose distance bits are a NaN: no test passes)
        b = INF
        c = (cx, cy, cz)
        for k in range(3):
            if c[k] - r > 0:
                b = min(b, f32(q[k] - f32(o[k] + f32(f32(c[k] - r) * h))))
            if c[k] + r < G.g[k] - 1:
                b = min(b, f32(f32(o[k] + f32(f32(c[k] + r + 1) * h)) - q[k]))
        bs = f32(b - eps)
        if b == INF:
            done = True
        elif W.key is not None and bs > 0 and best < f32(f32(bs * bs) * M6):
            done, face2 = True, f32(bs * bs)
        if done:
            rfin = r
            break
    B = f32(0)
    if not done:   # the list fallback: brute force
        d = dist2(q, T)
        i = int(np.lexsort((np.arange(len(T)), d))[0])
        return i, f32(d[i]), B, block_evals, own
    if W.key is None:
        return None, None, B, block_evals, own
    if rfin == 1:
        B = min(f32(f32(np.sqrt(f32(min(W.m2, rho, face2) * f32(0.99999)))) * M6), f32(1e30))
    return W.key[1], W.key[0], B, block_evals, own


def check_cloud(T, Q, skin=0.25):
    """every query of Q against target T: winner == brute force, B below every other target's true distance"""
    G = Grid(T)
    T64 = T.astype(np.float64)
    stats = dict(two=0, full=0, own=0, empty_own=0, bounded=0, fallback_or_shell=0)
    for q in Q:
        idx, d2, B, ev, own = first_pass_query(G, q, skin)
        _, _, _, ev_full, _ = first_pass_query(G, q, skin, two_stage=False)
        d = dist2(q, T)
        w = int(np.lexsort((np.arange(len(T)), d))[0])
        assert idx == w and d2 == d[w], (q, idx, w, d2, d[w])
        if len(T) > 1:
            true = np.sqrt(((T64 - q.astype(np.float64)) ** 2).sum(axis=1))
            others = np.delete(true, w)
            assert float(B) <= others.min(), (q, float(B), others.min())
        assert ev <= ev_full
        stats["two"] += ev
        stats["full"] += ev_full
        stats["own" if own else "empty_own"] += 1
        stats["bounded" if B > 0 else "fallback_or_shell"] += 1
    return stats


def surface(rng, n, scale=1.0):
    """a bumpy closed surface: the kind of cloud the cell size is chosen for"""
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    r = 1.0 + 0.15 * np.sin(5 * u[:, 0]) * np.cos(4 * u[:, 1])
    return (u * r[:, None] * scale).astype(f32)


def test_random_surface_clouds():
    rng = np.random.default_rng(11)
    tot = dict(two=0, full=0, own=0, empty_own=0)
    for scale, skin in ((1.0, 0.25), (40.0, 0.25), (1e-2, -1.0)):
        T = surface(rng, 3000, scale)
        Q = (surface(rng, 250, scale) + rng.normal(size=(250, 3)).astype(f32) * f32(0.01 * scale)).astype(f32)
        s = check_cloud(T, Q, skin)
        for k in tot:
            tot[k] += s[k]
        assert s["bounded"] > 200, s
    # the point of the rule: well under the full block's evaluations (the estimate for C2 is ~20 of ~45)
    assert tot["own"] > 600 and tot["two"] < 0.7 * tot["full"], tot


def test_integer_lattice_exact_ties():
    # targets on an 8^3 integer lattice, queries on cell mid-points, edge mid-points and lattice points: 8-, 2- and 1-way ties in
    # exact f32 arithmetic; the lowest index must win whichever row it sits in
    g = np.arange(8, dtype=f32)
    T = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(f32)
    rng = np.random.default_rng(3)
    T = T[rng.permutation(len(T))]
    c = rng.integers(0, 7, size=(120, 3)).astype(f32)
    Q = np.concatenate([c + f32(0.5), c + np.array([0.5, 0, 0], f32), c + np.array([0, 0.5, 0.5], f32), c])
    s = check_cloud(T, Q.astype(f32))
    assert s["own"] > 300, s


def test_queries_outside_the_box():
    rng = np.random.default_rng(7)
    T = surface(rng, 1500)
    u = rng.normal(size=(200, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    rad = np.where(np.arange(200) % 2 == 0, rng.uniform(1.0, 1.3, size=200), rng.uniform(1.3, 4.0, size=200))
    Q = (u * rad[:, None]).astype(f32)   # from just off the surface to far beyond the box: the block, the shells, then the list
    outside = ((Q < T.min(axis=0)) | (Q > T.max(axis=0))).any(axis=1).sum()
    s = check_cloud(T, Q)
    assert outside > 100 and s["fallback_or_shell"] > 20 and s["bounded"] > 20, (outside, s)


def test_empty_own_rows():
    # two thin sheets a few cells apart and queries between them: the own row is empty for many, rho stays +inf
    rng = np.random.default_rng(9)
    n = 1200
    xy = rng.uniform(0, 1, size=(n, 2))
    z = np.where(np.arange(n) % 2 == 0, 0.0, 0.35)   # (cell edge 0.1: the sheets are in z-cells 0 and 3, cells 1 and 2 are empty)
    T = np.column_stack([xy, z]).astype(f32)
    Q = np.column_stack([rng.uniform(0, 1, size=(250, 2)), rng.uniform(0.0, 0.35, size=250)]).astype(f32)
    s = check_cloud(T, Q)
    assert s["empty_own"] > 50 and s["own"] > 0, s


def test_single_target_and_non_finite_query():
    T = np.array([[0.25, -1.5, 3.0]], f32)
    rng = np.random.default_rng(1)
    Q = (T[0] + rng.normal(size=(40, 3))).astype(f32)
    check_cloud(T, Q)
    G = Grid(T)
    assert first_pass_query(G, np.array([np.nan, 0, 0], f32))[0] is None
    assert first_pass_query(G, np.array([0, np.inf, 0], f32))[0] is None
