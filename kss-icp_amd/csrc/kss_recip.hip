// kss_recip.hip -- reciprocal rejection in front of the trimmed pass (PCL's setUseReciprocalCorrespondences; DESIGN.md 2.25, 2.29;
// the definition at kss_icp_recip in include/kssicp.h): a winner i of target j (kss_o2o.hip's) keeps its correspondence only if NO
// source k of its pair has rkey(k, j) = (bits(dist2<nn_fma>(p_k, q_j)) & 0x7fffffff) << 32 | k below key(i).
// "Mutual" is an EXISTENCE statement: which sources are examined, and in what order, cannot change a bit of the result.  That is the
// only reason the sources may sit inside their cell in the order their atomics arrived (launch 4), why the escape of launch 5
// changes nothing, and why the result does not depend on the cell grid.
// ONE kernel family serves one pair and a batch, kss_o2o.hip's way: the launches go over the per-pair descriptors (PairbDesc) and
// grids (RecipPairDev), and a single pair is a batch of one descriptor without the row -> pair table -- {src_base 0, ns, tgt_off 0,
// nt, row_base 0, nrows stream_blocks(ns)}, its grid with cell_base 0, row_pair null (pair 0), state null (every pair is active).
// The lone pair's descriptor and grid travel INSIDE the argument struct (lone_desc, lone_grid), so it stages no table and its
// workgroups read none; every kernel has the template flag LONE, which launch_recip sets where row_pair is null, so that neither
// form pays for the other's loads (DESIGN.md 2.29 has the measurements that decided both).
// Every pair owns its slices of the workspace: its target's slots of the claim table (at tgt_off), its four counters, its cells (at
// cell_base) and its sources' slots of `sorted` (at src_base); i, k and the keys count from 0 INSIDE the pair, src_base + i is where
// a source's idx, d2 and position are.
// Per pass FIVE steps, ONE reset and FOUR launches whatever the pair count, over the NN pass's idx / d2 (by original source index)
// and the sources' current positions:
//   reset     hipMemsetAsync to all ones of the workspace: the claim table (one uint64 per target of the call), four uint32 counters
//             {m, u, r, unused} per pair and one uint32 per cell of every pair.  Counters AND cell counts hold their count MINUS ONE
//             (mod 2^32): one fill serves all.
//   claim     recip_walk_kernel<SRC, false>: kss_o2o.hip's claim -- one 64-bit unsigned atomicMin per candidate, m by ballot and
//             popcount -- and, in the same walk, every source with a finite position adds one to its cell's count (an integer atomic
//             without return value; the cells are many, so the adds spread; a wave whose lanes all meet ONE cell issues one add of
//             its popcount).  A position that is not finite is not binned.
//   scan      recip_scan_kernel: ONE workgroup of 1024 per pair turns the pair's counts into exclusive starts, in place (coalesced
//             tiles of 64 per wave): the starts count from the pair's slice of `sorted`.
//   scatter   recip_walk_kernel<SRC, true>: every binned source takes the next slot of its cell (atomicAdd with return value; afterwards a
//             cell's word is its END, the start of the next cell) and stores {x, y, z, bits(index inside the pair)} there.  The table
//             is complete since the claim launch ended: the winners are counted here into u.
//   resolve   recip_resolve_kernel: a candidate whose key is its slot's value is a winner.  It walks the rows of cells that meet
//             the clamped bounding box of its ball (radius sqrt(d2) plus the rounding slack below) around q_j -- a row of cells is
//             one contiguous range of `sorted` -- compares rkey(k, j) < key(i) and leaves at the first hit; a box of many cells
//             looks into q_j's own cell first.  A row of more than RECIP_LANE_MAX sources is left out of the lane's walk: after it
//             the wave takes such winners one at a time and scans their long rows in strides of 64 lanes.  ESCAPE: a ball whose box
//             spans more cells than the pair has binned sources has the pair's whole slice of `sorted` scanned that way instead:
//             never more work than brute force.
//             A mutual winner keeps idx / d2 bit for bit, every other candidate gets -1 and the quiet NaN 0x7fc00000, a source that
//             is no candidate passes through; plain vector stores.  r by ballot and popcount, one integer atomic per workgroup;
//             the pair's first workgroup publishes m and u (both complete since earlier launches ended) where a record is given.
// Why the box holds every source that can hit: a hit needs dist2(p_k, q_j) <= d2[i] as floats; a sum of non-negative terms rounds to
// no less than each term, so per axis fl(dx * dx) <= d2 with dx = fl(p - q), hence |p - q| <= sqrt(d2) * (1 + 2^-22) + 2^-74.  The
// box is q -+ (sqrt(d2) * 1.0001 + 2.4e-7 * |q| + 1e-22), which also covers the rounding of q -+ r itself, and the cell of a
// coordinate is a monotone function of it (float subtract, multiply by inv_h > 0, floor, clamp): lo <= p <= hi gives
// cell(lo) <= cell(p) <= cell(hi).
// The grid of the walks and the resolve is o2o_kernel's: the pair's stream_blocks(ns) workgroups of 256 through the row -> pair
// table.  Three properties hold per pair and keep the wave-wide steps sound:
//   - a workgroup belongs to ONE pair, so every ballot, shuffle, barrier and wave-wide hand-over stays inside a pair;
//   - the workgroups of a pair that is no longer active leave at once, before any barrier, ballot or shuffle, and write nothing;
//   - every loop bound that feeds a ballot (i0, the pair's ns and nrows, `todo`, the shuffled box) is the same in every lane.
// No inline assembly, no float atomics, LDS for the wave counters only.
#include <cmath>

#include "kss_device.hpp"
#include "kss_o2o_device.hpp"
#include "kss_pair_device.hpp"

namespace kss {

constexpr int RECIP_THREADS = O2O_THREADS;
constexpr int RECIP_SCAN_THREADS = 1024;

// cell_coord's rule (kss_device.hpp), clamped BEFORE the conversion: an infinite or NaN product lands in a border cell or cell 0
__device__ __forceinline__ int recip_coord(float v, float o, float inv_h, int g) {
    const float f = floorf((v - o) * inv_h);
    return (int)fminf(fmaxf(f, 0.0f), (float)(g - 1));
}
__device__ __forceinline__ int recip_cell(const RecipGrid& g, float x, float y, float z) {
    return (recip_coord(z, g.oz, g.inv_h, g.gz) * g.gy + recip_coord(y, g.oy, g.inv_h, g.gy)) * g.gx + recip_coord(x, g.ox, g.inv_h, g.gx);
}
// the current position of ORIGINAL source i
template <int SRC>
__device__ __forceinline__ void recip_pos(const PairSrc& s, int64_t i, float& x, float& y, float& z) {
    if constexpr (SRC == SRC_F3) {
        x = s.src3[3 * i]; y = s.src3[3 * i + 1]; z = s.src3[3 * i + 2];
    } else {
        const float4 p = s.src4[SRC == SRC_F4_PERM ? (int64_t)s.perm[i] : i];
        x = p.x; y = p.y; z = p.z;
    }
}
__device__ __forceinline__ bool recip_finite(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// one pair as its workgroups see it; LONE (row_pair null): the one pair a.lone_desc / a.lone_grid; state null: every pair is active
struct RecipPair {
    PairbDesc d;
    RecipGrid g;
    unsigned long long* table; unsigned* counters; unsigned* cells;
    float4* sorted;
};
__device__ __forceinline__ unsigned* recip_cells_of(const RecipArgs& a, const RecipPairDev& gp) {
    return recip_counters(a.work, a.total_tgt) + 4 * (int64_t)a.npairs + gp.cell_base;
}
template <bool LONE>
__device__ __forceinline__ int recip_pair_of_row(const RecipArgs& a) {
    if constexpr (LONE) return 0;
    else return a.row_pair[blockIdx.x];
}
// (the lone pair's bases are 0 by definition: said as constants, so that its instances carry none of them)
template <bool LONE>
__device__ __forceinline__ RecipPairDev recip_grid(const RecipArgs& a, int p) {
    if constexpr (LONE) return RecipPairDev{a.lone_grid.g, 0};
    else return a.grids[p];
}
template <bool LONE>
__device__ __forceinline__ RecipPair recip_pair(const RecipArgs& a, int p) {
    const RecipPairDev gp = recip_grid<LONE>(a, p);
    RecipPair w;
    if constexpr (LONE) {
        w.d = a.lone_desc;
        w.d.src_base = 0; w.d.tgt_off = 0; w.d.row_base = 0;
    } else {
        w.d = a.desc[p];
    }
    w.g = gp.g;
    w.table = (unsigned long long*)a.work + w.d.tgt_off;
    w.counters = recip_counters(a.work, a.total_tgt) + 4 * (int64_t)p;
    w.cells = recip_cells_of(a, gp);
    w.sorted = a.sorted + w.d.src_base;
    return w;
}
__device__ __forceinline__ bool recip_active(const RecipArgs& a, int p) { return !a.state || a.state[p].active != 0; }

// One slot of cells[cell] for every lane with `on` set; called by whole waves.  Where all those lanes share ONE cell (every source
// at one point: the worst contention an integer add can meet) one atomic takes the wave's slots and the lanes number themselves by
// prefix popcount; otherwise one atomic per lane, spread over the cells.  A caller that drops the result gets adds without return.
__device__ __forceinline__ unsigned recip_take(unsigned* __restrict__ cells, int cell, bool on) {
    const unsigned long long mask = __ballot(on);
    if (mask == 0ull) return 0u;
    const int lane = threadIdx.x & 63, lead = __ffsll((long long)mask) - 1;
    const int c0 = __shfl(cell, lead, 64);
    if (__ballot(on && cell != c0) == 0ull) {
        unsigned base = 0u;
        if (lane == lead) base = atomicAdd(&cells[c0], (unsigned)__popcll(mask));
        return __shfl(base, lead, 64) + (unsigned)__popcll(mask & ((1ull << lane) - 1ull));
    }
    return on ? atomicAdd(&cells[cell], 1u) : 0u;
}

// SCATTER false: claim + count; true: scatter + the winners' count.  i: the source's index inside its pair (keys, sorted's .w);
// src_base + i: where its idx, d2 and position are
template <int SRC, bool SCATTER, bool LONE>
__global__ __launch_bounds__(RECIP_THREADS) void recip_walk_kernel(const RecipArgs a) {
    __shared__ unsigned wave_cnt[RECIP_THREADS / 64];
    const int p = recip_pair_of_row<LONE>(a);
    if (!recip_active(a, p)) return;
    const RecipPair w = recip_pair<LONE>(a, p);
    const int64_t ns = w.d.ns, base = w.d.src_base;
    const int64_t step = (int64_t)w.d.nrows * RECIP_THREADS;
    unsigned cnt = 0u;
    for (int64_t i0 = (int64_t)((int)blockIdx.x - w.d.row_base) * RECIP_THREADS; i0 < ns; i0 += step) {   // (i0 is the same in every lane)
        const int64_t i = i0 + threadIdx.x;
        const bool live = i < ns;
        const int32_t j = live ? a.s.idx[base + i] : -1;
        const float v = live ? a.s.d2[base + i] : __uint_as_float(0x7fc00000u);
        // (a lane past the end holds j = -1, which is no candidate: tested without a branch on `live`, so that the one wait for
        // idx / d2 stands in front of everything and the claim's two atomics issue back to back)
        const bool cand = o2o_candidate(j, v, w.d.nt, a.s.max_d2);
        float x = 0.0f, y = 0.0f, z = 0.0f;
        if (live) recip_pos<SRC>(a.s, base + i, x, y, z);
        const bool binned = live && recip_finite(x, y, z);
        const int cell = binned ? recip_cell(w.g, x, y, z) : 0;
        if constexpr (!SCATTER) {
            if (cand) atomicMin(&w.table[j], o2o_key(v, i));
            recip_take(w.cells, cell, binned);
            cnt += (unsigned)__popcll(__ballot(cand));
        } else {
            const unsigned slot = recip_take(w.cells, cell, binned);
            if (binned && (int64_t)slot < ns) w.sorted[slot] = make_float4(x, y, z, __uint_as_float((unsigned)i));
            const bool win = cand && w.table[j] == o2o_key(v, i);
            cnt += (unsigned)__popcll(__ballot(win));
        }
    }
    o2o_count(cnt, wave_cnt, w.counters + (SCATTER ? 1 : 0));
}

// exclusive scan of (cells[k] + 1) in place, ONE workgroup per pair over the pair's own cells: every wave owns a run of consecutive
// cells (a multiple of 64) and walks it in tiles of 64, consecutive lanes on consecutive cells; first the runs' totals, the sixteen
// of them through LDS, then the tiles again with the carry
template <bool LONE>
__global__ __launch_bounds__(RECIP_SCAN_THREADS) void recip_scan_kernel(const RecipArgs a) {
    constexpr int NW = RECIP_SCAN_THREADS / 64;
    __shared__ unsigned wave_tot[NW];
    const int p = blockIdx.x;
    if (!recip_active(a, p)) return;
    const RecipPairDev gp = recip_grid<LONE>(a, p);
    unsigned* __restrict__ cells = recip_cells_of(a, gp);
    const int ncells = (int)recip_cells(gp.g);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int run = (ncells + NW * 64 - 1) / (NW * 64) * 64;
    const int b = min(wave * run, ncells), e = min(b + run, ncells);
    unsigned s = 0u;
#pragma unroll 4
    for (int k = b + lane; k < e; k += 64) s += cells[k] + 1u;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) wave_tot[wave] = s;
    __syncthreads();
    unsigned carry = 0u;
    for (int q = 0; q < wave; ++q) carry += wave_tot[q];
    unsigned next = b + lane < e ? cells[b + lane] + 1u : 0u;
    for (int k0 = b; k0 < e; k0 += 64) {
        const int k = k0 + lane;
        const unsigned c = next;
        next = k + 64 < e ? cells[k + 64] + 1u : 0u;   // (the next tile's load is in flight while this one is scanned)
        unsigned incl = c;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned up = __shfl_up(incl, off, 64);
            if (lane >= off) incl += up;
        }
        if (k < e) cells[k] = carry + incl - c;
        carry += __shfl(incl, 63, 64);
    }
}

// rkey(k, j) < key for the source in slot p
template <bool FMA>
__device__ __forceinline__ bool recip_below(const float4 p, float qx, float qy, float qz, unsigned long long key) {
    const float d = dist2<FMA>(p.x, p.y, p.z, qx, qy, qz);
    return (((unsigned long long)(__float_as_uint(d) & 0x7fffffffu) << 32) | (unsigned long long)__float_as_uint(p.w)) < key;
}

// some source in sorted[lo, hi) has rkey(k, j) < key: eight loads in flight per step (a slot past the end is read as the last one
// again: examining a source twice changes nothing)
template <bool FMA>
__device__ __forceinline__ bool recip_hit(const float4* __restrict__ sorted, unsigned lo, unsigned hi, float qx, float qy, float qz,
                                          unsigned long long key) {
    for (unsigned s = lo; s < hi; s += 8u) {
        const unsigned last = hi - 1u;
        float4 p[8];
#pragma unroll
        for (unsigned q = 0u; q < 8u; ++q) p[q] = sorted[min(s + q, last)];
        bool below = false;
#pragma unroll
        for (unsigned q = 0u; q < 8u; ++q) below = recip_below<FMA>(p[q], qx, qy, qz, key) || below;
        if (below) return true;
    }
    return false;
}

// the same by a whole wave (every argument the same in every lane): strides of 64 lanes, four loads in flight per lane, leaving at
// the first stride with a hit
template <bool FMA>
__device__ __forceinline__ bool recip_hit_wave(const float4* __restrict__ sorted, unsigned lo, unsigned hi, float qx, float qy, float qz,
                                               unsigned long long key, int lane) {
    bool found = false;
    for (unsigned base = lo; base < hi && !found; base += 256u) {
        bool below = false;
#pragma unroll
        for (unsigned q = 0u; q < 4u; ++q) {
            const unsigned s = base + 64u * q + (unsigned)lane;
            if (s < hi) below |= recip_below<FMA>(sorted[s], qx, qy, qz, key);
        }
        found = __ballot(below) != 0ull;
    }
    return found;
}

constexpr int RECIP_CENTRE_FIRST = 8;    // a box of more cells than this looks into q_j's own cell first: a hit is most likely there
constexpr unsigned RECIP_LANE_MAX = 128u;   // a row of more sources than this is left to the whole wave

template <bool FMA, bool LONE>
__global__ __launch_bounds__(RECIP_THREADS) void recip_resolve_kernel(const RecipArgs a) {
    __shared__ unsigned wave_cnt[RECIP_THREADS / 64];
    const int p = recip_pair_of_row<LONE>(a);
    if (!recip_active(a, p)) return;
    const RecipPair w = recip_pair<LONE>(a, p);
    const RecipGrid g = w.g;
    const float* __restrict__ tgt = a.tgt + 3 * w.d.tgt_off;
    const int64_t ns = w.d.ns, base = w.d.src_base;
    const int64_t ncells = recip_cells(g);
    const int64_t step = (int64_t)w.d.nrows * RECIP_THREADS;
    const int lane = threadIdx.x & 63;
    unsigned total = w.cells[ncells - 1];   // the pair's last cell's end: every binned source of the pair
    if ((int64_t)total > ns) total = (unsigned)ns;
    unsigned cnt = 0u;
    for (int64_t i0 = (int64_t)((int)blockIdx.x - w.d.row_base) * RECIP_THREADS; i0 < ns; i0 += step) {   // (i0 is the same in every lane)
        const int64_t i = i0 + threadIdx.x;
        const bool live = i < ns;
        const int32_t j = live ? a.s.idx[base + i] : -1;
        const float v = live ? a.s.d2[base + i] : __uint_as_float(0x7fc00000u);
        const bool cand = live && o2o_candidate(j, v, w.d.nt, a.s.max_d2);
        const unsigned long long key = o2o_key(v, i);
        const bool win = cand && w.table[j] == key;
        float qx = 0.0f, qy = 0.0f, qz = 0.0f;
        int x0 = 0, x1 = 0, y0 = 0, y1 = 0, z0 = 0, z1 = -1;   // (an empty box)
        bool hit = false, heavy = false;   // heavy: some row of the box, or the escape, is left to the wave
        if (win) {
            qx = tgt[3 * (int64_t)j]; qy = tgt[3 * (int64_t)j + 1]; qz = tgt[3 * (int64_t)j + 2];
            const float r = sqrtf(fabsf(v)) * 1.0001f + 1e-22f;
            const float rx = r + 2.4e-7f * fabsf(qx), ry = r + 2.4e-7f * fabsf(qy), rz = r + 2.4e-7f * fabsf(qz);
            x0 = recip_coord(qx - rx, g.ox, g.inv_h, g.gx); x1 = recip_coord(qx + rx, g.ox, g.inv_h, g.gx);
            y0 = recip_coord(qy - ry, g.oy, g.inv_h, g.gy); y1 = recip_coord(qy + ry, g.oy, g.inv_h, g.gy);
            z0 = recip_coord(qz - rz, g.oz, g.inv_h, g.gz); z1 = recip_coord(qz + rz, g.oz, g.inv_h, g.gz);
            const int64_t span = (int64_t)(x1 - x0 + 1) * (y1 - y0 + 1) * (z1 - z0 + 1);
            if (x1 < x0 || y1 < y0 || z1 < z0 || span > (int64_t)total) {
                heavy = true;   // the escape (a NaN target: its box is no box): the pair's whole slice, marked by x0 < 0
                x0 = -1;
            } else {
                if (span > RECIP_CENTRE_FIRST) {
                    const int64_t c = recip_cell(g, qx, qy, qz);
                    const unsigned lo = c > 0 ? w.cells[c - 1] : 0u, hi = min(w.cells[c], total);
                    if (hi <= lo + RECIP_LANE_MAX) hit = recip_hit<FMA>(w.sorted, lo, hi, qx, qy, qz, key);
                }
                for (int cz = z0; cz <= z1 && !hit; ++cz)
                    for (int cy = y0; cy <= y1 && !hit; ++cy) {
                        const int64_t c0 = ((int64_t)cz * g.gy + cy) * g.gx + x0;
                        const unsigned lo = c0 > 0 ? w.cells[c0 - 1] : 0u, hi = min(w.cells[c0 + (x1 - x0)], total);
                        if (hi > lo && hi - lo > RECIP_LANE_MAX) heavy = true;
                        else hit = recip_hit<FMA>(w.sorted, lo, hi, qx, qy, qz, key);
                    }
            }
        }
        // the rows left over, one winner at a time by the whole wave
        for (unsigned long long todo = __ballot(heavy && !hit); todo != 0ull; todo &= todo - 1ull) {
            const int l = __ffsll((long long)todo) - 1;
            const float ex = __shfl(qx, l, 64), ey = __shfl(qy, l, 64), ez = __shfl(qz, l, 64);
            const unsigned long long ek = ((unsigned long long)__shfl((unsigned)(key >> 32), l, 64) << 32) | (unsigned long long)__shfl((unsigned)key, l, 64);
            const int bx0 = __shfl(x0, l, 64), bx1 = __shfl(x1, l, 64), by0 = __shfl(y0, l, 64), by1 = __shfl(y1, l, 64);
            const int bz0 = __shfl(z0, l, 64), bz1 = __shfl(z1, l, 64);
            bool found = false;
            if (bx0 < 0) {
                found = recip_hit_wave<FMA>(w.sorted, 0u, total, ex, ey, ez, ek, lane);
            } else {
                for (int cz = bz0; cz <= bz1 && !found; ++cz)
                    for (int cy = by0; cy <= by1 && !found; ++cy) {
                        const int64_t c0 = ((int64_t)cz * g.gy + cy) * g.gx + bx0;
                        const unsigned lo = c0 > 0 ? w.cells[c0 - 1] : 0u, hi = min(w.cells[c0 + (bx1 - bx0)], total);
                        if (hi > lo && hi - lo > RECIP_LANE_MAX) found = recip_hit_wave<FMA>(w.sorted, lo, hi, ex, ey, ez, ek, lane);
                    }
            }
            if (lane == l) hit = found;
        }
        const bool mutual = win && !hit;
        if (live) {
            if (a.idx_out) a.idx_out[base + i] = cand && !mutual ? -1 : j;
            if (a.d2_out) a.d2_out[base + i] = cand && !mutual ? __uint_as_float(0x7fc00000u) : v;
        }
        cnt += (unsigned)__popcll(__ballot(mutual));
    }
    o2o_count(cnt, wave_cnt, w.counters + 2);
    if (a.info_mu && (int)blockIdx.x == w.d.row_base && threadIdx.x == 0) {   // the pair's first workgroup: m and u are complete since earlier launches ended
        a.info_mu[2 * (int64_t)p] = (double)(w.counters[0] + 1u);
        a.info_mu[2 * (int64_t)p + 1] = (double)(w.counters[1] + 1u);
    }
}

// ---- the targets' bounding boxes, once per call ----
// every pair's target box in one launch: workgroup b takes partial b % split of pair b / split -- the pair's targets
// (b % split) * 256 + t + k * 256 * split -- and writes {min xyz, max xyz}; a partial without a target stays {+inf, -inf}.
// desc null: the one pair `lone`
__global__ __launch_bounds__(RECIP_THREADS) void recip_bbox_kernel(const float* __restrict__ tgt_all, const PairbDesc* __restrict__ desc,
                                                                    const PairbDesc lone, int split, float* __restrict__ box) {
    __shared__ float sh[RECIP_THREADS / 64][6];
    const PairbDesc d = desc ? desc[blockIdx.x / split] : lone;
    const float* __restrict__ tgt = tgt_all + 3 * d.tgt_off;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t j = (int64_t)(blockIdx.x % split) * RECIP_THREADS + threadIdx.x; j < d.nt; j += (int64_t)split * RECIP_THREADS)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float v = tgt[3 * j + k];
            mn[k] = fminf(mn[k], v); mx[k] = fmaxf(mx[k], v);
        }
#pragma unroll
    for (int k = 0; k < 3; ++k)
        for (int off = 32; off > 0; off >>= 1) {
            mn[k] = fminf(mn[k], __shfl_down(mn[k], off, 64));
            mx[k] = fmaxf(mx[k], __shfl_down(mx[k], off, 64));
        }
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < 3; ++k) { sh[threadIdx.x >> 6][k] = mn[k]; sh[threadIdx.x >> 6][3 + k] = mx[k]; }
    __syncthreads();
    if (threadIdx.x < 6) {
        float v = sh[0][threadIdx.x];
        for (int q = 1; q < RECIP_THREADS / 64; ++q) v = threadIdx.x < 3 ? fminf(v, sh[q][threadIdx.x]) : fmaxf(v, sh[q][threadIdx.x]);
        box[6 * (int64_t)blockIdx.x + threadIdx.x] = v;
    }
}

void launch_recip_bbox(hipStream_t st, const float* d_tgt, const PairbDesc* d_desc, const PairbDesc& lone, int npairs, int split, float* d_box) {
    hipLaunchKernelGGL(recip_bbox_kernel, dim3((unsigned)npairs * (unsigned)split), dim3(RECIP_THREADS), 0, st, d_tgt, d_desc, lone, split, d_box);
}

size_t recip_work_bytes(int64_t total_tgt, int npairs, int64_t total_cells) {
    return (size_t)total_tgt * sizeof(unsigned long long) + ((size_t)npairs * 4 + (size_t)total_cells) * sizeof(unsigned);
}

template <int SRC, bool LONE>
static void launch_recip_walks(hipStream_t st, const RecipArgs& a, int total_rows) {
    hipLaunchKernelGGL((recip_walk_kernel<SRC, false, LONE>), dim3(total_rows), dim3(RECIP_THREADS), 0, st, a);
    hipLaunchKernelGGL(recip_scan_kernel<LONE>, dim3(a.npairs), dim3(RECIP_SCAN_THREADS), 0, st, a);
    hipLaunchKernelGGL((recip_walk_kernel<SRC, true, LONE>), dim3(total_rows), dim3(RECIP_THREADS), 0, st, a);
}
template <bool LONE>
static void launch_recip_steps(hipStream_t st, int total_rows, const RecipArgs& a, bool nn_fma) {
    if (a.s.src3) launch_recip_walks<SRC_F3, LONE>(st, a, total_rows);
    else if (a.s.perm) launch_recip_walks<SRC_F4_PERM, LONE>(st, a, total_rows);
    else launch_recip_walks<SRC_F4, LONE>(st, a, total_rows);
    if (nn_fma) hipLaunchKernelGGL((recip_resolve_kernel<true, LONE>), dim3(total_rows), dim3(RECIP_THREADS), 0, st, a);
    else hipLaunchKernelGGL((recip_resolve_kernel<false, LONE>), dim3(total_rows), dim3(RECIP_THREADS), 0, st, a);
}

int launch_recip(hipStream_t st, int total_rows, int64_t total_cells, const RecipArgs& a, bool nn_fma) {
    const hipError_t e = hipMemsetAsync(a.work, 0xff, recip_work_bytes(a.total_tgt, a.npairs, total_cells), st);
    if (e != hipSuccess) return (int)e;
    if (a.row_pair) launch_recip_steps<false>(st, total_rows, a, nn_fma);
    else launch_recip_steps<true>(st, total_rows, a, nn_fma);
    return 0;
}

}  // namespace kss