// kss_vmap.hip -- the voxel map of voxelized generalized ICP: one Gaussian per occupied voxel of a
// box, kept for as many registrations as the caller likes.  The definitions are restated at kss_vmap, kss_vmap_insert and
// kss_vmap_shift in include/kssicp.h; the record of a voxel is a SERIAL f64 sum over its points in ascending index of each call,
// in the order of the calls, so every bit of it is determined by the clouds alone.
// ONE pipeline puts points into a map (vmap_insert_into); the box, origin, inv and dims never change, the voxels are renumbered
// (a new occupied cell may lie between two old ones) and every touched voxel's sums are continued from acc:
//   flags                 flag[c] = occupied before: a memset for a map without a voxel, else one pass over the table;
//   cell                  every new point moved and turned, its lin, its arrival slot in the cell (an integer atomic on a zeroed
//                         count table in the scratch; the order of arrival is undone below), the cell's flag (hit now) and the two
//                         tallies of points left out;
//   scan                  the exclusive scan of the flags numbers the occupied cells in ascending lin; the voxel count and the
//                         tallies go to the host, which makes room for the new records.  Up to here the map has only been read: a
//                         call with nothing to add, a refused one and a failed allocation leave it as it was;
//   compact               the cell table IN PLACE, at the occupied cells alone (an empty cell stays -1, and a cell is occupied iff
//                         the scan steps over it, so the scan is the only table read in full): the new lin, the per-voxel NEW-point
//                         counts and every voxel's old number (-1: created now), the gather index of the old N and sums;
//   scan, scatter         the exclusive scan of the packed counts gives every voxel its slots; a point goes to start + arrival slot;
//   rank fix              every point ranks itself among its voxel's new points by index (grid_rank_fix_kernel's pattern): the
//                         slots of a voxel now hold them in ascending index whatever the atomics did;
//   continue              one lane per voxel: from the old sums (zero for a created voxel) on through its new points, serially in
//                         f64, then the six + three divisions; a voxel without a new point is copied.
// The new rec, acc and lin are built in the records that are not in use (VmapBuilt::spare) and change places with the old ones on
// the host after the last synchronisation.  The three entry points:
//   vmap_build            the float box of the mapped targets and their count (2 launches: fminf / fmaxf partials per workgroup,
//                         then one workgroup; dims follow on the host: f is monotone in x, so the largest f_a is f_a of the largest
//                         x_a), an empty table over it, the pipeline with no pose and records of exactly the voxel count;
//   vmap_empty            the empty table alone (kss_vmap_create_box);
//   vmap_insert           the pipeline on a live map, records with half as much headroom again.
// vmap_shift (below) moves the window and shares the records' reserve and swap; vmap_coarsen (at the end) fills a map from the
// kept sums of another.
// A voxel of N new points costs N^2 index compares in the rank fix (spread over its N lanes) and N dependent f64 additions on one
// lane in the walk: nothing at a few points per voxel, and seconds to minutes for a million-point cloud inside ONE voxel (a leaf
// far larger than the cloud) -- which is not a map anyone registers against.
// No float atomic, nothing fused (fp contraction is off), no workspace of the context: the scratch is allocated here and freed
// before a call returns, and what the map keeps (table, records, lin, sums; a coarse map also the work area of its fill) is its own.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>

#include "kss_internal.hpp"

namespace kss {

constexpr int VMAP_THREADS = 256;

struct VmapPose {
    VmapMove mv;
    int on = 0;   // 0: the points and normals as they are
};

// the point as the map takes it (transform_apply_f32_kernel's expression); true: mapped, all six of position and normal finite
__device__ __forceinline__ bool vmap_moved(const float* __restrict__ pts, const float* __restrict__ nrm, int64_t i, const VmapPose& T, float& x, float& y, float& z) {
    x = pts[3 * i]; y = pts[3 * i + 1]; z = pts[3 * i + 2];
    if (T.on) {
        const float* m = T.mv.m;
        const float a = x, b = y, c = z;
        x = ((m[0] * a + m[1] * b) + m[2] * c) + m[3];
        y = ((m[4] * a + m[5] * b) + m[6] * c) + m[7];
        z = ((m[8] * a + m[9] * b) + m[10] * c) + m[11];
    }
    return isfinite(x) && isfinite(y) && isfinite(z) && isfinite(nrm[3 * i]) && isfinite(nrm[3 * i + 1]) && isfinite(nrm[3 * i + 2]);
}

// lo / hi / count of the lanes of a workgroup (valid in lane 0): wave shuffles, the four wave results through LDS
__device__ __forceinline__ void vmap_box_reduce(float (&lo)[3], float (&hi)[3], unsigned long long& cnt) {
    __shared__ float sh[VMAP_THREADS / 64][6];
    __shared__ unsigned long long shc[VMAP_THREADS / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = fminf(lo[a], __shfl_down(lo[a], off, 64));
            hi[a] = fmaxf(hi[a], __shfl_down(hi[a], off, 64));
        }
        cnt += __shfl_down(cnt, off, 64);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { sh[wave][a] = lo[a]; sh[wave][3 + a] = hi[a]; }
        shc[wave] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < VMAP_THREADS / 64; ++w) {
#pragma unroll
            for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], sh[w][a]); hi[a] = fmaxf(hi[a], sh[w][3 + a]); }
            cnt += shc[w];
        }
    }
}

__global__ __launch_bounds__(VMAP_THREADS) void vmap_bounds_kernel(const float* __restrict__ tgt, const float* __restrict__ nrm, int64_t nt,
                                                                    float* __restrict__ part, unsigned long long* __restrict__ part_cnt) {
    const float inf = __builtin_inff();
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    unsigned long long cnt = 0;
    for (int64_t i = (int64_t)blockIdx.x * VMAP_THREADS + threadIdx.x; i < nt; i += (int64_t)gridDim.x * VMAP_THREADS) {
        float p[3];
        if (!vmap_moved(tgt, nrm, i, VmapPose(), p[0], p[1], p[2])) continue;
#pragma unroll
        for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], p[a]); hi[a] = fmaxf(hi[a], p[a]); }
        ++cnt;
    }
    vmap_box_reduce(lo, hi, cnt);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { part[6 * blockIdx.x + a] = lo[a]; part[6 * blockIdx.x + 3 + a] = hi[a]; }
        part_cnt[blockIdx.x] = cnt;
    }
}

// one workgroup: the partials' box and count into out[0..5] and *out_cnt
__global__ __launch_bounds__(VMAP_THREADS) void vmap_bounds_final_kernel(const float* __restrict__ part, const unsigned long long* __restrict__ part_cnt,
                                                                          int nb, float* __restrict__ out, unsigned long long* __restrict__ out_cnt) {
    const float inf = __builtin_inff();
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    unsigned long long cnt = 0;
    for (int b = threadIdx.x; b < nb; b += VMAP_THREADS) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], part[6 * b + a]); hi[a] = fmaxf(hi[a], part[6 * b + 3 + a]); }
        cnt += part_cnt[b];
    }
    vmap_box_reduce(lo, hi, cnt);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { out[a] = lo[a]; out[3 + a] = hi[a]; }
        *out_cnt = cnt;
    }
}

struct VmapGrid {
    float lo[3]; float inv;
    int dims[3];
    int base[3];   // the window's first cell per axis (0 until a shift): VmapDev's
};

__global__ __launch_bounds__(VMAP_THREADS) void vmap_insert_cell_kernel(const float* __restrict__ pts, const float* __restrict__ nrm, int64_t n,
                                                                         const VmapPose T, const VmapGrid g, int32_t* __restrict__ lin32,
                                                                         int32_t* __restrict__ slot, int32_t* __restrict__ cnt,
                                                                         int32_t* __restrict__ flag, unsigned long long* __restrict__ tally) {
    unsigned long long unmapped = 0, outside = 0;
    for (int64_t i = (int64_t)blockIdx.x * VMAP_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * VMAP_THREADS) {
        float x, y, z;
        if (!vmap_moved(pts, nrm, i, T, x, y, z)) { lin32[i] = -1; ++unmapped; continue; }
        // the lookup's rule (vgicp_source): compared in float, against the window base .. base + dims
        const float fx = floorf((x - g.lo[0]) * g.inv), fy = floorf((y - g.lo[1]) * g.inv), fz = floorf((z - g.lo[2]) * g.inv);
        if (!(fx >= (float)g.base[0] && fx < (float)(g.base[0] + g.dims[0]) && fy >= (float)g.base[1] && fy < (float)(g.base[1] + g.dims[1]) &&
              fz >= (float)g.base[2] && fz < (float)(g.base[2] + g.dims[2]))) {
            lin32[i] = -1; ++outside; continue;
        }
        const int cx = (int)fx - g.base[0], cy = (int)fy - g.base[1], cz = (int)fz - g.base[2];   // (|f| <= 2^24 inside the window)
        const int32_t lin = (int32_t)(((int64_t)cz * g.dims[1] + cy) * g.dims[0] + cx);   // (inside the table: the test above)
        lin32[i] = lin;
        slot[i] = atomicAdd(&cnt[lin], 1);
        flag[lin] = 1;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        unmapped += __shfl_down(unmapped, off, 64);
        outside += __shfl_down(outside, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (unmapped) atomicAdd(&tally[0], unmapped);
        if (outside) atomicAdd(&tally[1], outside);
    }
}

__global__ __launch_bounds__(VMAP_THREADS) void vmap_insert_flags_kernel(const int32_t* __restrict__ old_cell, int64_t ncells,
                                                                          int32_t* __restrict__ flag) {
    for (int64_t c = (int64_t)blockIdx.x * VMAP_THREADS + threadIdx.x; c < ncells; c += (int64_t)gridDim.x * VMAP_THREADS)
        flag[c] = old_cell[c] >= 0 ? 1 : 0;
}

// the map's cell table renumbered in place.  vox: the exclusive scan of the flags, ncells + 1 entries
__global__ __launch_bounds__(VMAP_THREADS) void vmap_insert_compact_kernel(int32_t* __restrict__ cell, const int32_t* __restrict__ cnt,
                                                                            const int32_t* __restrict__ vox, int64_t ncells,
                                                                            int64_t* __restrict__ lin, int32_t* __restrict__ vcnt,
                                                                            int32_t* __restrict__ vold) {
    for (int64_t c = (int64_t)blockIdx.x * VMAP_THREADS + threadIdx.x; c < ncells; c += (int64_t)gridDim.x * VMAP_THREADS) {
        const int32_t v = vox[c];
        if (vox[c + 1] == v) continue;
        lin[v] = c;
        vcnt[v] = cnt[c];   // (0: an old voxel no new point fell into)
        vold[v] = cell[c];
        cell[c] = v;
    }
}

__global__ __launch_bounds__(VMAP_THREADS) void vmap_scatter_kernel(const int32_t* __restrict__ lin32, const int32_t* __restrict__ slot, int64_t nt,
                                                                     const int32_t* __restrict__ cell, const int32_t* __restrict__ vstart,
                                                                     int32_t* __restrict__ tmp) {
    for (int64_t i = (int64_t)blockIdx.x * VMAP_THREADS + threadIdx.x; i < nt; i += (int64_t)gridDim.x * VMAP_THREADS) {
        const int32_t lin = lin32[i];
        if (lin >= 0) tmp[vstart[cell[lin]] + slot[i]] = (int32_t)i;
    }
}

// slot j of tmp: its target's rank by original index among the targets of its voxel
__global__ __launch_bounds__(VMAP_THREADS) void vmap_rank_fix_kernel(const int32_t* __restrict__ tmp, int64_t mapped, const int32_t* __restrict__ lin32,
                                                                      const int32_t* __restrict__ cell, const int32_t* __restrict__ vstart,
                                                                      int32_t* __restrict__ order) {
    for (int64_t j = (int64_t)blockIdx.x * VMAP_THREADS + threadIdx.x; j < mapped; j += (int64_t)gridDim.x * VMAP_THREADS) {
        const int32_t me = tmp[j];
        const int32_t v = cell[lin32[me]];
        const int32_t lo = vstart[v], hi = vstart[v + 1];
        int32_t rank = 0;
        for (int32_t k = lo; k < hi; ++k) rank += tmp[k] < me ? 1 : 0;
        order[lo + rank] = me;
    }
}

// one lane per voxel of the new numbering: the old sums continued through the voxel's new points in ascending index
__global__ __launch_bounds__(VMAP_THREADS) void vmap_continue_kernel(const float* __restrict__ pts, const float* __restrict__ nrm, const VmapPose T,
                                                                      const int32_t* __restrict__ order, const int32_t* __restrict__ vstart,
                                                                      const int32_t* __restrict__ vold, const double* __restrict__ old_rec,
                                                                      const double* __restrict__ old_acc, int64_t nvox, double* __restrict__ rec,
                                                                      double* __restrict__ acc) {
    for (int64_t v = (int64_t)blockIdx.x * VMAP_THREADS + threadIdx.x; v < nvox; v += (int64_t)gridDim.x * VMAP_THREADS) {
        const int32_t lo = vstart[v], hi = vstart[v + 1];
        const int64_t ov = vold[v];
        double* r = rec + v * VMAP_NSTAT;
        double* q = acc + v * VMAP_NACC;
        if (lo == hi) {   // (an old voxel: a created one has a new point)
#pragma unroll
            for (int a = 0; a < VMAP_NSTAT; ++a) r[a] = old_rec[ov * VMAP_NSTAT + a];
#pragma unroll
            for (int a = 0; a < VMAP_NACC; ++a) q[a] = old_acc[ov * VMAP_NACC + a];
            continue;
        }
        double N = 0.0, s[3] = {0.0, 0.0, 0.0}, P[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (ov >= 0) {
            N = old_rec[ov * VMAP_NSTAT];
#pragma unroll
            for (int a = 0; a < 3; ++a) s[a] = old_acc[ov * VMAP_NACC + a];
#pragma unroll
            for (int a = 0; a < 6; ++a) P[a] = old_acc[ov * VMAP_NACC + 3 + a];
        }
        for (int32_t k = lo; k < hi; ++k) {
            const int64_t i = order[k];
            float x, y, z;
            (void)vmap_moved(pts, nrm, i, T, x, y, z);
            double n0 = (double)nrm[3 * i], n1 = (double)nrm[3 * i + 1], n2 = (double)nrm[3 * i + 2];
            if (T.on) {   // VgicpMetric's expression for a turned source normal
                const float* m = T.mv.m;
                const double u0 = n0, u1 = n1, u2 = n2;
                n0 = ((double)m[0] * u0 + (double)m[1] * u1) + (double)m[2] * u2;
                n1 = ((double)m[4] * u0 + (double)m[5] * u1) + (double)m[6] * u2;
                n2 = ((double)m[8] * u0 + (double)m[9] * u1) + (double)m[10] * u2;
            }
            s[0] += (double)x; s[1] += (double)y; s[2] += (double)z;
            P[0] += n0 * n0; P[1] += n0 * n1; P[2] += n0 * n2;
            P[3] += n1 * n1; P[4] += n1 * n2;
            P[5] += n2 * n2;
        }
        N += (double)(hi - lo);
        r[0] = N;
#pragma unroll
        for (int a = 0; a < 3; ++a) { r[1 + a] = s[a] / N; q[a] = s[a]; }
#pragma unroll
        for (int a = 0; a < 6; ++a) { r[4 + a] = P[a] / N; q[3 + a] = P[a]; }
    }
}

void vmap_free(VmapBuilt& b) {
    if (b.cell) (void)hipFree(b.cell);
    if (b.rec) (void)hipFree(b.rec);   // (acc and lin are parts of this allocation: vmap_pack_at)
    if (b.spare) (void)hipFree(b.spare);
    if (b.work) (void)hipFree(b.work);
    b.cell = nullptr; b.rec = nullptr; b.lin = nullptr; b.acc = nullptr; b.spare = nullptr; b.work = nullptr;
    b.cap = b.spare_cap = 0;
    b.work_bytes = 0;
}

// a call's scratch: one allocation, carved into 256-byte aligned parts
struct VmapScratch {
    char* base = nullptr;
    size_t used = 0;
    ~VmapScratch() { if (base) (void)hipFree(base); }
    static size_t pad(size_t bytes) { return (bytes + 255) / 256 * 256; }
    template <class T>
    T* take(size_t count) {
        T* p = (T*)(base + used);
        used += pad(count * sizeof(T));
        return p;
    }
};

// rec, acc and lin for up to cap voxels as ONE allocation with rec as its base: an insert replaces all three at once, and a
// release costs more than every kernel of an insert together (0.17 ms: DESIGN.md 2.34)
static size_t vmap_pack_bytes(int64_t cap) {
    return VmapScratch::pad((size_t)cap * VMAP_NSTAT * sizeof(double)) + VmapScratch::pad((size_t)cap * VMAP_NACC * sizeof(double)) + (size_t)cap * sizeof(int64_t);
}
static void vmap_pack_at(VmapBuilt& b, void* base, int64_t cap) {
    b.rec = (double*)base;
    b.acc = (double*)((char*)base + VmapScratch::pad((size_t)cap * VMAP_NSTAT * sizeof(double)));
    b.lin = (int64_t*)((char*)b.acc + VmapScratch::pad((size_t)cap * VMAP_NACC * sizeof(double)));
    b.cap = cap;
}
// b.spare with room for n voxels: kept where it is large enough, else released and allocated again for `fresh` (>= n) voxels --
// the caller's headroom rule.  false: out of memory, b has no spare and is otherwise what it was
static bool vmap_reserve(VmapBuilt& b, int64_t n, int64_t fresh) {
    if (b.spare_cap >= n) return true;
    if (b.spare) (void)hipFree(b.spare);
    b.spare = nullptr; b.spare_cap = 0;
    if (hipMalloc(&b.spare, vmap_pack_bytes(fresh)) != hipSuccess) { b.spare = nullptr; return false; }
    b.spare_cap = fresh;
    return true;
}
// the records just built in b.spare and the ones in use change places (the latter null and 0 for a map that had none)
static void vmap_swap(VmapBuilt& b) {
    void* const old = b.rec;
    const int64_t old_cap = b.cap;
    vmap_pack_at(b, b.spare, b.spare_cap);
    b.spare = old; b.spare_cap = old_cap;
}

static VmapGrid vmap_grid(const VmapBuilt& b) {
    VmapGrid g;
    g.inv = b.inv;
    for (int a = 0; a < 3; ++a) { g.lo[a] = b.lo[a]; g.dims[a] = b.dims[a]; g.base[a] = b.base[a]; }
    return g;
}

// The header of a map over the box lo .. hi and its table of -1, filled on st and NOT waited for.  vmap_empty's return codes;
// 2 and 3 hold nothing
static int vmap_table(hipStream_t st, const float lo[3], const float hi[3], float inv, VmapBuilt& b) {
    int64_t ncells = 1;
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(lo[a]) || !std::isfinite(hi[a]) || hi[a] < lo[a]) return 1;
        b.lo[a] = lo[a] == 0.0f ? 0.0f : lo[a];   // (a zero origin is +0)
        const float f = floorf((hi[a] - b.lo[a]) * inv);
        if (!(f >= 0.0f && f < (float)VMAP_MAX_CELLS)) return 1;   // (a NaN and an infinity included: 0 * inf)
        b.dims[a] = 1 + (int)f;
        ncells *= b.dims[a];
        if (ncells > VMAP_MAX_CELLS) return 1;
    }
    b.inv = inv;
    if (hipMalloc((void**)&b.cell, (size_t)ncells * sizeof(int32_t)) != hipSuccess) return 2;
    if (hipMemsetAsync(b.cell, 0xff, (size_t)ncells * sizeof(int32_t), st) != hipSuccess) {
        vmap_free(b);
        return 3;
    }
    return 0;
}

int vmap_empty(hipStream_t st, const float lo[3], const float hi[3], float inv, VmapBuilt& out) {
    VmapBuilt b;
    const int rc = vmap_table(st, lo, hi, inv, b);
    if (rc != 0) return rc;
    if (hipStreamSynchronize(st) != hipSuccess) {
        vmap_free(b);
        return 3;
    }
    out = b;
    return 0;
}

// The pipeline of the header comment: n points into b at the pose.  headroom: records that have to be allocated get half as much
// room again (a map that is inserted into), else exactly the voxel count (the build).  vmap_insert's return codes and counts
static int vmap_insert_into(hipStream_t st, VmapBuilt& b, const float* d_pts, const float* d_nrm, int64_t n, const VmapPose& pose, bool headroom,
                            int64_t counts[VMAP_NINSERT]) {
    const VmapGrid g = vmap_grid(b);
    const int64_t ncells = (int64_t)b.dims[0] * b.dims[1] * b.dims[2];
    const int64_t vmax = std::min<int64_t>(b.nvox + n, ncells);   // at most this many voxels afterwards
    const int nb = stream_blocks(n);
    // ---- the scratch; the map is only read until the new records are allocated ----
    VmapScratch w;
    const size_t scan_bytes = std::max(scan_scratch_bytes((int)ncells), scan_scratch_bytes((int)vmax));
    const size_t want = 2 * VmapScratch::pad((size_t)ncells * 4) + VmapScratch::pad(((size_t)ncells + 1) * 4) + VmapScratch::pad(scan_bytes) +
                        4 * VmapScratch::pad((size_t)n * 4) + 2 * VmapScratch::pad((size_t)vmax * 4) + VmapScratch::pad(((size_t)vmax + 1) * 4) +
                        VmapScratch::pad(2 * sizeof(unsigned long long));
    if (hipMalloc((void**)&w.base, want) != hipSuccess) return 2;
    int32_t* d_vox = w.take<int32_t>((size_t)ncells + 1);          // (the scan's total and the tallies behind it: read back together)
    unsigned long long* d_tally = w.take<unsigned long long>(2);   // (the tallies, the count table, the flags: zeroed together)
    int32_t* d_cnt = w.take<int32_t>((size_t)ncells);
    int32_t* d_flag = w.take<int32_t>((size_t)ncells);
    int32_t* d_scan = (int32_t*)w.take<char>(scan_bytes);
    int32_t* d_lin32 = w.take<int32_t>((size_t)n);
    int32_t* d_slot = w.take<int32_t>((size_t)n);
    int32_t* d_tmp = w.take<int32_t>((size_t)n);
    int32_t* d_order = w.take<int32_t>((size_t)n);
    int32_t* d_vcnt = w.take<int32_t>((size_t)vmax);
    int32_t* d_vold = w.take<int32_t>((size_t)vmax);
    int32_t* d_vstart = w.take<int32_t>((size_t)vmax + 1);
    // one memset zeroes the tallies and the counts -- and, for a map without a voxel, the flags behind them: no cell was occupied
    // before (the table is all -1), so they need no pass over it
    const bool fresh = b.nvox == 0;
    if (hipMemsetAsync(d_tally, 0, (size_t)((char*)(fresh ? d_flag + ncells : d_cnt + ncells) - (char*)d_tally), st) != hipSuccess) return 3;
    if (!fresh) hipLaunchKernelGGL(vmap_insert_flags_kernel, dim3(stream_blocks(ncells)), dim3(VMAP_THREADS), 0, st, (const int32_t*)b.cell, ncells, d_flag);
    hipLaunchKernelGGL(vmap_insert_cell_kernel, dim3(nb), dim3(VMAP_THREADS), 0, st, d_pts, d_nrm, n, pose, g, d_lin32, d_slot, d_cnt, d_flag, d_tally);
    launch_scan(st, d_flag, (int)ncells, d_vox, d_scan, false);
    // ONE copy brings back the scan's total, vox[ncells], and the tallies with the padding between them (a second copy waits
    // 20 us behind the first: DESIGN.md 2.36)
    alignas(8) unsigned char back[256 + 2 * sizeof(unsigned long long)];
    const size_t back_bytes = (size_t)((char*)(d_tally + 2) - (char*)(d_vox + ncells));   // (4 .. 256 bytes, then the 16 of the tallies)
    if (hipMemcpyAsync(back, d_vox + ncells, back_bytes, hipMemcpyDeviceToHost, st) != hipSuccess) return 3;
    if (hipGetLastError() != hipSuccess) return 3;
    if (hipStreamSynchronize(st) != hipSuccess) return 3;
    int32_t nvox32;
    unsigned long long tally[2];
    memcpy(&nvox32, back, sizeof nvox32);
    memcpy(tally, back + back_bytes - sizeof tally, sizeof tally);
    const int64_t nvox = nvox32;
    const int64_t added = n - (int64_t)tally[0] - (int64_t)tally[1];
    if (added < 0 || nvox < b.nvox || nvox > vmax || (added == 0 && nvox != b.nvox)) return 3;
    counts[0] = added; counts[1] = (int64_t)tally[0]; counts[2] = (int64_t)tally[1]; counts[3] = nvox - b.nvox;
    if (added == 0) return 0;   // nothing to add: the map stays
    // the records that are not in use (the ones the last insert replaced) take the new ones, so a sequence of inserts releases
    // nothing but its scratch.  This is the last allocation, in front of the first store into the map's table
    if (!vmap_reserve(b, nvox, headroom ? std::min<int64_t>(nvox + nvox / 2, ncells) : nvox)) return 2;
    VmapBuilt nw;   // rec, acc and lin that take the place of b's
    vmap_pack_at(nw, b.spare, b.spare_cap);
    // ---- the table in place, the records beside the old ones (a HIP error from here on leaves a map that is not to be used) ----
    hipLaunchKernelGGL(vmap_insert_compact_kernel, dim3(stream_blocks(ncells)), dim3(VMAP_THREADS), 0, st, b.cell, (const int32_t*)d_cnt,
                       (const int32_t*)d_vox, ncells, nw.lin, d_vcnt, d_vold);
    launch_scan(st, d_vcnt, (int)nvox, d_vstart, d_scan, false);
    hipLaunchKernelGGL(vmap_scatter_kernel, dim3(nb), dim3(VMAP_THREADS), 0, st, (const int32_t*)d_lin32, (const int32_t*)d_slot, n,
                       (const int32_t*)b.cell, (const int32_t*)d_vstart, d_tmp);
    hipLaunchKernelGGL(vmap_rank_fix_kernel, dim3(stream_blocks(added)), dim3(VMAP_THREADS), 0, st, (const int32_t*)d_tmp, added,
                       (const int32_t*)d_lin32, (const int32_t*)b.cell, (const int32_t*)d_vstart, d_order);
    hipLaunchKernelGGL(vmap_continue_kernel, dim3(stream_blocks(nvox)), dim3(VMAP_THREADS), 0, st, d_pts, d_nrm, pose, (const int32_t*)d_order,
                       (const int32_t*)d_vstart, (const int32_t*)d_vold, (const double*)b.rec, (const double*)b.acc, nvox, nw.rec, nw.acc);
    if (hipGetLastError() != hipSuccess) return 3;
    if (hipStreamSynchronize(st) != hipSuccess) return 3;   // (the scratch is freed on return)
    vmap_swap(b);
    b.mapped += added; b.nvox = nvox;
    return 0;
}

int vmap_insert(hipStream_t st, VmapBuilt& b, const float* d_pts, const float* d_nrm, int64_t n, const float* T, int64_t counts[VMAP_NINSERT]) {
    VmapPose pose;
    if (T) {
        for (int k = 0; k < 12; ++k) pose.mv.m[k] = T[k];
        pose.on = 1;
    }
    return vmap_insert_into(st, b, d_pts, d_nrm, n, pose, true, counts);
}

int vmap_build(hipStream_t st, const float* d_tgt, const float* d_nrm, int64_t nt, float inv, VmapBuilt& out) {
    const int nb = stream_blocks(nt);
    // ---- the box ----
    VmapScratch box;
    if (hipMalloc((void**)&box.base, VmapScratch::pad((size_t)(nb + 1) * 6 * sizeof(float)) + VmapScratch::pad((size_t)(nb + 1) * 8)) != hipSuccess) return 2;
    float* d_part = box.take<float>((size_t)(nb + 1) * 6);
    unsigned long long* d_pcnt = box.take<unsigned long long>((size_t)nb + 1);
    hipLaunchKernelGGL(vmap_bounds_kernel, dim3(nb), dim3(VMAP_THREADS), 0, st, d_tgt, d_nrm, nt, d_part, d_pcnt);
    hipLaunchKernelGGL(vmap_bounds_final_kernel, dim3(1), dim3(VMAP_THREADS), 0, st, (const float*)d_part, (const unsigned long long*)d_pcnt, nb,
                       d_part + (size_t)nb * 6, d_pcnt + nb);
    float hbox[6];
    unsigned long long hcnt = 0;
    if (hipMemcpyAsync(hbox, d_part + (size_t)nb * 6, sizeof hbox, hipMemcpyDeviceToHost, st) != hipSuccess) return 3;
    if (hipMemcpyAsync(&hcnt, d_pcnt + nb, sizeof hcnt, hipMemcpyDeviceToHost, st) != hipSuccess) return 3;
    if (hipStreamSynchronize(st) != hipSuccess) return 3;
    if (hcnt == 0) return 1;
    // ---- the empty table over it, then the mapped targets inserted as they are.  x >= lo and x <= hi give 0 <= f <= dims - 1
    // (subtraction, multiplication by inv >= 0 and floorf are monotone), so the insert must take exactly the box pass's targets ----
    VmapBuilt b;
    int rc = vmap_table(st, hbox, hbox + 3, inv, b);
    if (rc != 0) return rc;
    int64_t counts[VMAP_NINSERT] = {0, 0, 0, 0};
    rc = vmap_insert_into(st, b, d_tgt, d_nrm, nt, VmapPose(), false, counts);
    if (rc == 0 && (counts[0] != (int64_t)hcnt || counts[1] != nt - (int64_t)hcnt || counts[2] != 0)) rc = 3;
    if (rc != 0) {
        vmap_free(b);
        return rc;
    }
    out = b;
    return 0;
}

// ---- the window moved over the lattice (kss_vmap_shift) --------------------------------------------------------
// lo, inv, leaf and dims stay; base += k.  A voxel of local cell c survives iff 0 <= c_a - k_a < dims_a on all three axes, and its
// lin becomes lin - delta, delta = (k_z * dims_y + k_y) * dims_x + k_x: the survivors keep their relative order, so they stay
// packed in ascending lin and their rec and acc are copied bit for bit.  No pass over the dense table:
//   flag                  one lane per old voxel: its lin decoded into the local cell, the survive flag, and the dropped voxels' N
//                         tallied as a 64-bit integer (a wave shuffle, one integer atomic per wave);
//   scan                  the new numbering; the kept count and the tally go to the host, which makes room in b.spare.  Up to here
//                         the map has only been read;
//   clear                 cell[lin[v]] = -1 for every old voxel, dropped ones included;
//   move                  a launch of its own behind the clear -- one voxel's new cell may be another voxel's old one -- : a
//                         survivor's rec, acc and lin - delta into its new slot, the slot's number into cell[lin - delta].
// The host then swaps the record allocations as the insert does.  Nothing survives: the clear alone, and the map is an empty one.
struct VmapShift {
    int dims[3];
    int k[3];   // clamped to +-dims: a larger shift drops everything just the same
};

__device__ __forceinline__ bool vmap_shift_survives(const VmapShift& s, int64_t lin) {
    const int64_t row = lin / s.dims[0];
    const int cx = (int)(lin - row * s.dims[0]), cz = (int)(row / s.dims[1]), cy = (int)(row - (int64_t)cz * s.dims[1]);
    const int nx = cx - s.k[0], ny = cy - s.k[1], nz = cz - s.k[2];
    return nx >= 0 && nx < s.dims[0] && ny >= 0 && ny < s.dims[1] && nz >= 0 && nz < s.dims[2];
}

__global__ __launch_bounds__(VMAP_THREADS) void vmap_shift_flag_kernel(const int64_t* __restrict__ lin, const double* __restrict__ rec, int64_t nvox,
                                                                        const VmapShift s, int32_t* __restrict__ flag,
                                                                        unsigned long long* __restrict__ tally) {
    unsigned long long dropped = 0;
    for (int64_t v = (int64_t)blockIdx.x * VMAP_THREADS + threadIdx.x; v < nvox; v += (int64_t)gridDim.x * VMAP_THREADS) {
        const bool keep = vmap_shift_survives(s, lin[v]);
        flag[v] = keep ? 1 : 0;
        if (!keep) dropped += (unsigned long long)rec[v * VMAP_NSTAT];   // N: an integer below 2^53
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) dropped += __shfl_down(dropped, off, 64);
    if ((threadIdx.x & 63) == 0 && dropped) atomicAdd(&tally[0], dropped);
}

__global__ __launch_bounds__(VMAP_THREADS) void vmap_shift_clear_kernel(const int64_t* __restrict__ lin, int64_t nvox, int32_t* __restrict__ cell) {
    for (int64_t v = (int64_t)blockIdx.x * VMAP_THREADS + threadIdx.x; v < nvox; v += (int64_t)gridDim.x * VMAP_THREADS) cell[lin[v]] = -1;
}

// num: the exclusive scan of the flags, nvox + 1 entries; a survivor is a voxel the scan steps over
__global__ __launch_bounds__(VMAP_THREADS) void vmap_shift_move_kernel(const int64_t* __restrict__ lin, const double* __restrict__ rec,
                                                                        const double* __restrict__ acc, const int32_t* __restrict__ num, int64_t nvox,
                                                                        int64_t ncells, int64_t delta, int64_t* __restrict__ nlin, double* __restrict__ nrec,
                                                                        double* __restrict__ nacc, int32_t* __restrict__ cell) {
    for (int64_t v = (int64_t)blockIdx.x * VMAP_THREADS + threadIdx.x; v < nvox; v += (int64_t)gridDim.x * VMAP_THREADS) {
        const int64_t w = num[v];
        if (num[v + 1] == w) continue;
        const int64_t to = lin[v] - delta;
        if (to < 0 || to >= ncells) continue;   // (a survivor's new cell is in the window: this only keeps a store inside the table)
#pragma unroll
        for (int a = 0; a < VMAP_NSTAT; ++a) nrec[w * VMAP_NSTAT + a] = rec[v * VMAP_NSTAT + a];
#pragma unroll
        for (int a = 0; a < VMAP_NACC; ++a) nacc[w * VMAP_NACC + a] = acc[v * VMAP_NACC + a];
        nlin[w] = to;
        cell[to] = (int32_t)w;
    }
}

bool vmap_recentre_k(const VmapBuilt& b, const float centre[3], int64_t slack, int64_t k[3]) {
    for (int a = 0; a < 3; ++a) {
        const float f = floorf((centre[a] - b.lo[a]) * b.inv);   // the map's expression
        if (!(fabsf(f) <= 16777216.0f)) return false;            // (a NaN and an infinity included)
        const int64_t d = ((int64_t)f - b.dims[a] / 2) - b.base[a];
        k[a] = (d > slack || -d > slack) ? d : 0;
    }
    return true;
}

int vmap_shift(hipStream_t st, VmapBuilt& b, const int64_t k[3], int64_t counts[VMAP_NSHIFT]) {
    VmapShift s;
    for (int a = 0; a < 3; ++a) {
        s.dims[a] = b.dims[a];
        s.k[a] = (int)std::max<int64_t>(-b.dims[a], std::min<int64_t>(b.dims[a], k[a]));
    }
    const int64_t delta = (k[2] * b.dims[1] + k[1]) * b.dims[0] + k[0];   // (|k_a| <= 2^25 and dims_x * dims_y <= 2^26: below 2^52)
    counts[0] = b.nvox; counts[1] = 0; counts[2] = 0; counts[3] = delta;
    if (k[0] == 0 && k[1] == 0 && k[2] == 0) return 0;
    if (b.nvox == 0) {   // nothing to move: the window alone
        for (int a = 0; a < 3; ++a) b.base[a] += (int)k[a];
        return 0;
    }
    const int64_t ncells = (int64_t)b.dims[0] * b.dims[1] * b.dims[2];
    const int64_t nvox = b.nvox;
    const int nb = stream_blocks(nvox);
    // ---- the scratch; the map is only read until the destination is allocated ----
    VmapScratch w;
    const size_t scan_bytes = scan_scratch_bytes((int)nvox);
    const size_t want = VmapScratch::pad((size_t)nvox * 4) + VmapScratch::pad(((size_t)nvox + 1) * 4) + VmapScratch::pad(scan_bytes) +
                        VmapScratch::pad(sizeof(unsigned long long));
    if (hipMalloc((void**)&w.base, want) != hipSuccess) return 2;
    int32_t* d_flag = w.take<int32_t>((size_t)nvox);
    int32_t* d_num = w.take<int32_t>((size_t)nvox + 1);
    int32_t* d_scan = (int32_t*)w.take<char>(scan_bytes);
    unsigned long long* d_tally = w.take<unsigned long long>(1);
    if (hipMemsetAsync(d_tally, 0, sizeof(unsigned long long), st) != hipSuccess) return 3;
    hipLaunchKernelGGL(vmap_shift_flag_kernel, dim3(nb), dim3(VMAP_THREADS), 0, st, (const int64_t*)b.lin, (const double*)b.rec, nvox, s, d_flag, d_tally);
    launch_scan(st, d_flag, (int)nvox, d_num, d_scan, false);
    int32_t kept32 = 0;
    unsigned long long tally = 0;
    if (hipMemcpyAsync(&kept32, d_num + nvox, sizeof kept32, hipMemcpyDeviceToHost, st) != hipSuccess) return 3;
    if (hipMemcpyAsync(&tally, d_tally, sizeof tally, hipMemcpyDeviceToHost, st) != hipSuccess) return 3;
    if (hipGetLastError() != hipSuccess) return 3;
    if (hipStreamSynchronize(st) != hipSuccess) return 3;
    const int64_t kept = kept32;
    if (kept < 0 || kept > nvox || (int64_t)tally > b.mapped || (kept == nvox) != (tally == 0) || (kept == 0 && (int64_t)tally != b.mapped)) return 3;
    // the destination: the records not in use, grown by the insert's rule where they are too small.  The last allocation, in
    // front of the first store into the map's table
    if (!vmap_reserve(b, kept, std::min<int64_t>(kept + kept / 2, ncells))) return 2;
    // ---- the table at the occupied cells alone (a HIP error from here on leaves a map that is not to be used) ----
    hipLaunchKernelGGL(vmap_shift_clear_kernel, dim3(nb), dim3(VMAP_THREADS), 0, st, (const int64_t*)b.lin, nvox, b.cell);
    VmapBuilt nw;
    if (kept > 0) {
        vmap_pack_at(nw, b.spare, b.spare_cap);
        hipLaunchKernelGGL(vmap_shift_move_kernel, dim3(nb), dim3(VMAP_THREADS), 0, st, (const int64_t*)b.lin, (const double*)b.rec, (const double*)b.acc,
                           (const int32_t*)d_num, nvox, ncells, delta, nw.lin, nw.rec, nw.acc, b.cell);
    }
    if (hipGetLastError() != hipSuccess) return 3;
    if (hipStreamSynchronize(st) != hipSuccess) return 3;   // (the scratch is freed on return)
    if (kept > 0) vmap_swap(b);   // (nothing kept: the records stay where they are, with no voxel in them)
    for (int a = 0; a < 3; ++a) b.base[a] += (int)k[a];
    b.mapped -= (int64_t)tally; b.nvox = kept;
    counts[0] = kept; counts[1] = nvox - kept; counts[2] = (int64_t)tally;
    return 0;
}

// ---- the pyramid: a map whose voxels are k x k x k blocks of another's (kss_vmap_coarsen) ------------------------
// lo stays, leaf' = k * leaf, base'_a = floor(base_a / k), dims'_a = (dims_a + k - 2) / k + 1.  A fine voxel of lattice cell a has
// the parent floor(a / k); a coarse voxel is the serial f64 sum of its children's KEPT sums in ascending fine lin.  No point is
// looked at, and the fine map is only read:
//   flag                  one lane per fine voxel: its lin decoded, its parent's coarse lin, flag[lin'] = 1 (plain stores of the
//                         same value) on a zeroed flag table over the coarse cells;
//   scan                  the exclusive scan of the flags numbers the coarse voxels in ascending lin'; their count goes to the
//                         host, which makes room in the destination's records.  Up to here the destination has only been read;
//   compact               EVERY cell of the coarse table (the voxel's number or -1: what the destination held does not matter) and
//                         lin';
//   merge                 a group of G lanes per coarse voxel: the up to k^3 children in ascending (a_z, a_y, a_x), G look-ups in
//                         the fine cell table at a time, one per lane; then every lane of the group walks the G answers in lane
//                         order (a shuffle each) and adds the occupied children's N, s and P -- all lanes the same additions in the
//                         same order, so the serial sum of the definition is the group's, and lane 0 stores it and the quotients.
// The flags, the numbering and the scan's scratch live in the destination's work area, allocated once for its dims: a refresh of
// a coarse map (kss_vmap_coarsen_into) allocates nothing while the voxel count fits the records it has.
struct VmapCoarse {
    int k;
    int fdims[3], fbase[3];   // the fine map's
    int dims[3], base[3];     // the coarse map's
};

__device__ __forceinline__ int vmap_floor_div(int a, int k) {
    const int q = a / k;
    return (a % k != 0 && a < 0) ? q - 1 : q;
}

__global__ __launch_bounds__(VMAP_THREADS) void vmap_coarsen_flag_kernel(const int64_t* __restrict__ lin, int64_t nvox, const VmapCoarse g,
                                                                          int32_t* __restrict__ flag) {
    for (int64_t v = (int64_t)blockIdx.x * VMAP_THREADS + threadIdx.x; v < nvox; v += (int64_t)gridDim.x * VMAP_THREADS) {
        const int64_t l = lin[v];
        const int64_t row = l / g.fdims[0];
        const int cx = (int)(l - row * g.fdims[0]), cz = (int)(row / g.fdims[1]), cy = (int)(row - (int64_t)cz * g.fdims[1]);
        const int X = vmap_floor_div(g.fbase[0] + cx, g.k) - g.base[0], Y = vmap_floor_div(g.fbase[1] + cy, g.k) - g.base[1],
                  Z = vmap_floor_div(g.fbase[2] + cz, g.k) - g.base[2];
        // (a parent is in the coarse window by the choice of dims': this only keeps a store inside the table)
        if (X < 0 || X >= g.dims[0] || Y < 0 || Y >= g.dims[1] || Z < 0 || Z >= g.dims[2]) continue;
        flag[((int64_t)Z * g.dims[1] + Y) * g.dims[0] + X] = 1;
    }
}

// vox: the exclusive scan of the flags, ncells + 1 entries
__global__ __launch_bounds__(VMAP_THREADS) void vmap_coarsen_compact_kernel(const int32_t* __restrict__ vox, int64_t ncells, int64_t cap,
                                                                             int32_t* __restrict__ cell, int64_t* __restrict__ lin) {
    for (int64_t c = (int64_t)blockIdx.x * VMAP_THREADS + threadIdx.x; c < ncells; c += (int64_t)gridDim.x * VMAP_THREADS) {
        const int32_t v = vox[c];
        const bool occ = vox[c + 1] != v && v < cap;   // (v < cap: the host has made room for the scan's total)
        cell[c] = occ ? v : -1;
        if (occ) lin[v] = c;
    }
}

template <int G>
__global__ __launch_bounds__(VMAP_THREADS) void vmap_coarsen_merge_kernel(const int64_t* __restrict__ lin, int64_t nvox, const VmapCoarse g,
                                                                           const int32_t* __restrict__ fcell, const double* __restrict__ frec,
                                                                           const double* __restrict__ facc, double* __restrict__ rec,
                                                                           double* __restrict__ acc) {
    const int t = threadIdx.x & (G - 1);
    const int nchild = g.k * g.k * g.k;
    const int64_t groups = (int64_t)gridDim.x * (VMAP_THREADS / G);
    for (int64_t v = (int64_t)blockIdx.x * (VMAP_THREADS / G) + threadIdx.x / G; v < nvox; v += groups) {
        const int64_t l = lin[v];
        const int64_t row = l / g.dims[0];
        const int X = (int)(l - row * g.dims[0]), Z = (int)(row / g.dims[1]), Y = (int)(row - (int64_t)Z * g.dims[1]);
        // the first child's local cell in the fine window (it may lie in front of the window: those children do not exist)
        const int x0 = (g.base[0] + X) * g.k - g.fbase[0], y0 = (g.base[1] + Y) * g.k - g.fbase[1], z0 = (g.base[2] + Z) * g.k - g.fbase[2];
        double N = 0.0, s[3] = {0.0, 0.0, 0.0}, P[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int j0 = 0; j0 < nchild; j0 += G) {
            const int j = j0 + t;
            int32_t mine = -1;
            if (j < nchild) {
                const int jz = j / (g.k * g.k), jy = (j - jz * g.k * g.k) / g.k, jx = j - (jz * g.k + jy) * g.k;
                const int cx = x0 + jx, cy = y0 + jy, cz = z0 + jz;
                if (cx >= 0 && cx < g.fdims[0] && cy >= 0 && cy < g.fdims[1] && cz >= 0 && cz < g.fdims[2])
                    mine = fcell[((int64_t)cz * g.fdims[1] + cy) * g.fdims[0] + cx];
            }
#pragma unroll
            for (int u = 0; u < G; ++u) {
                const int64_t fv = __shfl(mine, u, G);
                if (fv < 0) continue;
                N += frec[fv * VMAP_NSTAT];
#pragma unroll
                for (int a = 0; a < 3; ++a) s[a] += facc[fv * VMAP_NACC + a];
#pragma unroll
                for (int a = 0; a < 6; ++a) P[a] += facc[fv * VMAP_NACC + 3 + a];
            }
        }
        if (t != 0) continue;
        double* r = rec + v * VMAP_NSTAT;
        double* q = acc + v * VMAP_NACC;
        r[0] = N;
#pragma unroll
        for (int a = 0; a < 3; ++a) { r[1 + a] = s[a] / N; q[a] = s[a]; }
#pragma unroll
        for (int a = 0; a < 6; ++a) { r[4 + a] = P[a] / N; q[3 + a] = P[a]; }
    }
}

template <int G>
static void launch_coarsen_merge(hipStream_t st, const VmapBuilt& src, const VmapCoarse& g, const VmapBuilt& dst, int64_t nvox) {
    const int64_t blocks = (nvox + VMAP_THREADS / G - 1) / (VMAP_THREADS / G);
    hipLaunchKernelGGL(vmap_coarsen_merge_kernel<G>, dim3((unsigned)std::min<int64_t>(blocks, 1 << 20)), dim3(VMAP_THREADS), 0, st,
                       (const int64_t*)dst.lin, nvox, g, (const int32_t*)src.cell, (const double*)src.rec, (const double*)src.acc, dst.rec, dst.acc);
}

void vmap_coarsen_header(const VmapBuilt& src, int k, double leaf, VmapBuilt& h) {
    for (int a = 0; a < 3; ++a) {
        h.lo[a] = src.lo[a];
        const int q = src.base[a] / k;
        h.base[a] = (src.base[a] % k != 0 && src.base[a] < 0) ? q - 1 : q;
        h.dims[a] = (src.dims[a] + k - 2) / k + 1;
    }
    h.inv = 1.0f / (float)leaf;
}

int vmap_coarsen_table(VmapBuilt& h) {
    const int64_t ncells = (int64_t)h.dims[0] * h.dims[1] * h.dims[2];
    if (hipMalloc((void**)&h.cell, (size_t)ncells * sizeof(int32_t)) != hipSuccess) { h.cell = nullptr; return 2; }
    return 0;
}

int vmap_coarsen_into(hipStream_t st, const VmapBuilt& src, int k, VmapBuilt& dst) {
    VmapCoarse g;
    g.k = k;
    VmapBuilt h;
    vmap_coarsen_header(src, k, 1.0, h);   // (base and dims alone are read from h)
    for (int a = 0; a < 3; ++a) { g.fdims[a] = src.dims[a]; g.fbase[a] = src.base[a]; g.dims[a] = dst.dims[a]; g.base[a] = h.base[a]; }
    const int64_t ncells = (int64_t)dst.dims[0] * dst.dims[1] * dst.dims[2];
    if (src.nvox == 0) {   // an empty map, as vmap_empty leaves one
        if (hipMemsetAsync(dst.cell, 0xff, (size_t)ncells * sizeof(int32_t), st) != hipSuccess) return 3;
        for (int a = 0; a < 3; ++a) dst.base[a] = h.base[a];
        dst.mapped = 0; dst.nvox = 0;
        return 0;
    }
    // ---- the work area: a function of dst's dims alone, so it is allocated by the first fill and kept ----
    const size_t scan_bytes = scan_scratch_bytes((int)ncells);
    const size_t want = VmapScratch::pad((size_t)ncells * 4) + VmapScratch::pad(((size_t)ncells + 1) * 4) + VmapScratch::pad(scan_bytes);
    if (dst.work_bytes < want) {
        void* nw = nullptr;
        if (hipMalloc(&nw, want) != hipSuccess) return 2;
        if (dst.work) (void)hipFree(dst.work);
        dst.work = nw; dst.work_bytes = want;
    }
    VmapScratch w;
    w.base = (char*)dst.work;
    int32_t* d_flag = w.take<int32_t>((size_t)ncells);
    int32_t* d_vox = w.take<int32_t>((size_t)ncells + 1);
    int32_t* d_scan = (int32_t*)w.take<char>(scan_bytes);
    w.base = nullptr;   // (the map's, not this call's to free)
    if (hipMemsetAsync(d_flag, 0, (size_t)ncells * sizeof(int32_t), st) != hipSuccess) return 3;
    hipLaunchKernelGGL(vmap_coarsen_flag_kernel, dim3(stream_blocks(src.nvox)), dim3(VMAP_THREADS), 0, st, (const int64_t*)src.lin, src.nvox, g, d_flag);
    launch_scan(st, d_flag, (int)ncells, d_vox, d_scan, false);
    int32_t nvox32 = 0;
    if (hipMemcpyAsync(&nvox32, d_vox + ncells, sizeof nvox32, hipMemcpyDeviceToHost, st) != hipSuccess) return 3;
    if (hipGetLastError() != hipSuccess) return 3;
    if (hipStreamSynchronize(st) != hipSuccess) return 3;   // the call's one synchronisation
    const int64_t nvox = nvox32;
    if (nvox <= 0 || nvox > src.nvox || nvox > ncells) return 3;
    // the records: the ones in use where they have room, else the ones not in use, else new ones by the insert's rule.  The last
    // allocation, in front of the first store into dst
    if (dst.cap < nvox) {
        if (!vmap_reserve(dst, nvox, std::min<int64_t>(nvox + nvox / 2, ncells))) return 2;
        vmap_swap(dst);
    }
    hipLaunchKernelGGL(vmap_coarsen_compact_kernel, dim3(stream_blocks(ncells)), dim3(VMAP_THREADS), 0, st, (const int32_t*)d_vox, ncells, dst.cap,
                       dst.cell, dst.lin);
    if (k <= 3) launch_coarsen_merge<8>(st, src, g, dst, nvox);    // 8 or 27 children: one or four rounds of 8 look-ups
    else launch_coarsen_merge<64>(st, src, g, dst, nvox);          // 64 .. 512 children: a wave per voxel, one to eight rounds
    if (hipGetLastError() != hipSuccess) return 3;
    for (int a = 0; a < 3; ++a) dst.base[a] = h.base[a];
    dst.mapped = src.mapped; dst.nvox = nvox;
    return 0;
}

}  // namespace kss
