// kss_vmap.hip -- the voxel map of voxelized generalized ICP (kss_vmap_create): one Gaussian per occupied voxel
// of a target cloud, built once and kept for as many registrations as the caller likes.  The definition is restated at kss_vmap
// in include/kssicp.h; the record of a voxel is a SERIAL f64 sum over its targets in ascending original index, so every bit of it
// is determined by the cloud alone.
//   bounds (2 launches)   the float box of the mapped targets (all six of position and normal finite) and their count: fminf /
//                         fmaxf partials per workgroup, then one workgroup.  dims follow on the host: f is monotone in x, so the
//                         largest f_a is f_a of the largest x_a.
//   count                 every mapped target's cell: its lin, its arrival slot in the cell (an integer atomic; the order of arrival
//                         is undone below) and the cell's occupied flag.
//   scan, compact         the exclusive scan of the flags numbers the occupied cells in ascending lin: the dense table becomes
//                         cell -> voxel (-1: empty), the voxels' lin and counts are packed.
//   scan, scatter         the exclusive scan of the packed counts gives every voxel its slots; a target goes to start + arrival slot.
//   rank fix              every target ranks itself among its voxel's targets by original index (grid_rank_fix_kernel's pattern):
//                         the slots of a voxel now hold its targets in ascending index whatever the atomics did.
//   stats                 one lane per voxel walks its slots: N, sum q, sum n n^T in f64, then the six + three divisions.
// A voxel of N targets costs N^2 index compares in the rank fix (spread over its N lanes) and N dependent f64 additions on one
// lane in the walk: nothing at a few points per voxel, and seconds to minutes for a million-point cloud inside ONE voxel (a leaf
// far larger than the cloud) -- which is not a map anyone registers against.
// No float atomic, nothing fused (fp contraction is off), no workspace of the context: the scratch is allocated here and freed
// before the build returns, and what the map keeps (table, records, lin) is its own.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <limits>

#include "kss_internal.hpp"

namespace kss {

constexpr int VMAP_THREADS = 256;

__device__ __forceinline__ bool vmap_mapped(const float* __restrict__ tgt, const float* __restrict__ nrm, int64_t i, float& x, float& y, float& z) {
    x = tgt[3 * i]; y = tgt[3 * i + 1]; z = tgt[3 * i + 2];
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
        if (!vmap_mapped(tgt, nrm, i, p[0], p[1], p[2])) continue;
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
};

// the cell of a mapped target.  x >= lo and x <= hi give 0 <= f <= dims - 1 (subtraction, multiplication by inv >= 0 and floorf
// are monotone); the clamp only keeps an index inside the table should that reasoning ever be wrong.
__device__ __forceinline__ int32_t vmap_lin(const VmapGrid& g, float x, float y, float z) {
    const float p[3] = {x, y, z};
    int c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float f = floorf((p[a] - g.lo[a]) * g.inv);
        c[a] = f >= 0.0f ? (f < (float)g.dims[a] ? (int)f : g.dims[a] - 1) : 0;
    }
    return (int32_t)(((int64_t)c[2] * g.dims[1] + c[1]) * g.dims[0] + c[0]);   // (below 2^26)
}

__global__ __launch_bounds__(VMAP_THREADS) void vmap_count_kernel(const float* __restrict__ tgt, const float* __restrict__ nrm, int64_t nt,
                                                                   const VmapGrid g, int32_t* __restrict__ lin32, int32_t* __restrict__ slot,
                                                                   int32_t* __restrict__ cnt, int32_t* __restrict__ flag) {
    for (int64_t i = (int64_t)blockIdx.x * VMAP_THREADS + threadIdx.x; i < nt; i += (int64_t)gridDim.x * VMAP_THREADS) {
        float x, y, z;
        if (!vmap_mapped(tgt, nrm, i, x, y, z)) { lin32[i] = -1; continue; }
        const int32_t lin = vmap_lin(g, x, y, z);
        lin32[i] = lin;
        slot[i] = atomicAdd(&cnt[lin], 1);
        flag[lin] = 1;
    }
}

// cnt -> the cell table in place; vox: the exclusive scan of the flags
__global__ __launch_bounds__(VMAP_THREADS) void vmap_compact_kernel(int32_t* __restrict__ cell, const int32_t* __restrict__ vox, int64_t ncells,
                                                                     int64_t* __restrict__ vlin, int32_t* __restrict__ vcnt) {
    for (int64_t c = (int64_t)blockIdx.x * VMAP_THREADS + threadIdx.x; c < ncells; c += (int64_t)gridDim.x * VMAP_THREADS) {
        const int32_t n = cell[c];
        if (n > 0) {
            const int32_t v = vox[c];
            vlin[v] = c;
            vcnt[v] = n;
            cell[c] = v;
        } else {
            cell[c] = -1;
        }
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

// one lane per voxel: the record of the definition, serially in ascending original index
__global__ __launch_bounds__(VMAP_THREADS) void vmap_stats_kernel(const float* __restrict__ tgt, const float* __restrict__ nrm,
                                                                   const int32_t* __restrict__ order, const int32_t* __restrict__ vstart, int64_t nvox,
                                                                   double* __restrict__ rec) {
    for (int64_t v = (int64_t)blockIdx.x * VMAP_THREADS + threadIdx.x; v < nvox; v += (int64_t)gridDim.x * VMAP_THREADS) {
        double s[3] = {0.0, 0.0, 0.0}, P[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        const int32_t lo = vstart[v], hi = vstart[v + 1];
        for (int32_t k = lo; k < hi; ++k) {
            const int64_t i = order[k];
            const double n0 = (double)nrm[3 * i], n1 = (double)nrm[3 * i + 1], n2 = (double)nrm[3 * i + 2];
            s[0] += (double)tgt[3 * i]; s[1] += (double)tgt[3 * i + 1]; s[2] += (double)tgt[3 * i + 2];
            P[0] += n0 * n0; P[1] += n0 * n1; P[2] += n0 * n2;
            P[3] += n1 * n1; P[4] += n1 * n2;
            P[5] += n2 * n2;
        }
        const double N = (double)(hi - lo);
        double* r = rec + v * VMAP_NSTAT;
        r[0] = N;
#pragma unroll
        for (int a = 0; a < 3; ++a) r[1 + a] = s[a] / N;
#pragma unroll
        for (int a = 0; a < 6; ++a) r[4 + a] = P[a] / N;
    }
}

void vmap_free(VmapBuilt& b) {
    if (b.cell) (void)hipFree(b.cell);
    if (b.rec) (void)hipFree(b.rec);
    if (b.lin) (void)hipFree(b.lin);
    b.cell = nullptr; b.rec = nullptr; b.lin = nullptr;
}

// the build's scratch: one allocation, carved into 256-byte aligned parts
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
    VmapGrid g;
    g.inv = inv;
    int64_t ncells = 1;
    for (int a = 0; a < 3; ++a) {
        g.lo[a] = hbox[a] == 0.0f ? 0.0f : hbox[a];   // (a zero origin is +0)
        const float f = floorf((hbox[3 + a] - g.lo[a]) * inv);
        if (!(f >= 0.0f && f < (float)VMAP_MAX_CELLS)) return 1;   // (a NaN included: 0 * inf)
        g.dims[a] = 1 + (int)f;
        ncells *= g.dims[a];
        if (ncells > VMAP_MAX_CELLS) return 1;
    }
    const int64_t mapped = (int64_t)hcnt;
    const int64_t vmax = std::min<int64_t>(mapped, ncells);   // at most this many voxels
    // ---- the table (kept) and the scratch ----
    VmapBuilt b;
    VmapScratch w;
    const size_t scan_bytes = std::max(scan_scratch_bytes((int)ncells), scan_scratch_bytes((int)vmax));
    const size_t want = VmapScratch::pad((size_t)ncells * 4) + VmapScratch::pad(((size_t)ncells + 1) * 4) + VmapScratch::pad(scan_bytes) +
                        4 * VmapScratch::pad((size_t)nt * 4) + VmapScratch::pad((size_t)vmax * 4) + VmapScratch::pad(((size_t)vmax + 1) * 4);
    if (hipMalloc((void**)&b.cell, (size_t)ncells * sizeof(int32_t)) != hipSuccess) return 2;
    if (hipMalloc((void**)&w.base, want) != hipSuccess) { vmap_free(b); return 2; }
    int32_t* d_flag = w.take<int32_t>((size_t)ncells);
    int32_t* d_vox = w.take<int32_t>((size_t)ncells + 1);
    int32_t* d_scan = (int32_t*)w.take<char>(scan_bytes);
    int32_t* d_lin32 = w.take<int32_t>((size_t)nt);
    int32_t* d_slot = w.take<int32_t>((size_t)nt);
    int32_t* d_tmp = w.take<int32_t>((size_t)nt);
    int32_t* d_order = w.take<int32_t>((size_t)nt);
    int32_t* d_vcnt = w.take<int32_t>((size_t)vmax);
    int32_t* d_vstart = w.take<int32_t>((size_t)vmax + 1);
    auto fail = [&](int rc) { vmap_free(b); return rc; };
    if (hipMalloc((void**)&b.lin, (size_t)vmax * sizeof(int64_t)) != hipSuccess) return fail(2);
    if (hipMemsetAsync(b.cell, 0, (size_t)ncells * sizeof(int32_t), st) != hipSuccess) return fail(3);
    if (hipMemsetAsync(d_flag, 0, (size_t)ncells * sizeof(int32_t), st) != hipSuccess) return fail(3);
    hipLaunchKernelGGL(vmap_count_kernel, dim3(nb), dim3(VMAP_THREADS), 0, st, d_tgt, d_nrm, nt, g, d_lin32, d_slot, b.cell, d_flag);
    launch_scan(st, d_flag, (int)ncells, d_vox, d_scan, false);
    hipLaunchKernelGGL(vmap_compact_kernel, dim3(stream_blocks(ncells)), dim3(VMAP_THREADS), 0, st, b.cell, (const int32_t*)d_vox, ncells, b.lin, d_vcnt);
    int32_t nvox32 = 0;
    if (hipMemcpyAsync(&nvox32, d_vox + ncells, sizeof nvox32, hipMemcpyDeviceToHost, st) != hipSuccess) return fail(3);
    if (hipStreamSynchronize(st) != hipSuccess) return fail(3);
    const int64_t nvox = nvox32;
    if (nvox < 1 || nvox > vmax) return fail(3);
    if (hipMalloc((void**)&b.rec, (size_t)nvox * VMAP_NSTAT * sizeof(double)) != hipSuccess) return fail(2);
    launch_scan(st, d_vcnt, (int)nvox, d_vstart, d_scan, false);
    hipLaunchKernelGGL(vmap_scatter_kernel, dim3(nb), dim3(VMAP_THREADS), 0, st, (const int32_t*)d_lin32, (const int32_t*)d_slot, nt,
                       (const int32_t*)b.cell, (const int32_t*)d_vstart, d_tmp);
    hipLaunchKernelGGL(vmap_rank_fix_kernel, dim3(stream_blocks(mapped)), dim3(VMAP_THREADS), 0, st, (const int32_t*)d_tmp, mapped,
                       (const int32_t*)d_lin32, (const int32_t*)b.cell, (const int32_t*)d_vstart, d_order);
    hipLaunchKernelGGL(vmap_stats_kernel, dim3(stream_blocks(nvox)), dim3(VMAP_THREADS), 0, st, d_tgt, d_nrm, (const int32_t*)d_order,
                       (const int32_t*)d_vstart, nvox, b.rec);
    if (hipGetLastError() != hipSuccess) return fail(3);
    if (hipStreamSynchronize(st) != hipSuccess) return fail(3);   // (the scratch is freed on return)
    b.mapped = mapped; b.nvox = nvox;
    for (int a = 0; a < 3; ++a) { b.dims[a] = g.dims[a]; b.lo[a] = g.lo[a]; }
    b.inv = inv;
    out = b;
    return 0;
}

}  // namespace kss
