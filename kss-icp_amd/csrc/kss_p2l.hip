// kss_p2l.hip -- point-to-plane correspondence sums (pcl::registration::TransformationEstimationPointToPlaneLLS, PCL 1.8.1;
// the arithmetic is restated in include/kssicp.h at KSS_P2L_NSUMS and in DESIGN.md 2.9):
//   p2l_rows_kernel   one 32-column f64 partial row per workgroup.  Grid of stream_blocks(n) workgroups, lane t of
//                     workgroup b takes the sources b * 256 + t + k * 256 * grid in ORIGINAL index order, then block_sum's
//                     wave tree and fixed wave order.  The bits depend on the source count only (not on the NN engine,
//                     its tuning or the CU count).
//   p2l_final_kernel  one workgroup: fixed-order column sums of those rows, written to host-mapped memory.
// Two launches and no hand-over counter: nothing here has to be zero at rest.
#pragma clang fp contract(off)

#include "kss_device.hpp"

namespace kss {

constexpr int P2L_THREADS = 256;

// Where the current source positions come from: SRC_F3 packed float triples in original order (kss_p2l_sums); SRC_F4 the
// NN pass's float4 output in original order (brute-force engine); SRC_F4_PERM the same in cell order, perm[i] = the slot of
// original source i.
enum { SRC_F3 = 0, SRC_F4 = 1, SRC_F4_PERM = 2 };

// TRIM (trimmed ICP, kss_trim.hip): the threshold is the pass's cut tau, read from device memory where the selection left it
// (-1: no candidate), and a correspondence is kept when 0 <= d2 <= tau; the body and the summation order are the same, so an
// overlap of 1 -- tau = the largest d2 within max_d2 -- gives the untrimmed record bit for bit.
template <int SRC, bool TRIM>
__global__ __launch_bounds__(P2L_THREADS) void p2l_rows_kernel(const float* __restrict__ src3, const float4* __restrict__ src4,
                                                               const int32_t* __restrict__ perm, const int32_t* __restrict__ idx,
                                                               const float* __restrict__ d2_in, const float* __restrict__ tgt,
                                                               const float* __restrict__ nrm, int64_t n, int64_t nt, double max_d2,
                                                               const double* __restrict__ cut_ptr, double* __restrict__ rows) {
    __shared__ double sh[P2L_THREADS / 64][P2L_NSUMS];
    double acc[P2L_NSUMS];
#pragma unroll
    for (int c = 0; c < P2L_NSUMS; ++c) acc[c] = 0.0;
    if constexpr (TRIM) max_d2 = *cut_ptr;
    for (int64_t i = (int64_t)blockIdx.x * P2L_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * P2L_THREADS) {
        const int64_t j = idx[i];
        if (j < 0 || j >= nt) continue;   // (kss_p2l_sums_dev: an index outside the target contributes nothing)
        float sx, sy, sz;
        if constexpr (SRC == SRC_F3) {
            sx = src3[3 * i]; sy = src3[3 * i + 1]; sz = src3[3 * i + 2];
        } else {
            const float4 p = src4[SRC == SRC_F4_PERM ? (int64_t)perm[i] : i];
            sx = p.x; sy = p.y; sz = p.z;
        }
        const float qx = tgt[3 * j], qy = tgt[3 * j + 1], qz = tgt[3 * j + 2];
        const float nx = nrm[3 * j], ny = nrm[3 * j + 1], nz = nrm[3 * j + 2];
        const double d2 = (double)(d2_in ? d2_in[i] : dist2<false>(sx, sy, sz, qx, qy, qz));
        acc[29] += d2;
        // PCL: `if (distance > max_dist_sqr) continue;`, and a correspondence whose normal is not finite is dropped
        if ((TRIM ? d2 >= 0.0 && d2 <= max_d2 : !(d2 > max_d2)) && isfinite(nx) && isfinite(ny) && isfinite(nz)) {
            // float, left to right, no fma (PCL computes these in float and widens)
            const float a = nz * sy - ny * sz;
            const float b = nx * sz - nz * sx;
            const float c = ny * sx - nx * sy;
            const float r = ((nx * qx + ny * qy) + nz * qz) - nx * sx - ny * sy - nz * sz;
            const double v[6] = {(double)a, (double)b, (double)c, (double)nx, (double)ny, (double)nz};
            const double rd = (double)r;
            acc[0] += 1.0;
            int k = 1;
#pragma unroll
            for (int p = 0; p < 6; ++p)
#pragma unroll
                for (int q = p; q < 6; ++q) acc[k++] += v[p] * v[q];
#pragma unroll
            for (int p = 0; p < 6; ++p) acc[22 + p] += v[p] * rd;
            acc[28] += d2;
            acc[30] += rd * rd;
        }
    }
    const double r = block_sum<P2L_NSUMS>(acc, sh);
    if (threadIdx.x < P2L_NSUMS) rows[(int64_t)blockIdx.x * P2L_NSUMS + threadIdx.x] = r;
}

// Column c of the rows: lane (g, c) = (tid / 32, tid % 32) takes rows g, g + 8, g + 16, ... (32 lanes read one 256-byte
// row) into eight accumulators -- row g + 8 (8 m + u) goes to accumulator u while a whole round of eight fits, the tail to
// accumulator 0 -- added as ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7)); then the 8 group totals in group order.
// (Eight loads in flight per lane: with one accumulator the lane waits out one memory latency per row, 12 us at 391 rows.)
// Slot 31 is written as 0.
constexpr int P2L_GROUPS = P2L_THREADS / P2L_NSUMS;
__global__ __launch_bounds__(P2L_THREADS) void p2l_final_kernel(const double* __restrict__ rows, int nrows, double* __restrict__ out) {
    __shared__ double shg[P2L_GROUPS][P2L_NSUMS];
    const int g = threadIdx.x / P2L_NSUMS, c = threadIdx.x % P2L_NSUMS;
    constexpr int G = P2L_GROUPS;
    double a[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int k = g;
    for (; k + 7 * G < nrows; k += 8 * G) {
#pragma unroll
        for (int u = 0; u < 8; ++u) a[u] += rows[(int64_t)(k + u * G) * P2L_NSUMS + c];
    }
    for (; k < nrows; k += G) a[0] += rows[(int64_t)k * P2L_NSUMS + c];
    shg[g][c] = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
    __syncthreads();
    if (threadIdx.x < P2L_NSUMS) {
        double v = 0.0;
        for (int gg = 0; gg < P2L_GROUPS; ++gg) v += shg[gg][threadIdx.x];
        out[threadIdx.x] = threadIdx.x == P2L_NSUMS - 1 ? 0.0 : v;
    }
}

// perm[orig] = k for the cell-ordered sources of a cell-list plan (.w of the packed source = original index)
__global__ __launch_bounds__(256) void p2l_perm_kernel(const float4* __restrict__ src, int64_t n, int32_t* __restrict__ perm) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
        const int oi = __float_as_int(src[k].w);
        if (oi >= 0 && oi < n) perm[oi] = (int32_t)k;
    }
}

__global__ __launch_bounds__(256) void f64_to_f32_kernel(const double* __restrict__ in, int64_t n, float* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) out[i] = (float)in[i];
}

int p2l_rows_blocks(int64_t n) { return stream_blocks(n); }

void launch_p2l_sums(hipStream_t st, const float* d_src3, const float4* d_src4, const int32_t* d_perm, const int32_t* d_idx,
                     const float* d_d2, const float* d_tgt3, const float* d_nrm3, int64_t n, int64_t nt, double max_d2,
                     double* d_rows, double* d_out, const double* d_cut) {
    const int nb = p2l_rows_blocks(n);
    const dim3 g(nb), b(P2L_THREADS);
#define KSS_P2L_ROWS(SRC, TRIM) \
    hipLaunchKernelGGL((p2l_rows_kernel<SRC, TRIM>), g, b, 0, st, d_src3, d_src4, d_perm, d_idx, d_d2, d_tgt3, d_nrm3, n, nt, max_d2, d_cut, d_rows)
    if (d_cut) {   // trimmed: d_d2 is the NN pass's output
        if (d_src3) KSS_P2L_ROWS(SRC_F3, true);
        else if (d_perm) KSS_P2L_ROWS(SRC_F4_PERM, true);
        else KSS_P2L_ROWS(SRC_F4, true);
    } else {
        if (d_src3) KSS_P2L_ROWS(SRC_F3, false);
        else if (d_perm) KSS_P2L_ROWS(SRC_F4_PERM, false);
        else KSS_P2L_ROWS(SRC_F4, false);
    }
#undef KSS_P2L_ROWS
    hipLaunchKernelGGL(p2l_final_kernel, dim3(1), dim3(P2L_THREADS), 0, st, (const double*)d_rows, nb, d_out);
}

void launch_p2l_perm(hipStream_t st, const float4* d_src, int64_t n, int32_t* d_perm) {
    hipLaunchKernelGGL(p2l_perm_kernel, dim3(stream_blocks(n)), dim3(256), 0, st, d_src, n, d_perm);
}

void launch_f64_to_f32(hipStream_t st, const double* d_in, int64_t n, float* d_out) {
    if (n <= 0) return;
    hipLaunchKernelGGL(f64_to_f32_kernel, dim3(stream_blocks(n)), dim3(256), 0, st, d_in, n, d_out);
}

}  // namespace kss
