// kss_p2l.hip -- point-to-plane correspondence sums (pcl::registration::TransformationEstimationPointToPlaneLLS, PCL 1.8.1;
// the arithmetic is restated in include/kssicp.h at KSS_P2L_NSUMS and in DESIGN.md 2.9):
//   p2l_rows_kernel   one 32-column f64 partial row per workgroup.  Grid of stream_blocks(n) workgroups, lane t of
//                     workgroup b takes the sources b * 256 + t + k * 256 * grid in ORIGINAL index order, then block_sum's
//                     wave tree and fixed wave order.  The bits depend on the source count only (not on the NN engine,
//                     its tuning or the CU count).
//   p2l_final_kernel  one workgroup: fixed-order column sums of those rows, written to host-mapped memory.
// Two launches and no hand-over counter: nothing here has to be zero at rest.
#pragma clang fp contract(off)

#include "kss_pair_device.hpp"

namespace kss {

// SRC: where the source positions come from; TRIM (trimmed ICP, kss_trim.hip): the threshold is the pass's cut tau, read from
// device memory where the selection left it.  The per-source body is p2l_source (kss_pair_device.hpp), shared with the batch.
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
    for (int64_t i = (int64_t)blockIdx.x * P2L_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * P2L_THREADS)
        p2l_source<SRC, TRIM>(acc, src3, src4, perm, idx, d2_in, tgt, nrm, i, nt, max_d2);   // (kss_pair_device.hpp)
    const double r = block_sum<P2L_NSUMS>(acc, sh);
    if (threadIdx.x < P2L_NSUMS) rows[(int64_t)blockIdx.x * P2L_NSUMS + threadIdx.x] = r;
}

// the rows' column sums in p2l_rows_column_sum's fixed order (kss_pair_device.hpp); slot 31 is written as 0
__global__ __launch_bounds__(P2L_THREADS) void p2l_final_kernel(const double* __restrict__ rows, int nrows, double* __restrict__ out) {
    __shared__ double shg[P2L_GROUPS][P2L_NSUMS];
    const double v = p2l_rows_column_sum(rows, nrows, shg);
    if (threadIdx.x < P2L_NSUMS) out[threadIdx.x] = threadIdx.x == P2L_NSUMS - 1 ? 0.0 : v;
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

// the final launch alone, for a rows kernel of another translation unit (kss_gicp.hip)
void launch_p2l_final(hipStream_t st, const double* d_rows, int nrows, double* d_out) {
    hipLaunchKernelGGL(p2l_final_kernel, dim3(1), dim3(P2L_THREADS), 0, st, d_rows, nrows, d_out);
}

void launch_p2l_perm(hipStream_t st, const float4* d_src, int64_t n, int32_t* d_perm) {
    hipLaunchKernelGGL(p2l_perm_kernel, dim3(stream_blocks(n)), dim3(256), 0, st, d_src, n, d_perm);
}

void launch_f64_to_f32(hipStream_t st, const double* d_in, int64_t n, float* d_out) {
    if (n <= 0) return;
    hipLaunchKernelGGL(f64_to_f32_kernel, dim3(stream_blocks(n)), dim3(256), 0, st, d_in, n, d_out);
}

}  // namespace kss
