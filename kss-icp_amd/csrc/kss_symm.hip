// kss_symm.hip -- symmetric ICP (point-to-plane on the sum of both normals, Rusinkiewicz 2019; the definition at kss_icp_symm in
// include/kssicp.h): the correspondence sums of one pass.
//   symm_rows_kernel  gicp_rows_kernel's shape: one 32-column f64 partial row per workgroup, p2l_rows_blocks(n) workgroups of 256
//                     lanes, lane t of workgroup b takes the sources b * 256 + t + k * 256 * grid in ORIGINAL index order (the
//                     source normals are read by that index), then block_sum's wave tree and fixed wave order.
//   p2l_final_kernel  (kss_p2l.hip, unchanged) the fixed-order column sums into host-mapped memory.
// The record has the layout of KSS_P2L_NSUMS and the bits depend on the source count only.  Two launches, no hand-over counter.
#pragma clang fp contract(off)

#include "kss_pair_device.hpp"

namespace kss {

template <int SRC>
__global__ __launch_bounds__(P2L_THREADS) void symm_rows_kernel(const float* __restrict__ src3, const float4* __restrict__ src4,
                                                                const int32_t* __restrict__ perm, const int32_t* __restrict__ idx,
                                                                const float* __restrict__ d2_in, const float* __restrict__ sn,
                                                                const float* __restrict__ tgt, const float* __restrict__ nrm, int64_t n,
                                                                int64_t nt, double max_d2, const GicpRot Rn, int align,
                                                                double* __restrict__ rows) {
    __shared__ double sh[P2L_THREADS / 64][P2L_NSUMS];
    double acc[P2L_NSUMS];
#pragma unroll
    for (int c = 0; c < P2L_NSUMS; ++c) acc[c] = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * P2L_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * P2L_THREADS)
        symm_source<SRC>(acc, src3, src4, perm, idx, d2_in, sn, tgt, nrm, i, nt, max_d2, Rn, align);   // (kss_pair_device.hpp)
    const double r = block_sum<P2L_NSUMS>(acc, sh);
    if (threadIdx.x < P2L_NSUMS) rows[(int64_t)blockIdx.x * P2L_NSUMS + threadIdx.x] = r;
}

void launch_symm_sums(hipStream_t st, const float* d_src3, const float4* d_src4, const int32_t* d_perm, const int32_t* d_idx,
                      const float* d_d2, const float* d_sn3, const float* d_tgt3, const float* d_nrm3, int64_t n, int64_t nt,
                      double max_d2, const float Rn[9], int align, double* d_rows, double* d_out) {
    const int nb = p2l_rows_blocks(n);
    const dim3 g(nb), b(P2L_THREADS);
    GicpRot R;
    for (int k = 0; k < 9; ++k) R.r[k] = Rn ? Rn[k] : (k % 4 == 0 ? 1.0f : 0.0f);
#define KSS_SYMM_ROWS(SRC) \
    hipLaunchKernelGGL((symm_rows_kernel<SRC>), g, b, 0, st, d_src3, d_src4, d_perm, d_idx, d_d2, d_sn3, d_tgt3, d_nrm3, n, nt, max_d2, R, align, d_rows)
    if (d_src3) KSS_SYMM_ROWS(SRC_F3);
    else if (d_perm) KSS_SYMM_ROWS(SRC_F4_PERM);
    else KSS_SYMM_ROWS(SRC_F4);
#undef KSS_SYMM_ROWS
    launch_p2l_final(st, d_rows, nb, d_out);
}

}  // namespace kss
